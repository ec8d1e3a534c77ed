"""What rgbd_odometry and rgbd_odometry_model send over the C ABI, pinned against the recording stand-in for the library
(tests/recording_lib.py; no GPU), in the manner of tests/test_binding_depth_consistency_cpu.py; and VisualOdometryRgbd's composition
of the poses and its lost-frame policy on a stub volume."""
import types

import numpy as np
import pytest

from pyslam_amd import _lib as L
from pyslam_amd import volumetric as V
from pyslam_amd import volumetric_semantic as S
from pyslam_amd.odometry import VisualOdometryRgbd
from tests.recording_lib import ref, volume
from tests.test_binding_calls_cpu import ANY, P, REF, covers, expect, host, refused, shaped, tsdf  # noqa: F401 (host: a fixture)

H, W = 6, 20
CAM = V.PinholeCameraIntrinsic(W, H, 30.0, 31.0, 9.5, 2.5)
FIELDS = ("depth_scale", "depth_min", "depth_max", "depth_outlier_trunc", "depth_huber_delta", "intensity_weight", "intensity_huber_delta",
          "n_levels")
I64 = L.ctypes.c_int64


def frames(u16=False, seed=0):
    rng = np.random.default_rng(seed)
    d = (1.0 + rng.random((2, H, W))).astype(np.float32)
    if u16:
        d = np.rint(d * 1000).astype(np.uint16)
    return d[0], d[1], rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def params(call, index):
    p = ref(call[1][index])
    return dict({f: getattr(p, f) for f in FIELDS}, iterations=tuple(p.iterations))


def test_structs_mirror_the_header():
    """Field order and sizes of the two structs as include/hipvol.h declares them (8-byte alignment, no padding but the tail's)."""
    assert [n for n, _ in L.HvOdometryParams._fields_] == list(FIELDS) + ["iterations"]
    assert L.ctypes.sizeof(L.HvOdometryParams) == 7 * 8 + 4 + 4 * L.HV_TRACK_MAX_LEVELS + 4
    assert [n for n, _ in L.HvOdometryResult._fields_] == ["transformation", "information", "fitness", "inlier_rmse", "inliers", "valid",
                                                         "iterations", "degenerate", "success", "photometric_inliers", "intensity_rmse"]
    assert L.ctypes.sizeof(L.HvOdometryResult) == (16 + 36 + 2) * 8 + 2 * 8 + 4 * L.HV_TRACK_MAX_LEVELS + 2 * 4 + 2 * 8
    assert L.HvOdometryResult.photometric_inliers.offset == L.ctypes.sizeof(L.HvTrackResult)  # the tracker's result, then the two


@covers("rgbd_odometry")
def test_depth_only_defaults_on_every_kind_of_volume(host):
    sd, td, _, _ = frames()
    for vol in (tsdf(), volume(V.VoxelBlockGrid, voxel_size=0.05, block_size=8), volume(S.VoxelBlockSemanticGrid, voxel_size=0.05, block_size=8)):
        out = vol.rgbd_odometry(host(sd), host(td), CAM)
        call, = expect(vol, ("hv_rgbd_odometry", P(sd), P(td), L.HV_DEPTH_F32, None, None, H, W, ANY, None, REF(L.HvOdometryParams),
                             REF(L.HvOdometryResult), None, 0, REF(I64), L.HV_HOST))
        assert params(call, 10) == dict(depth_scale=1.0, depth_min=0.1, depth_max=3.0, depth_outlier_trunc=0.07, depth_huber_delta=0.05,
                                        intensity_weight=0.01, intensity_huber_delta=0.1, n_levels=3, iterations=(10, 5, 4, 0, 0, 0, 0, 0))
        assert isinstance(out, V.OdometryResult) and out.trace is None and out.photometric_inliers is None and out.intensity_rmse is None
        assert out.iterations == (0, 0, 0) and out.success is False and out.transformation.shape == (4, 4)


@covers("rgbd_odometry")
def test_marshals_every_argument_and_the_trace_stride_follows_the_method(host):
    sd, td, sc, tc = frames(u16=True)
    vol = tsdf()
    T0 = np.eye(4)
    T0[:3, 3] = (0.125, 0.25, 0.375)  # exact in float32: the float32 matrix below is sent as these float64 values
    vol._lib.script("hv_rgbd_odometry", 2, peek={9: (np.float64, 16), 8: (np.float64, 4)})
    out = vol.rgbd_odometry(host(sd), host(td), CAM, init=T0.astype(np.float32), source_color=host(sc), target_color=host(tc), depth_scale=1000.0,
                            depth_min=0.2, depth_max=4.0, iterations=(3, 2), depth_outlier_trunc=0.1, depth_huber_delta=0.06,
                            intensity_weight=0.5, intensity_huber_delta=0.2, trace=True)
    call, = expect(vol, ("hv_rgbd_odometry", P(sd), P(td), L.HV_DEPTH_U16, P(sc), P(tc), H, W, ANY, ANY, REF(L.HvOdometryParams),
                         REF(L.HvOdometryResult), ANY, 5, REF(I64), L.HV_HOST))
    assert params(call, 10) == dict(depth_scale=1000.0, depth_min=0.2, depth_max=4.0, depth_outlier_trunc=0.1, depth_huber_delta=0.06,
                                    intensity_weight=0.5, intensity_huber_delta=0.2, n_levels=2, iterations=(3, 2, 0, 0, 0, 0, 0, 0))
    np.testing.assert_array_equal(vol._lib.peeked[-1][9], T0.ravel())
    np.testing.assert_array_equal(vol._lib.peeked[-1][8], [30.0, 31.0, 9.5, 2.5])
    # two rows came back (scripted): hybrid rows carry the two photometric columns; the result has the photometric fields
    assert len(out.trace) == 2 and "photometric_inliers" in out.trace[0] and out.photometric_inliers == 0 and out.intensity_rmse == 0.0
    assert out.iterations == (0, 0)
    # depth only with a trace: the tracker's 56-column rows
    vol = tsdf()
    vol._lib.script("hv_rgbd_odometry", 1)
    out = vol.rgbd_odometry(sd, td, CAM, depth_scale=1000.0, iterations=(3, 2, 1), trace=True)
    expect(vol, ("hv_rgbd_odometry", P(sd), P(td), L.HV_DEPTH_U16, None, None, H, W, ANY, None, REF(L.HvOdometryParams),
                 REF(L.HvOdometryResult), ANY, 6, REF(I64), L.HV_HOST))
    assert len(out.trace) == 1 and "photometric_inliers" not in out.trace[0]
    # a float64 depth is sent as float32, a strided one contiguous
    wide = np.ones((H, 2 * W))
    vol.rgbd_odometry(wide[:, ::2], wide[:, 1::2], CAM)
    expect(vol, ("hv_rgbd_odometry", ANY, ANY, L.HV_DEPTH_F32, None, None, H, W, ANY, None, REF(L.HvOdometryParams), REF(L.HvOdometryResult),
                 None, 0, REF(I64), L.HV_HOST))


def test_trace_buffers_have_the_strides_of_the_header():
    """The row buffer handed over holds steps x stride doubles: 56 per row depth only, 58 hybrid (rows beyond it would be cut)."""
    sd, td, sc, tc = frames()
    vol = tsdf()
    for kw, stride in ((dict(), L.HV_TRACK_TRACE_STRIDE), (dict(source_color=sc, target_color=tc), L.HV_TRACK_COLOR_TRACE_STRIDE)):
        vol._lib.script("hv_rgbd_odometry", 3, peek={12: (np.float64, 3 * stride)})
        out = vol.rgbd_odometry(sd, td, CAM, iterations=(2, 1), trace=True, **kw)
        expect(vol, ("hv_rgbd_odometry", ANY, ANY, L.HV_DEPTH_F32, ANY if kw else None, ANY if kw else None, H, W, ANY, None,
                     REF(L.HvOdometryParams), REF(L.HvOdometryResult), ANY, 3, REF(I64), L.HV_HOST))
        assert len(out.trace) == 3 and (stride, len(vol._lib.peeked[-1][12])) in ((56, 168), (58, 174))


@covers("rgbd_odometry")
def test_refusals_come_before_any_call():
    sd, td, sc, tc = frames()
    vol = tsdf()
    call = vol.rgbd_odometry
    refused(vol, ValueError, "give both source_color and target_color", call, sd, td, CAM, source_color=sc)
    refused(vol, ValueError, "give both source_color and target_color", call, sd, td, CAM, target_color=tc)
    refused(vol, ValueError, "source_depth is (6, 20), target_depth is (6, 19): the two frames must have the same shape", call, sd, td[:, :-1], CAM)
    refused(vol, ValueError, "source_depth is uint16, target_depth is float32: the two frames must have the same dtype", call,
            (sd * 1000).astype(np.uint16), td, CAM)
    refused(vol, RuntimeError, V._UNSUPPORTED_IMAGE, call, sd[:-1], td[:-1], CAM)  # not the camera's size
    refused(vol, RuntimeError, V._UNSUPPORTED_IMAGE, call, sd, td, CAM, source_color=sc, target_color=tc[:, :-1])
    refused(vol, RuntimeError, V._UNSUPPORTED_IMAGE, call, sd, td, CAM, source_color=sc.astype(np.float32), target_color=tc)
    for bad in (np.full((4, 4), np.nan), np.diag([1.0, 1.0, 1.0, np.inf]), np.ones((4, 4))):
        refused(vol, ValueError, "init must be a finite rigid 4x4 with bottom row 0 0 0 1", call, sd, td, CAM, init=bad)
    refused(vol, RuntimeError, "4x4", call, sd, td, CAM, init=np.eye(3))
    assert vol._lib.calls == []


def test_frames_in_different_places_are_refused():
    torch = pytest.importorskip("torch")
    sd, td, _, _ = frames()

    class OnGpu:  # a tensor that says it lives on a GPU: the check reads is_cuda and device only
        is_cuda, device, dtype, shape = True, "cuda:0", torch.float32, (H, W)

        def data_ptr(self):
            return 64

        def contiguous(self):
            return self

        def to(self, dtype):
            return self

    vol = tsdf()
    refused(vol, ValueError, "source_depth lives on cuda:0, target_depth on the host: the two frames must live in the same place",
            vol.rgbd_odometry, OnGpu(), td, CAM)


@covers("rgbd_odometry_model")
def test_model_call(host):
    d, _, c, _ = frames()
    vol = tsdf()
    out = vol.rgbd_odometry_model(host(d), CAM, level=1, depth_scale=2.0, depth_min=0.3, depth_max=5.0, depth_outlier_trunc=0.2)
    call, = expect(vol, ("hv_rgbd_odometry_model", P(d), L.HV_DEPTH_F32, None, H, W, ANY, REF(L.HvOdometryParams), 1, P(out["depth"]),
                         P(out["normal"]), P(out["mask"]), None, L.HV_HOST))
    p = params(call, 7)
    assert (p["depth_scale"], p["depth_min"], p["depth_max"], p["depth_outlier_trunc"]) == (2.0, 0.3, 5.0, 0.2)
    shaped(out["depth"], (3, 10), np.float32), shaped(out["normal"], (3, 10, 3), np.float32), shaped(out["mask"], (3, 10), np.bool_)
    assert out["record"] is None
    out = vol.rgbd_odometry_model(host(d), CAM, color=host(c))
    expect(vol, ("hv_rgbd_odometry_model", P(d), L.HV_DEPTH_F32, P(c), H, W, ANY, REF(L.HvOdometryParams), 0, P(out["depth"]), P(out["normal"]),
                 P(out["mask"]), P(out["record"]), L.HV_HOST))
    shaped(out["record"], (H, W, 4), np.float32)
    refused(vol, ValueError, "a 6x20 frame has no pyramid level 3", vol.rgbd_odometry_model, d, CAM, level=3)
    refused(vol, ValueError, "no pyramid level -1", vol.rgbd_odometry_model, d, CAM, level=-1)
    refused(vol, RuntimeError, V._UNSUPPORTED_IMAGE, vol.rgbd_odometry_model, d, CAM, color=c[:-1])


class StubVolume:
    """rgbd_odometry that records its operands and answers with scripted results."""

    def __init__(self, results):
        self.calls, self.results = [], list(results)

    def rgbd_odometry(self, source_depth, target_depth, intrinsic, **kw):
        self.calls.append((source_depth, target_depth, intrinsic, kw))
        return self.results.pop(0)


def result(T, success=True):
    return V.OdometryResult(T, 0.9, 0.001, np.eye(6), success, (1, 1, 1), 0, 100, 110)


def step(tx, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0, tx], [s, c, 0, 0.0], [0, 0, 1, 0.01], [0, 0, 0, 1.0]])


def test_stream_class_composes_poses_and_keeps_the_pose_of_a_lost_frame():
    cam = types.SimpleNamespace(fx=30.0, fy=31.0, cx=9.5, cy=2.5, width=W, height=H)
    T1, T2, T3 = step(0.1, 5.0), step(-0.2, 10.0), step(0.3, -3.0)
    vol = StubVolume([result(T1), result(T2, success=False), result(T3)])
    T0 = step(1.0, 30.0)
    vo = VisualOdometryRgbd(vol, cam, method="hybrid", keep_on_device=False, T_wc0=T0, iterations=(4, 2), intensity_weight=0.1)
    depth = [np.full((H, W), 1.0 + i, np.float32) for i in range(4)]
    color = [np.full((H, W, 3), i, np.uint8) for i in range(4)]
    assert np.array_equal(vo.track(color[0], depth[0]), T0) and vol.calls == [] and not vo.lost and vo.last_result is None
    assert np.array_equal(vo.track(color[1], depth[1]), T0 @ T1) and not vo.lost
    assert np.array_equal(vo.track(color[2], depth[2]), T0 @ T1) and vo.lost and vo.last_result.success is False  # the pose stays
    assert np.array_equal(vo.track(color[3], depth[3]), (T0 @ T1) @ T3) and not vo.lost and vo.frames == 4
    # each frame is the SOURCE against the previous frame as TARGET - the lost one included - from an identity start
    for k, (sd, td, K, kw) in enumerate(vol.calls):
        assert sd is depth[k + 1] and td is depth[k] and kw["source_color"] is color[k + 1] and kw["target_color"] is color[k]
        assert "init" not in kw and kw["iterations"] == (4, 2) and kw["intensity_weight"] == 0.1
        assert (K.width, K.height) == (W, H) and list(K.as_array()) == [30.0, 31.0, 9.5, 2.5]
    # point_to_plane sends no colour and takes None for it; the first pose defaults to the identity
    vol = StubVolume([result(T1)])
    vo = VisualOdometryRgbd(vol, cam, method="point_to_plane", keep_on_device=False)
    assert np.array_equal(vo.track(None, depth[0]), np.eye(4)) and np.array_equal(vo.track(color[1], depth[1]), T1)
    assert vol.calls[0][3] == dict(source_color=None, target_color=None)
    with pytest.raises(ValueError, match="method must be one of"):
        VisualOdometryRgbd(vol, cam, method="icp")
    with pytest.raises(ValueError, match="needs the colour image"):
        VisualOdometryRgbd(vol, cam, keep_on_device=False).track(None, depth[0])


def test_stream_class_sends_what_rgbd_odometry_takes():
    """On the recording library: a valid hv_rgbd_odometry call per frame after the first; an unsuccessful result (the stand-in
    fills nothing) marks every frame lost and keeps the identity."""
    cam = types.SimpleNamespace(fx=30.0, fy=31.0, cx=9.5, cy=2.5, width=W, height=H)
    vol = tsdf()
    vo = VisualOdometryRgbd(vol, cam, keep_on_device=False)
    sd, td, sc, tc = frames()
    vo.track(tc, td)
    assert vol._lib.calls == []
    T = vo.track(sc, sd)
    expect(vol, ("hv_rgbd_odometry", P(sd), P(td), L.HV_DEPTH_F32, P(sc), P(tc), H, W, ANY, None, REF(L.HvOdometryParams),
                 REF(L.HvOdometryResult), None, 0, REF(I64), L.HV_HOST))
    assert vo.lost and np.array_equal(T, np.eye(4))
