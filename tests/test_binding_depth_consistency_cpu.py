"""What filter_depth_consistency sends over the C ABI, pinned against the recording stand-in for the library (tests/recording_lib.py; no
GPU), in the manner of tests/test_binding_mvs_cpu.py; prep.consistency_views; DepthEstimatorMvs's raw depths, its choice of the views
to check against and its skips on a stub volume; and the dense front's four parameters."""
import types

import numpy as np
import pytest

from pyslam_amd import _lib as L
from pyslam_amd import volumetric as V
from pyslam_amd import volumetric_semantic as S
from pyslam_amd.prep import consistency_views, plane_sweep_views
from tests.recording_lib import ref, volume
from tests.test_binding_calls_cpu import ANY, P, REF, covers, expect, host, refused, shaped, tsdf  # noqa: F401 (host: a fixture)

H, W = 6, 20
FIELDS = ("max_reproj_error", "inv_depth_tol", "rel_depth_tol", "min_consistent", "max_violations", "fuse")
VIEWS = np.array([[[1, 0, 0, -1], [0, 1, 0, 0], [0, 0, 1, 0]], [[1, 0, 0, 2], [0, 1, 0, 0.5], [0, 0, 1, 0.25]]], np.float32)
BACK = np.array([[[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 1, 0]], [[1, 0, 0, -2], [0, 1, 0, -0.5], [0, 0, 1, -0.25]]], np.float32)
PEEK = {6: (np.float32, 24), 7: (np.float32, 24)}


def depths(n=2, seed=0):
    rng = np.random.default_rng(seed)
    return (1.0 + rng.random((H, W))).astype(np.float32), (1.0 + rng.random((n, H, W))).astype(np.float32)


def params(call):
    p = ref(call[1][8])
    return {f: getattr(p, f) for f in FIELDS}


def pose(tx=0.0, ty=0.0, tz=0.0):
    T = np.eye(4)
    T[:3, 3] = (tx, ty, tz)
    return T


@covers("filter_depth_consistency")
def test_defaults_and_result_kinds():
    depth, sources = depths()
    for vol in (tsdf(), volume(V.VoxelBlockGrid, voxel_size=0.05, block_size=8), volume(S.VoxelBlockSemanticGrid, voxel_size=0.05, block_size=8)):
        vol._lib.script("hv_depth_consistency", peek=PEEK)
        out, counts = vol.filter_depth_consistency(depth, sources, VIEWS, BACK)
        call, = expect(vol, ("hv_depth_consistency", P(depth), P(sources), 2, H, W, ANY, ANY, REF(L.HvConsistencyParams), P(out), None, None, L.HV_HOST))
        shaped(out, (H, W), np.float32)
        assert counts is None
        assert params(call) == dict(max_reproj_error=1.0, inv_depth_tol=0.0, rel_depth_tol=np.float32(0.01), min_consistent=1, max_violations=0, fuse=1)
        np.testing.assert_array_equal(vol._lib.peeked[-1][6], VIEWS.ravel())
        np.testing.assert_array_equal(vol._lib.peeked[-1][7], BACK.ravel())


@covers("filter_depth_consistency")
def test_marshals_every_argument(host):
    depth, sources = depths(3)
    vol = tsdf()
    vol._lib.script("hv_depth_consistency", peek={1: (np.float32, H * W), 2: (np.float32, 3 * H * W), 6: (np.float32, 36), 7: (np.float32, 36)})
    views, back = np.concatenate([VIEWS, VIEWS[:1] * 2]), np.concatenate([BACK, BACK[:1] * 2])
    result = vol.filter_depth_consistency(host(depth), [host(s) for s in sources], host(views), host(back), max_reproj_error=0.75, inv_depth_tol=0.125,
                                          rel_depth_tol=0.5, min_consistent=3, max_violations=2, fuse=False, counts=True, stats=True)
    out, counts, stats = result
    call, = expect(vol, ("hv_depth_consistency", P(depth), ANY, 3, H, W, ANY, ANY, REF(L.HvConsistencyParams), P(out), P(counts),
                         REF(L.HvConsistencyStats), L.HV_HOST))
    shaped(out, (H, W), np.float32), shaped(counts, (H, W, 4), np.uint8)  # host operands of either kind: numpy results
    assert params(call) == dict(max_reproj_error=0.75, inv_depth_tol=0.125, rel_depth_tol=0.5, min_consistent=3, max_violations=2, fuse=0)
    assert all(type(x) is int for x in call[1][3:6]) and call[1][12] == L.HV_HOST
    assert isinstance(stats, V.ConsistencyStats) and stats == V.ConsistencyStats()
    assert V.ConsistencyStats.__slots__ == tuple(name for name, _ in L.HvConsistencyStats._fields_)
    assert V._stats(V.ConsistencyStats, L.HvConsistencyStats(100, 101, 102)).as_tuple() == (100, 101, 102)
    # a list of sources is sent as one contiguous block, in order; the matrices as float32 [N,3,4]
    np.testing.assert_array_equal(vol._lib.peeked[-1][1], depth.ravel())
    np.testing.assert_array_equal(vol._lib.peeked[-1][2], sources.ravel())
    np.testing.assert_array_equal(vol._lib.peeked[-1][6], views.ravel())
    np.testing.assert_array_equal(vol._lib.peeked[-1][7], back.ravel())
    # strided views are made contiguous for the call; numpy integers are plain ints by then; float64 matrices are rounded
    wide = np.ones((H, 2 * W), np.float32)
    out, counts = vol.filter_depth_consistency(wide[:, ::2], wide[None, :, 1::2], VIEWS[:1].astype(np.float64), BACK[:1].astype(np.float64),
                                               min_consistent=np.int64(0), max_violations=np.int32(1), counts=True)
    call, = expect(vol, ("hv_depth_consistency", ANY, ANY, 1, H, W, ANY, ANY, REF(L.HvConsistencyParams), P(out), P(counts), None, L.HV_HOST))
    assert params(call)["min_consistent"] == 0 and params(call)["max_violations"] == 1 and params(call)["fuse"] == 1
    np.testing.assert_array_equal(vol._lib.peeked[-1][6][:12], VIEWS[0].ravel())


@covers("filter_depth_consistency")
def test_views_from_poses():
    depth, sources = depths()
    vol = tsdf()
    vol._lib.script("hv_depth_consistency", peek=PEEK)
    K = V.PinholeCameraIntrinsic(W, H, 30.0, 31.0, 9.5, 2.5)
    T_ref, T_src = pose(0.1, 0.0, 0.2), np.stack([pose(0.0, 0.05, 0.2), pose(0.3, 0.0, 0.1)])
    want, want_back = consistency_views(K, T_ref, K, T_src)
    np.testing.assert_array_equal(want, plane_sweep_views(K, T_ref, K, T_src))
    for s in range(2):
        np.testing.assert_array_equal(want_back[s], plane_sweep_views(K, T_src[s], K, T_ref)[0])
    assert want_back.shape == (2, 3, 4) and want_back.dtype == np.float32 and want_back.flags.c_contiguous
    for intrinsic in (K, (30.0, 31.0, 9.5, 2.5), np.array([[30.0, 0, 9.5], [0, 31.0, 2.5], [0, 0, 1]])):
        vol.filter_depth_consistency(depth, sources, intrinsic=intrinsic, T_ref=T_ref, T_sources=T_src)
        expect(vol, ("hv_depth_consistency", P(depth), P(sources), 2, H, W, ANY, ANY, REF(L.HvConsistencyParams), ANY, None, None, L.HV_HOST))
        np.testing.assert_array_equal(vol._lib.peeked[-1][6], want.ravel())
        np.testing.assert_array_equal(vol._lib.peeked[-1][7], want_back.ravel())
    # a pure translation along x by t: A = I, b = (fx t, 0, 0) there and (-fx t, 0, 0) back; one camera per source
    m, b = consistency_views(K, pose(), [K, (60.0, 62.0, 9.5, 2.5)], np.stack([pose(-0.5), pose(-0.5)]))
    np.testing.assert_allclose(m[0], [[1, 0, 0, -15.0], [0, 1, 0, 0], [0, 0, 1, 0]], atol=1e-6)
    np.testing.assert_allclose(b[0], [[1, 0, 0, 15.0], [0, 1, 0, 0], [0, 0, 1, 0]], atol=1e-6)
    np.testing.assert_allclose(b[1], [[0.5, 0, 4.75, 15.0], [0, 0.5, 1.25, 0], [0, 0, 1, 0]], atol=1e-6)
    call = lambda *a, **kw: vol.filter_depth_consistency(depth, sources, *a, **kw)
    either = "pass either views and back_views or intrinsic"
    refused(vol, ValueError, either, call)
    refused(vol, ValueError, either, call, want)
    refused(vol, ValueError, either, call, back_views=want_back)
    refused(vol, ValueError, either, call, want, want_back, intrinsic=K)
    refused(vol, ValueError, either, call, want, want_back, T_ref=T_ref)
    refused(vol, ValueError, "intrinsic needs the poses", call, intrinsic=K, T_ref=T_ref)
    refused(vol, ValueError, "views must be [2, 3, 4]", call, intrinsic=K, T_ref=T_ref, T_sources=T_src[:1])


@covers("filter_depth_consistency")
def test_refusals_come_before_any_call():
    depth, sources = depths()
    vol = tsdf()
    call = lambda *a, **kw: vol.filter_depth_consistency(*(a or (depth, sources, VIEWS, BACK)), **kw)
    for bad in (-1.0, np.nan, np.inf, 1e39):
        refused(vol, ValueError, "max_reproj_error must be finite and not negative", call, max_reproj_error=bad)
        refused(vol, ValueError, "the depth tolerances must be finite and not negative", call, inv_depth_tol=bad)
        refused(vol, ValueError, "the depth tolerances must be finite and not negative", call, rel_depth_tol=bad)
    refused(vol, ValueError, "one of inv_depth_tol and rel_depth_tol must be positive", call, inv_depth_tol=0.0, rel_depth_tol=0.0)
    refused(vol, ValueError, "one of inv_depth_tol and rel_depth_tol must be positive", call, inv_depth_tol=1e-60, rel_depth_tol=0.0)  # 0 as float32
    for bad in (-1, 3, 1.5):
        refused(vol, ValueError, "min_consistent must be in 0..2", call, min_consistent=bad)
        refused(vol, ValueError, "max_violations must be in 0..2", call, max_violations=bad)
    for bad in (np.nan, np.inf):
        m = VIEWS.copy()
        m[1, 0, 3] = bad
        refused(vol, ValueError, "a view matrix entry is not finite", call, depth, sources, m, BACK)
        refused(vol, ValueError, "a view matrix entry is not finite", call, depth, sources, VIEWS, m)
    refused(vol, ValueError, "filter_depth_consistency: views must be [2, 3, 4]", call, depth, sources, VIEWS[:1], BACK)
    refused(vol, ValueError, "filter_depth_consistency: back_views must be [2, 3, 4]", call, depth, sources, VIEWS, BACK[:1])
    refused(vol, ValueError, "filter_depth_consistency: views must be [2, 3, 4]", call, depth, sources, VIEWS.reshape(2, 4, 3), BACK)
    refused(vol, ValueError, "need 1..4 source views, got 5", call, depth, np.ones((5, H, W), np.float32), np.tile(VIEWS[:1], (5, 1, 1)), np.tile(BACK[:1], (5, 1, 1)))
    refused(vol, ValueError, "must live in the same place", call, depth, [], VIEWS, BACK)
    refused(vol, ValueError, "bad image size", call, depth[:0], sources[:, :0], VIEWS, BACK)
    refused(vol, ValueError, "bad image size", call, depth[:, :0], sources[:, :, :0], VIEWS, BACK)
    refused(vol, ValueError, "depth maps of the reference's shape", call, depth, sources[:, :, :-1], VIEWS, BACK)
    refused(vol, ValueError, "depth maps of the reference's shape", call, depth, [sources[0], sources[1][:-1]], VIEWS, BACK)
    refused(vol, ValueError, "depth maps of the reference's shape", call, depth, sources[0], VIEWS[:1], BACK[:1])
    refused(vol, ValueError, "depth maps of the reference's shape", call, depth[None], sources[None], VIEWS, BACK)
    refused(vol, ValueError, "the depth maps must be float32", call, depth.astype(np.float64), sources, VIEWS, BACK)
    refused(vol, ValueError, "the depth maps must be float32", call, depth, (1000 * sources).astype(np.uint16), VIEWS, BACK)
    assert vol._lib.calls == []


class StubVolume:
    """multiview_sgm and filter_depth_consistency that record their arguments and answer with arrays of the right kind."""

    def __init__(self):
        self.calls = []

    def multiview_sgm(self, ref, sources, views=None, **kw):
        self.calls.append(("mvs", ref, list(sources), kw))
        return np.full(ref.shape[:2], 16, np.int16), np.full(ref.shape[:2], float(ref[0, 0, 0]), np.float32)  # the raw depth names its frame

    def filter_depth_consistency(self, depth, source_depths, views=None, back_views=None, **kw):
        self.calls.append(("check", depth, list(source_depths), kw))
        return depth + 0.5, (np.zeros(depth.shape + (4,), np.uint8) if kw.get("counts") else None)


def frame(i):
    return np.full((H, W, 3), i, np.uint8)


CAM = types.SimpleNamespace(fx=30.0, fy=31.0, cx=9.5, cy=2.5)


def test_depth_estimator_mvs_checks_against_the_raw_depths_of_its_sources():
    from pyslam_amd.depth_estimation import DepthEstimatorMvs

    vol = StubVolume()
    est = DepthEstimatorMvs(vol, CAM, keep_on_device=False, min_depth=0.5, max_depth=4.0, max_sources=2, min_baseline=0.125, max_baseline=0.5,
                            ring_size=4, num_planes=29, consistency_min_views=1, consistency_inv_depth_steps=2.0, consistency_max_reproj=0.75,
                            consistency_max_violations=2)
    assert est.plane_step() == (2.0 - 0.25) / 28 and est.counts_map is None
    assert est.mvs_params == dict(num_planes=29)  # the check's settings are the estimator's own, not the matcher's
    # frame 1: nothing to match against - no depth, and no raw depth in the ring
    assert est.infer_posed(frame(1), pose(0.0)) == (None, None) and vol.calls == [] and est.ring[0][3] is None
    # frame 2 is matched against frame 1, which carries no depth: skipped, but its raw depth is kept
    assert est.infer_posed(frame(2), pose(-0.25)) == (None, None)
    assert [c[0] for c in vol.calls] == ["mvs"] and est.index_map is None and est.counts_map is None and est.sources_used == (0,)
    assert (est.ring[0][3] == 2.0).all() and est.ring[1][3] is None
    vol.calls.clear()
    # frame 3 is matched against 2 and 1 and checked against 2 alone: max_violations is capped at the views checked against
    depth, pts3d = est.infer_posed(frame(3), pose(-0.5))
    (_, _, matched, _), (_, raw, against, kw) = vol.calls
    assert [int(m[0, 0, 0]) for m in matched] == [2, 1] and (raw == 3.0).all() and [float(a[0, 0]) for a in against] == [2.0]
    assert pts3d is None and (depth == 3.5).all() and est.counts_map.shape == (H, W, 4) and est.index_map.dtype == np.int16
    assert kw["intrinsic"] == (30.0, 31.0, 9.5, 2.5) and kw["inv_depth_tol"] == 2.0 * est.plane_step() and kw["rel_depth_tol"] == 0.0
    assert kw["max_reproj_error"] == 0.75 and kw["min_consistent"] == 1 and kw["max_violations"] == 1 and kw["fuse"] is True and kw["counts"] is True
    np.testing.assert_array_equal(kw["T_ref"], pose(-0.5))
    np.testing.assert_array_equal(kw["T_sources"], pose(-0.25)[None])
    assert (est.ring[0][3] == 3.0).all()  # the ring keeps the raw depth, not the checked one: a verdict does not cascade
    vol.calls.clear()
    # frame 4 against 3 and 2, both with a raw depth, the most recent first
    est.infer_posed(frame(4), pose(-0.75))
    assert [float(a[0, 0]) for a in vol.calls[1][2]] == [3.0, 2.0] and vol.calls[1][3]["max_violations"] == 2
    np.testing.assert_array_equal(vol.calls[1][3]["T_sources"], np.stack([pose(-0.5), pose(-0.25)]))
    # consistency_min_views = 2: one source with a depth is not enough
    vol.calls.clear()
    est2 = DepthEstimatorMvs(vol, CAM, keep_on_device=False, min_depth=0.5, min_baseline=0.125, max_baseline=0.5, consistency_min_views=2)
    got = [est2.infer_posed(frame(i), pose(-0.25 * i))[0] is None for i in range(4)]
    assert got == [True, True, True, False] and [c[0] for c in vol.calls] == ["mvs", "mvs", "mvs", "check"]
    assert vol.calls[-1][3]["min_consistent"] == 2 and vol.calls[-1][3]["inv_depth_tol"] == 2.0 / 127
    for bad in (dict(consistency_min_views=-1), dict(consistency_min_views=3), dict(consistency_min_views=1.5), dict(consistency_max_violations=-1),
                dict(consistency_inv_depth_steps=0.0), dict(consistency_inv_depth_steps=np.nan), dict(consistency_max_reproj=-1.0)):
        with pytest.raises(ValueError):
            DepthEstimatorMvs(vol, CAM, **{**dict(min_depth=0.4, min_baseline=0.1), **bad})


def test_depth_estimator_mvs_without_the_check_is_what_it_was():
    from pyslam_amd.depth_estimation import DepthEstimatorMvs

    vol = StubVolume()
    est = DepthEstimatorMvs(vol, CAM, keep_on_device=False, min_depth=0.5, min_baseline=0.125, max_baseline=0.5)
    assert est.consistency_min_views == 0
    assert est.infer_posed(frame(1), pose(0.0)) == (None, None)
    depth, _ = est.infer_posed(frame(2), pose(-0.25))
    assert [c[0] for c in vol.calls] == ["mvs"] and (depth == 2.0).all() and est.counts_map is None and est.index_map is not None
    assert set(vol.calls[0][3]) == {"intrinsic", "T_ref", "T_sources", "min_depth", "max_depth"}


def test_depth_estimator_mvs_sends_what_filter_depth_consistency_takes():
    """On the recording library: the estimator's check is a valid filter_depth_consistency call with the matrices of its poses."""
    from pyslam_amd.depth_estimation import DepthEstimatorMvs

    vol = tsdf()
    vol._lib.script("hv_depth_consistency", peek={6: (np.float32, 12), 7: (np.float32, 12)})
    est = DepthEstimatorMvs(vol, CAM, keep_on_device=False, min_depth=0.5, min_baseline=0.05, num_planes=64, consistency_min_views=1)
    rng = np.random.default_rng(3)
    images = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    assert est.infer_posed(images[0], pose(0.0)) == (None, None) and vol._lib.calls == []
    assert est.infer_posed(images[1], pose(-0.1)) == (None, None)
    expect(vol, ("hv_mvs_sgm", ANY, ANY, 1, H, W, 3, ANY, REF(L.HvMvsParams), ANY, P(est.ring[0][3]), None, L.HV_HOST))
    depth, _ = est.infer_posed(images[2], pose(-0.2))
    _, call = expect(vol, ("hv_mvs_sgm", ANY, ANY, 2, H, W, 3, ANY, REF(L.HvMvsParams), P(est.index_map), P(est.ring[0][3]), None, L.HV_HOST),
                     ("hv_depth_consistency", P(est.ring[0][3]), ANY, 1, H, W, ANY, ANY, REF(L.HvConsistencyParams), P(depth), P(est.counts_map), None,
                      L.HV_HOST))
    assert params(call) == dict(max_reproj_error=1.0, inv_depth_tol=np.float32(2.0 / 63), rel_depth_tol=0.0, min_consistent=1, max_violations=0, fuse=1)
    K = (30.0, 31.0, 9.5, 2.5)
    want, want_back = consistency_views(K, pose(-0.2), K, pose(-0.1))
    np.testing.assert_array_equal(vol._lib.peeked[-1][6], want.ravel())
    np.testing.assert_array_equal(vol._lib.peeked[-1][7], want_back.ravel())


def test_dense_front_hands_the_four_parameters_over(monkeypatch):
    from pyslam_amd.dense.parameters import Parameters
    from pyslam_amd.dense.volumetric_integrator_base import VolumetricIntegratorBase
    from pyslam_amd.depth_estimation import DepthEstimatorMvs

    names = ("kVolumetricIntegrationMvsConsistencyMinViews", "kVolumetricIntegrationMvsConsistencyInvDepthSteps",
             "kVolumetricIntegrationMvsConsistencyMaxReproj", "kVolumetricIntegrationMvsConsistencyMaxViolations")
    assert [getattr(Parameters, k) for k in names] == [0, 1.0, 1.0, 0]
    cam = types.SimpleNamespace(fx=100.0, fy=100.0, cx=10.0, cy=3.0, width=W, height=H, D=np.zeros(5), bf=14.4375)
    monkeypatch.setattr(Parameters, "kVolumetricIntegrationUseDepthEstimator", True)
    monkeypatch.setattr(Parameters, "kVolumetricIntegrationDepthEstimatorType", "DEPTH_MVS_HIP")
    monkeypatch.setattr(DepthEstimatorMvs, "infer_posed", lambda self, img, T_cw: (None, None))
    kd = types.SimpleNamespace(img=frame(1), img_right=None, depth=None, id=3, pose=pose(0.1), semantic_img=None, semantic_instances_img=None)

    def estimator():
        integ = VolumetricIntegratorBase.__new__(VolumetricIntegratorBase)
        integ.init(cam, None, None, {}, {})
        integ.volume = tsdf()
        assert integ.estimate_depth_if_needed_and_rectify(kd) == (None, None, None, None, None)
        return integ.depth_estimator

    est = estimator()
    assert (est.consistency_min_views, est.consistency_inv_depth_steps, est.consistency_max_reproj, est.consistency_max_violations) == (0, 1.0, 1.0, 0)
    for k, val in zip(names, (2, 1.5, 0.5, 1)):
        monkeypatch.setattr(Parameters, k, val)
    est = estimator()
    assert (est.consistency_min_views, est.consistency_inv_depth_steps, est.consistency_max_reproj, est.consistency_max_violations) == (2, 1.5, 0.5, 1)
    assert "consistency_min_views" not in est.mvs_params
