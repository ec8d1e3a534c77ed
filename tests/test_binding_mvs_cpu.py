"""What multiview_sgm sends over the C ABI, pinned against the recording stand-in for the library (tests/recording_lib.py; no GPU), in
the manner of tests/test_binding_stereo_cpu.py; DepthEstimatorMvs's ring and choice of sources on a stub volume; and the dense
front's choice of the estimator and its skip of a keyframe without enough sources."""
import types

import numpy as np
import pytest

from pyslam_amd import _lib as L
from pyslam_amd import volumetric as V
from pyslam_amd import volumetric_semantic as S
from pyslam_amd.prep import plane_sweep_views
from tests.recording_lib import ref, volume
from tests.test_binding_calls_cpu import ANY, P, REF, covers, expect, host, refused, shaped, tsdf  # noqa: F401 (host: a fixture)

H, W = 6, 20
FIELDS = ("num_planes", "p1", "p2", "uniqueness_ratio", "min_views", "paths", "min_depth", "max_depth", "speckle_window_size", "speckle_range")
VIEWS = np.array([[[1, 0, 0, -1], [0, 1, 0, 0], [0, 0, 1, 0]], [[1, 0, 0, 2], [0, 1, 0, 0.5], [0, 0, 1, 0.25]]], np.float32)


def images(n=2, channels=3, seed=0):
    rng = np.random.default_rng(seed)
    shape = (H, W) if channels == 1 else (H, W, channels)
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, (n,) + shape, dtype=np.uint8)


def params(call):
    p = ref(call[1][8])
    return {f: getattr(p, f) for f in FIELDS}


def pose(tx=0.0, ty=0.0, tz=0.0):
    T = np.eye(4)
    T[:3, 3] = (tx, ty, tz)
    return T


@pytest.mark.parametrize("channels", [1, 3])
@covers("multiview_sgm")
def test_multiview_sgm_defaults_and_result_kinds(channels):
    image, sources = images(2, channels)
    for vol in (tsdf(), volume(V.VoxelBlockGrid, voxel_size=0.05, block_size=8), volume(S.VoxelBlockSemanticGrid, voxel_size=0.05, block_size=8)):
        vol._lib.script("hv_mvs_sgm", peek={7: (np.float32, 24)})
        index, depth = vol.multiview_sgm(image, sources, VIEWS, min_depth=0.5)
        call, = expect(vol, ("hv_mvs_sgm", P(image), P(sources), 2, H, W, channels, ANY, REF(L.HvMvsParams), P(index), P(depth), None, L.HV_HOST))
        shaped(index, (H, W), np.int16), shaped(depth, (H, W), np.float32)
        assert params(call) == dict(num_planes=128, p1=10, p2=120, uniqueness_ratio=15, min_views=1, paths=8, min_depth=0.5, max_depth=np.inf,
                                    speckle_window_size=0, speckle_range=1)
        np.testing.assert_array_equal(vol._lib.peeked[-1][7], VIEWS.ravel())


@covers("multiview_sgm")
def test_multiview_sgm_marshals_every_argument(host):
    image, sources = images(3)
    vol = tsdf()
    vol._lib.script("hv_mvs_sgm", peek={1: (np.uint8, H * W * 3), 2: (np.uint8, 3 * H * W * 3), 7: (np.float32, 36)})
    views = np.concatenate([VIEWS, VIEWS[:1] * 2])
    index, depth = vol.multiview_sgm(host(image), [host(s) for s in sources], host(views), min_depth=0.25, max_depth=6.5, num_planes=48, p1=7, p2=99,
                                     uniqueness_ratio=0, min_views=3, paths=4, speckle_window_size=50, speckle_range=2)
    call, = expect(vol, ("hv_mvs_sgm", P(image), ANY, 3, H, W, 3, ANY, REF(L.HvMvsParams), P(index), P(depth), None, L.HV_HOST))
    shaped(index, (H, W), np.int16), shaped(depth, (H, W), np.float32)  # host operands of either kind: numpy results
    assert params(call) == dict(num_planes=48, p1=7, p2=99, uniqueness_ratio=0, min_views=3, paths=4, min_depth=0.25, max_depth=6.5,
                                speckle_window_size=50, speckle_range=2)
    assert all(type(x) is int for x in call[1][3:7])
    # a list of sources is sent as one contiguous block, in order; the matrices as float32 [N,3,4]
    np.testing.assert_array_equal(vol._lib.peeked[-1][2], sources.ravel())
    np.testing.assert_array_equal(vol._lib.peeked[-1][7], views.ravel())
    # one output only; strided views are made contiguous for the call; numpy integers are plain ints by then; float64 matrices are rounded
    wide = np.zeros((H, 2 * W, 3), np.uint8)
    index, depth = vol.multiview_sgm(wide[:, ::2], wide[None, :, 1::2], VIEWS[:1].astype(np.float64), min_depth=1.0, num_planes=np.int64(16),
                                     paths=np.int32(8), depth=False)
    call, = expect(vol, ("hv_mvs_sgm", ANY, ANY, 1, H, W, 3, ANY, REF(L.HvMvsParams), P(index), None, None, L.HV_HOST))
    assert depth is None and params(call)["num_planes"] == 16 and params(call)["paths"] == 8
    index, depth = vol.multiview_sgm(image, sources, views, min_depth=1.0, index=False)
    expect(vol, ("hv_mvs_sgm", P(image), P(sources), 3, H, W, 3, ANY, REF(L.HvMvsParams), None, P(depth), None, L.HV_HOST))
    assert index is None


@covers("multiview_sgm")
def test_multiview_sgm_views_from_poses():
    image, sources = images(2)
    vol = tsdf()
    vol._lib.script("hv_mvs_sgm", peek={7: (np.float32, 24)})
    K = V.PinholeCameraIntrinsic(W, H, 30.0, 31.0, 9.5, 2.5)
    T_ref, T_src = pose(0.1, 0.0, 0.2), np.stack([pose(0.0, 0.05, 0.2), pose(0.3, 0.0, 0.1)])
    want = plane_sweep_views(K, T_ref, K, T_src)
    for intrinsic in (K, (30.0, 31.0, 9.5, 2.5), np.array([[30.0, 0, 9.5], [0, 31.0, 2.5], [0, 0, 1]])):
        vol.multiview_sgm(image, sources, intrinsic=intrinsic, T_ref=T_ref, T_sources=T_src, min_depth=0.5)
        expect(vol, ("hv_mvs_sgm", P(image), P(sources), 2, H, W, 3, ANY, REF(L.HvMvsParams), ANY, ANY, None, L.HV_HOST))
        np.testing.assert_array_equal(vol._lib.peeked[-1][7], want.ravel())
    # the same matrices handed over directly: the same call
    vol.multiview_sgm(image, sources, want, min_depth=0.5)
    np.testing.assert_array_equal(vol._lib.peeked[-1][7], want.ravel())
    expect(vol, ("hv_mvs_sgm", P(image), P(sources), 2, H, W, 3, ANY, REF(L.HvMvsParams), ANY, ANY, None, L.HV_HOST))
    # a pure translation along x by t: A = I, b = (fx t, 0, 0)
    m = plane_sweep_views(K, pose(), K, pose(-0.5))
    np.testing.assert_allclose(m[0], [[1, 0, 0, -15.0], [0, 1, 0, 0], [0, 0, 1, 0]], atol=1e-6)
    call = lambda **kw: vol.multiview_sgm(image, sources, min_depth=0.5, **kw)
    refused(vol, ValueError, "pass either views or intrinsic", call)
    refused(vol, ValueError, "pass either views or intrinsic", call, views=want, intrinsic=K)
    refused(vol, ValueError, "pass either views or intrinsic", call, views=want, T_ref=T_ref)
    refused(vol, ValueError, "intrinsic needs the poses", call, intrinsic=K, T_ref=T_ref)
    refused(vol, ValueError, "views must be [2, 3, 4]", call, intrinsic=K, T_ref=T_ref, T_sources=T_src[:1])


@covers("multiview_sgm")
def test_multiview_sgm_refusals_come_before_any_call():
    image, sources = images(2)
    vol = tsdf()
    call = lambda *a, **kw: vol.multiview_sgm(*(a or (image, sources, VIEWS)), **{"min_depth": 0.5, **kw})
    for bad in (0, 8, 24, 272, -16):
        refused(vol, ValueError, "multiview_sgm: num_planes must be a multiple of 16 in 16..256", call, num_planes=bad)
    for p1, p2 in ((0, 10), (-1, 10), (11, 10), (10, 1024)):
        refused(vol, ValueError, "multiview_sgm: need 0 < p1 <= p2 <= 1023", call, p1=p1, p2=p2)
    for bad in (-1, 100):
        refused(vol, ValueError, "multiview_sgm: uniqueness_ratio must be in 0..99", call, uniqueness_ratio=bad)
    for bad in (0, 2, 5, 16):
        refused(vol, ValueError, "multiview_sgm: paths must be 4 or 8", call, paths=bad)
    for bad in (0, 3, -1, 1.5):
        refused(vol, ValueError, "multiview_sgm: min_views must be in 1..2", call, min_views=bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(vol, ValueError, "multiview_sgm: min_depth must be finite and positive", call, min_depth=bad)
    refused(vol, ValueError, "the plane step overflows float32", call, min_depth=1e-60)
    for bad in (0.5, 0.25, np.nan, -np.inf):
        refused(vol, ValueError, "multiview_sgm: need max_depth > min_depth", call, max_depth=bad)
    for bad in (-1, (1 << 30) + 1, 2.5):
        refused(vol, ValueError, "multiview_sgm: speckle_window_size must be an integer in 0..2^30", call, speckle_window_size=bad)
    for bad in (-1, 4096):
        refused(vol, ValueError, "multiview_sgm: speckle_range must be an integer in 0..4095", call, speckle_range=bad)
    for bad in (np.nan, np.inf):
        m = VIEWS.copy()
        m[1, 0, 3] = bad
        refused(vol, ValueError, "multiview_sgm: a view matrix entry is not finite", call, image, sources, m)
    refused(vol, ValueError, "multiview_sgm: views must be [2, 3, 4]", call, image, sources, VIEWS[:1])
    refused(vol, ValueError, "multiview_sgm: views must be [2, 3, 4]", call, image, sources, VIEWS.reshape(2, 4, 3))
    refused(vol, ValueError, "multiview_sgm: no output asked for", call, index=False, depth=False)
    refused(vol, ValueError, "multiview_sgm: need 1..4 source views, got 5", call, image, np.zeros((5, H, W, 3), np.uint8), np.tile(VIEWS[:1], (5, 1, 1)))
    refused(vol, ValueError, "multiview_sgm: ref and sources must live in the same place", call, image, [], VIEWS)
    refused(vol, ValueError, "multiview_sgm: images must have 1 or 3 channels, got 2", call, image[..., :2], sources[..., :2], VIEWS)
    refused(vol, ValueError, "multiview_sgm: bad image size", call, image[:0], sources[:, :0], VIEWS)
    refused(vol, ValueError, "multiview_sgm: bad image size", call, image[:, :0], sources[:, :, :0], VIEWS)
    refused(vol, ValueError, "images of the reference's shape", call, image, sources[:, :, :-1], VIEWS)
    refused(vol, ValueError, "images of the reference's shape", call, image, [sources[0], sources[1][:-1]], VIEWS)
    refused(vol, ValueError, "images of the reference's shape", call, image, sources[0], VIEWS[:1])
    refused(vol, ValueError, "multiview_sgm: the images must be uint8", call, image.astype(np.float32), sources, VIEWS)
    refused(vol, ValueError, "multiview_sgm: the images must be uint8", call, image, sources.astype(np.int16), VIEWS)
    with pytest.raises(TypeError):
        vol.multiview_sgm(image, sources, VIEWS)  # min_depth has no default: the sweep's range is the caller's to set
    assert vol._lib.calls == []


class StubVolume:
    """multiview_sgm that records its arguments and answers with arrays of the right kind."""

    def __init__(self):
        self.calls = []

    def multiview_sgm(self, ref, sources, views=None, **kw):
        self.calls.append((ref, list(sources), views, kw))
        return np.full(ref.shape[:2], 16, np.int16), np.full(ref.shape[:2], 2.0, np.float32)


def frame(i):
    return np.full((H, W, 3), i, np.uint8)


def test_depth_estimator_mvs_ring_and_source_choice():
    from pyslam_amd.depth_estimation import DepthEstimatorMvs

    cam = types.SimpleNamespace(fx=30.0, fy=31.0, cx=9.5, cy=2.5)
    vol = StubVolume()
    est = DepthEstimatorMvs(vol, cam, keep_on_device=False, min_depth=0.4, max_depth=8.0, max_sources=2, min_baseline=0.125, max_baseline=0.4375,
                            ring_size=4, num_planes=32, paths=4)
    assert est.index_map is None
    # camera centres along x (T_cw = [I | -c]), binary fractions: the distances are exact
    centres = (0.0, 0.0625, 0.25, 0.375, 0.75, 0.765625, 0.78125, 0.796875, 0.8125)
    got = [est.infer_posed(frame(i), pose(-c)) for i, c in enumerate(centres[:2])]
    assert got == [(None, None), (None, None)] and vol.calls == [] and est.index_map is None  # nothing yet; then 0.0625 is too near
    depth, pts3d = est.infer_posed(frame(2), pose(-centres[2]))  # frames 1 (0.1875) and 0 (0.25) qualify, the most recent first
    image, sources, views, kw = vol.calls.pop()
    assert pts3d is None and depth.dtype == np.float32 and est.index_map.dtype == np.int16 and est.sources_used == (0, 1)
    assert (image == 2).all() and [int(s[0, 0, 0]) for s in sources] == [1, 0] and views is None
    assert kw["intrinsic"] == (30.0, 31.0, 9.5, 2.5) and kw["min_depth"] == 0.4 and kw["max_depth"] == 8.0 and kw["num_planes"] == 32 and kw["paths"] == 4
    np.testing.assert_array_equal(kw["T_ref"], pose(-0.25))
    np.testing.assert_array_equal(kw["T_sources"], np.stack([pose(-0.0625), pose(0.0)]))
    est.infer_posed(frame(3), pose(-centres[3]))  # 2 (0.125, the bound itself), 1 (0.3125) and 0 (0.375) qualify: the two most recent
    assert [int(s[0, 0, 0]) for s in vol.calls.pop()[1]] == [2, 1] and est.sources_used == (0, 1)
    est.infer_posed(frame(4), pose(-centres[4]))  # only 3 (0.375) lies within max_baseline
    assert [int(s[0, 0, 0]) for s in vol.calls.pop()[1]] == [3] and est.sources_used == (0,)
    est.infer_posed(frame(5), pose(-centres[5]))  # 4 is too near, 3 (0.390625) qualifies, 2 and 1 are too far, 0 has left the ring
    assert [int(s[0, 0, 0]) for s in vol.calls.pop()[1]] == [3] and est.sources_used == (1,)
    assert [int(r[0][0, 0, 0]) for r in est.ring] == [5, 4, 3, 2]  # ring_size keyframes, the last one first
    for i in (6, 7):  # creeping on: 3 is the one usable source until it leaves the ring
        est.infer_posed(frame(i), pose(-centres[i]))
        assert [int(s[0, 0, 0]) for s in vol.calls.pop()[1]] == [3] and est.sources_used == (i - 4,)
    got = est.infer_posed(frame(8), pose(-centres[8]))  # the ring holds near frames only: the keyframe is skipped
    assert got == (None, None) and est.index_map is None and est.sources_used == () and vol.calls == []
    # min_views = 2: one qualifying keyframe is not enough
    est2 = DepthEstimatorMvs(vol, cam, keep_on_device=False, min_depth=0.4, min_baseline=0.125, max_baseline=0.4375, min_views=2)
    assert [est2.infer_posed(frame(i), pose(-c))[0] is None for i, c in enumerate((0.0, 0.25, 0.5))] == [True, True, True]
    assert est2.infer_posed(frame(3), pose(-0.625))[0] is not None and vol.calls.pop()[3]["min_views"] == 2  # 0.5 (0.125) and 0.25 (0.375)
    with pytest.raises(ValueError, match="infer_posed"):
        est.infer(frame(0), frame(1))
    for bad in (dict(max_sources=0), dict(max_sources=5), dict(min_baseline=0.5, max_baseline=0.1), dict(ring_size=1)):
        with pytest.raises(ValueError):
            DepthEstimatorMvs(vol, cam, **{**dict(min_depth=0.4, min_baseline=0.1), **bad})


def test_depth_estimator_mvs_sends_what_multiview_sgm_takes():
    """On the recording library: the estimator's call is a valid multiview_sgm call with the matrices of its poses."""
    from pyslam_amd.depth_estimation import DepthEstimatorMvs

    cam = types.SimpleNamespace(fx=30.0, fy=31.0, cx=9.5, cy=2.5)
    vol = tsdf()
    vol._lib.script("hv_mvs_sgm", peek={7: (np.float32, 12)})
    est = DepthEstimatorMvs(vol, cam, keep_on_device=False, min_depth=0.5, min_baseline=0.05, num_planes=64)
    first, second = images(1, seed=1)[0], images(1, seed=2)[0]
    assert est.infer_posed(first, pose(0.0)) == (None, None) and vol._lib.calls == []
    depth, _ = est.infer_posed(second, pose(-0.1))
    call, = expect(vol, ("hv_mvs_sgm", ANY, ANY, 1, H, W, 3, ANY, REF(L.HvMvsParams), P(est.index_map), P(depth), None, L.HV_HOST))
    assert params(call)["num_planes"] == 64 and params(call)["min_depth"] == 0.5 and params(call)["max_depth"] == np.inf
    np.testing.assert_array_equal(vol._lib.peeked[-1][7], plane_sweep_views((30.0, 31.0, 9.5, 2.5), pose(-0.1), (30.0, 31.0, 9.5, 2.5), pose(0.0)).ravel())


def test_dense_front_selects_the_estimator_and_skips_without_sources(monkeypatch):
    from pyslam_amd.dense.parameters import Parameters
    from pyslam_amd.dense.volumetric_integrator_base import VolumetricIntegratorBase
    from pyslam_amd.depth_estimation import DepthEstimatorMvs

    cam = types.SimpleNamespace(fx=100.0, fy=100.0, cx=10.0, cy=3.0, width=W, height=H, D=np.zeros(5), bf=14.4375)
    names = ("kVolumetricIntegrationUseDepthEstimator", "kVolumetricIntegrationDepthEstimatorType", "kVolumetricIntegrationMvsNumPlanes",
             "kVolumetricIntegrationMvsMinDepth", "kVolumetricIntegrationMvsMaxDepth", "kVolumetricIntegrationMvsMaxSources",
             "kVolumetricIntegrationMvsMinBaseline", "kVolumetricIntegrationMvsMaxBaseline", "kVolumetricIntegrationMvsSpeckleWindowSize",
             "kVolumetricIntegrationMvsSpeckleRange")
    saved = {k: getattr(Parameters, k) for k in names}
    assert [saved[k] for k in names[2:]] == [128, 0.5, np.inf, 2, 0.05, 0.5, 0, 1]
    try:
        def front(kind, use=True, camera=cam, **kwargs):
            Parameters.kVolumetricIntegrationUseDepthEstimator, Parameters.kVolumetricIntegrationDepthEstimatorType = use, kind
            integ = VolumetricIntegratorBase.__new__(VolumetricIntegratorBase)
            integ.init(camera, None, None, {}, kwargs)
            return integ

        injected = object()
        assert front("DEPTH_MVS_HIP", depth_estimator_factory=lambda c: injected).depth_estimator is injected  # keeps precedence
        assert not front("DEPTH_MVS_HIP", use=False).depth_estimator_pending
        distorted = types.SimpleNamespace(**{**vars(cam), "D": np.array([0.1, -0.05, 0.0, 0.0, 0.0])})
        with pytest.raises(ValueError, match="undistort first"):
            front("DEPTH_MVS_HIP", camera=distorted)
        Parameters.kVolumetricIntegrationMvsNumPlanes, Parameters.kVolumetricIntegrationMvsMinDepth = 64, 0.75
        Parameters.kVolumetricIntegrationMvsMaxDepth, Parameters.kVolumetricIntegrationMvsMaxSources = 9.0, 3
        Parameters.kVolumetricIntegrationMvsMinBaseline, Parameters.kVolumetricIntegrationMvsMaxBaseline = 0.02, 0.4
        Parameters.kVolumetricIntegrationMvsSpeckleWindowSize, Parameters.kVolumetricIntegrationMvsSpeckleRange = 50, 2
        integ = front("DEPTH_MVS_HIP")
        assert integ.depth_estimator is None and integ.depth_estimator_pending  # the volume does not exist yet
        integ.volume = tsdf()
        seen = []
        answers = [(None, None), (np.ones((H, W), np.float32), None)]
        monkeypatch.setattr(DepthEstimatorMvs, "infer_posed", lambda self, img, T_cw: (seen.append((img, T_cw)), answers[len(seen) - 1])[1])
        monkeypatch.setattr(Parameters, "kVolumetricIntegrationDepthEstimationFilterShadowPoints", False, raising=False)
        image = images()[0]
        kd = types.SimpleNamespace(img=image, img_right=None, depth=None, id=3, pose=pose(0.1), semantic_img=None, semantic_instances_img=None)
        assert integ.estimate_depth_if_needed_and_rectify(kd) == (None, None, None, None, None)  # no sources yet: the keyframe is skipped
        est = integ.depth_estimator
        assert isinstance(est, DepthEstimatorMvs) and est.volume is integ.volume and est.camera is cam and est.keep_on_device
        assert (est.min_depth, est.max_depth, est.max_sources, est.min_baseline, est.max_baseline) == (0.75, 9.0, 3, 0.02, 0.4)
        assert est.mvs_params == dict(num_planes=64, speckle_window_size=50, speckle_range=2)
        assert not integ.depth_estimator_pending and 3 not in integ.img_id_to_depth and integ.volume._lib.calls == []
        kd4 = types.SimpleNamespace(img=image, img_right=None, depth=None, id=4, pose=pose(0.2), semantic_img=None, semantic_instances_img=None)
        color, depth, pts3d, _, _ = integ.estimate_depth_if_needed_and_rectify(kd4)
        assert integ.depth_estimator is est and 4 in integ.img_id_to_depth and pts3d is None
        assert seen[0][0] is image and seen[1][0] is image and seen[0][1] is kd.pose and seen[1][1] is kd4.pose
        shaped(depth, (H, W), np.float32)
        # the stereo estimator is still what "DEPTH_SGM_HIP" makes
        from pyslam_amd.depth_estimation import DepthEstimatorSgm

        integ = front("DEPTH_SGM_HIP")
        integ.volume = tsdf()
        monkeypatch.setattr(DepthEstimatorSgm, "infer", lambda self, img, img_right=None: (np.ones((H, W), np.float32), None))
        integ.estimate_depth_if_needed_and_rectify(types.SimpleNamespace(img=image, img_right=image, depth=None, id=5, pose=pose(), semantic_img=None,
                                                                          semantic_instances_img=None))
        assert isinstance(integ.depth_estimator, DepthEstimatorSgm)
    finally:
        for k, val in saved.items():
            setattr(Parameters, k, val)
