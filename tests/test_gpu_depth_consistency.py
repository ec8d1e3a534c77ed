"""GPU: _Volume.filter_depth_consistency (hv_depth_consistency) against the numpy restatement (tests/depth_consistency_reference.py),
bit for bit - the depth as uint32 views, the counts and the stats exactly - at the tile edges of the kernel
(depth_consistency_cases.SHAPES) with 1..4 views, on the planted rule edges, through DepthEstimatorMvs and the dense front, and
against the synthetic room's true depth."""
import ctypes

import numpy as np
import pytest

from pyslam_amd import _lib as L
from tests import depth_consistency_cases as cc
from tests import depth_consistency_reference as dr
from tests import mvs_cases as mc
from tests import mvs_reference as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vol():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    v = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)
    yield v
    v.close()


def _same(got, want):
    depth, counts, stats = got
    rdepth, rcounts, rstats = want
    assert depth.dtype == np.float32 and depth.shape == rdepth.shape
    np.testing.assert_array_equal(depth.view(np.uint32), rdepth.view(np.uint32))
    assert counts.dtype == np.uint8 and counts.shape == rcounts.shape
    np.testing.assert_array_equal(counts, rcounts)
    assert stats.as_tuple() == rstats


def _check(vol, depth, sources, views, back_views, **kw):
    want = dr.depth_consistency(depth, sources, views, back_views, **kw)
    _same(vol.filter_depth_consistency(depth, sources, views, back_views, counts=True, stats=True, **kw), want)
    return want


@pytest.mark.parametrize("N", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_matches_the_restatement_at_every_tile_edge(vol, shape, N):
    depth, sources, views, back_views, *_ = cc.random_case(*shape, N)
    for kw in cc.rule_settings(N):
        _, counts, stats = _check(vol, depth, sources, views, back_views, **kw)
    assert stats[2] > 0 and counts[..., 1].any() and counts[..., 2].any()  # (the case holds every class: test_depth_consistency_reference_cpu.py)
    # the tolerances of a plane sweep instead of a sensor's
    _check(vol, depth, sources, views, back_views, inv_depth_tol=1.0 / 31, rel_depth_tol=0.0, max_reproj_error=0.5)


@pytest.mark.parametrize("case", cc.planted(), ids=lambda c: c[0])
def test_planted_rule_edges(vol, case):
    _, depth, sources, views, back_views, kw, _ = case
    want = _check(vol, depth, sources, views, back_views, **kw)
    _check(vol, depth, sources, views, back_views, **{**kw, "fuse": False})
    # one output only: the depth alone through the binding, either alone over the C ABI
    only, none = vol.filter_depth_consistency(depth, sources, views, back_views, **kw)
    assert none is None
    np.testing.assert_array_equal(only.view(np.uint32), want[0].view(np.uint32))
    prm = L.HvConsistencyParams(kw["max_reproj_error"], kw["inv_depth_tol"], kw["rel_depth_tol"], kw.get("min_consistent", 1), kw.get("max_violations", 0), 1)
    H, W = depth.shape
    out, counts = np.full((H, W), -77.0, np.float32), np.full((H, W, 4), 0x5A, np.uint8)
    args = (vol._h, L.ptr(depth), L.ptr(sources), len(sources), H, W, L.ptr(views), L.ptr(back_views), ctypes.byref(prm))
    assert vol._lib.hv_depth_consistency(*args, None, L.ptr(counts), None, L.HV_HOST) == 0
    np.testing.assert_array_equal(counts, want[1])
    assert vol._lib.hv_depth_consistency(*args, L.ptr(out), None, None, L.HV_HOST) == 0
    np.testing.assert_array_equal(out.view(np.uint32), want[0].view(np.uint32))


def test_device_tensors_agree_with_host_arrays(vol):
    import torch

    depth, sources, views, back_views, K, T_ref, T_src = cc.random_case(37, 83, 3, seed=1)
    host = _check(vol, depth, sources, views, back_views, max_violations=1)
    d, s = torch.from_numpy(depth).cuda(), torch.from_numpy(sources).cuda()
    dev = vol.filter_depth_consistency(d, s, views, back_views, max_violations=1, counts=True, stats=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in dev[:2]) and dev[0].dtype == torch.float32 and dev[1].dtype == torch.uint8
    _same((dev[0].cpu().numpy(), dev[1].cpu().numpy(), dev[2]), host)
    as_list = vol.filter_depth_consistency(d, [t for t in s], views, back_views, max_violations=1, counts=True, stats=True)
    _same((as_list[0].cpu().numpy(), as_list[1].cpu().numpy(), as_list[2]), host)
    from_poses = vol.filter_depth_consistency(d, s, intrinsic=K, T_ref=T_ref, T_sources=T_src, max_violations=1)  # no stats: queued, not waited for
    assert from_poses[1] is None
    np.testing.assert_array_equal(from_poses[0].cpu().numpy().view(np.uint32), host[0].view(np.uint32))
    with pytest.raises(ValueError, match="same place"):
        vol.filter_depth_consistency(d, sources, views, back_views)
    with pytest.raises(ValueError, match="float32"):
        vol.filter_depth_consistency(d.double(), s.double(), views, back_views)


GOOD = dict(max_reproj_error=1.0, inv_depth_tol=0.0, rel_depth_tol=0.01, min_consistent=1, max_violations=0, fuse=1)
BAD_PARAMS = [dict(max_reproj_error=-1.0), dict(max_reproj_error=np.nan), dict(max_reproj_error=np.inf), dict(inv_depth_tol=-0.5),
              dict(inv_depth_tol=np.nan), dict(inv_depth_tol=np.inf), dict(rel_depth_tol=-0.01), dict(rel_depth_tol=np.nan), dict(rel_depth_tol=np.inf),
              dict(inv_depth_tol=0.0, rel_depth_tol=0.0), dict(min_consistent=-1), dict(min_consistent=3), dict(max_violations=-1), dict(max_violations=3)]


def test_invalid_arguments_write_nothing(vol):
    H, W, N = 12, 40, 2
    depth, sources, views, back_views, *_ = cc.random_case(H, W, N)
    out = np.full((H, W), -77.0, np.float32)
    counts = np.full((H, W, 4), 0x5A, np.uint8)
    stats = L.HvConsistencyStats(7, 7, 7)

    def call(prm, depth=depth, sources=sources, n=N, h=H, w=W, views=views, back_views=back_views, out=out, counts=counts):
        return vol._lib.hv_depth_consistency(vol._h, L.ptr(depth), L.ptr(sources), n, h, w, L.ptr(views), L.ptr(back_views),
                                             ctypes.byref(prm) if prm is not None else None, L.ptr(out), L.ptr(counts), ctypes.byref(stats), L.HV_HOST)

    def refused(rc):
        assert rc == -1, rc  # HV_ERR_INVALID
        assert (out == -77.0).all() and (counts == 0x5A).all() and (stats.valid_pixels, stats.kept_pixels, stats.agree_sum) == (7, 7, 7)
        with pytest.raises(L.HipVolError):
            L.check(rc)

    for bad in BAD_PARAMS:
        refused(call(L.HvConsistencyParams(**{**GOOD, **bad})))
    good = L.HvConsistencyParams(**GOOD)
    refused(call(good, depth=None))
    refused(call(good, sources=None))
    refused(call(good, views=None))
    refused(call(good, back_views=None))
    refused(call(None))
    refused(call(good, out=None, counts=None))
    for n in (0, 5, -1):
        refused(call(good, n=n))
    for h, w in ((0, W), (H, 0), (-1, W), (32769, 1), (32768, 32768)):
        refused(call(good, h=h, w=w))
    for bad in (np.nan, np.inf, -np.inf):
        m = views.copy()
        m[1, 2, 3] = bad
        refused(call(good, views=m))
        refused(call(good, back_views=m))
    # the good call goes through
    assert call(good) == 0
    want = dr.depth_consistency(depth, sources, views, back_views)
    np.testing.assert_array_equal(out.view(np.uint32), want[0].view(np.uint32))
    np.testing.assert_array_equal(counts, want[1])
    assert (stats.valid_pixels, stats.kept_pixels, stats.agree_sum) == want[2]
    for bad in (dict(max_reproj_error=-1.0), dict(inv_depth_tol=np.nan), dict(rel_depth_tol=0.0), dict(min_consistent=3), dict(max_violations=-1)):
        with pytest.raises(ValueError):  # the binding refuses the same arguments before it calls
            vol.filter_depth_consistency(depth, sources, views, back_views, **bad)


def test_a_map_is_left_alone():
    from pyslam_amd.synthetic import SyntheticRGBD
    from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume

    s = SyntheticRGBD("tiny_160x120_2cm")
    v = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 12)
    try:
        K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
        for i in range(2):
            depth, rgb, T = s[i]
            v.integrate(RGBDImage(rgb, depth, 1.0, 4.0), K, T)
        v.mark_merged()
        before = v.dump()
        assert len(before[0]) > 10 and len(v.dirty_keys()) == 0
        depth, sources, views, back_views, *_ = cc.random_case(37, 83, 2)
        _check(v, depth, sources, views, back_views)
        assert len(v.dirty_keys()) == 0
        for a, b in zip(before, v.dump()):
            np.testing.assert_array_equal(a, b)
    finally:
        v.close()


@pytest.fixture(scope="module")
def room():
    s, frames = cc.truth_frames()
    return s, frames


def test_ground_truth(vol, room):
    """Three multiview_sgm calls on the device (poses 150, 140 and 130, each against its own two earlier poses), then the check of the
    first against the other two, against the synthetic room's true depth.  Measured with the restatements, which the kernels equal
    bit for bit (tests/test_depth_consistency_reference_cpu.py): valid 0.5092, off by more than one plane step 0.0148 (0.1205 before
    the check), median error 0.193 plane steps.  Asserted with the margins of the matchers' ground-truth tests."""
    s, frames = room
    K = s.intrinsics
    raw = [vol.multiview_sgm(rgb, sources, intrinsic=K, T_ref=T, T_sources=T_src, index=False, **mc.TRUTH_PARAMS)[1] for rgb, _, T, sources, T_src in frames]
    out, _ = vol.filter_depth_consistency(raw[0], raw[1:], intrinsic=K, T_ref=frames[0][2], T_sources=np.stack([frames[1][2], frames[2][2]]), **cc.TRUTH_CHECK)
    valid, off, median = cc.depth_figures(out, frames[0][1])
    print(f"valid {valid:.4f}, off by > 1 plane step {off:.4f}, median error {median:.3f} steps")
    assert valid >= cc.TRUTH_MEASURED[0] - 0.05
    assert off <= 1.5 * cc.TRUTH_MEASURED[1]
    assert median <= 1.5 * cc.TRUTH_MEASURED[2]


def test_depth_estimator_checks_keyframes_against_the_ring(vol):
    """DepthEstimatorMvs with consistency_min_views = 1 on the poses 120, 130, 140 and 150: no depth for the first, the second is
    skipped with its raw depth in the ring, the later ones equal the restatement of the check applied to the restated plane-sweep
    depths; with the default 0 the outputs are those of multiview_sgm itself, bit for bit."""
    from pyslam_amd.depth_estimation import DepthEstimatorMvs
    from pyslam_amd.prep import consistency_views, plane_sweep_views
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD(mc.TRUTH_CONFIG, noise=False, invalid_frac=0.0)
    cam = type("Camera", (), dict(zip(("fx", "fy", "cx", "cy"), s.intrinsics)))()
    K = tuple(float(k) for k in s.intrinsics)
    kw = dict(min_baseline=0.1, max_baseline=0.3, **mc.TRUTH_PARAMS)
    est = DepthEstimatorMvs(vol, cam, keep_on_device=False, consistency_min_views=1, **kw)
    plain = DepthEstimatorMvs(vol, cam, keep_on_device=False, **kw)
    frames, raw = [], []
    for n, i in enumerate((120, 130, 140, 150)):
        _, rgb, T = s[i]
        depth, _ = est.infer_posed(rgb, T)
        unchecked, _ = plain.infer_posed(rgb, T)
        assert plain.counts_map is None
        used = [frames[n - 1 - k] for k in est.sources_used]
        assert est.sources_used == plain.sources_used == ((), (0,), (0, 1), (0, 1))[n]
        want = None
        if used:
            views = plane_sweep_views(K, T, K, np.stack([f[1] for f in used]))
            want = mr.multiview_sgm(rgb, [f[0] for f in used], views, **mc.TRUTH_PARAMS)
            np.testing.assert_array_equal(unchecked.view(np.uint32), want[1].view(np.uint32))
            np.testing.assert_array_equal(plain.index_map, want[0])
            np.testing.assert_array_equal(est.ring[0][3].view(np.uint32), want[1].view(np.uint32))  # the raw depth, checked or not
        else:
            assert unchecked is None and est.ring[0][3] is None
        if n < 2:
            assert depth is None and est.counts_map is None and est.index_map is None  # nothing to match with; nothing to check against
        else:
            against = [(raw[n - 1 - k], frames[n - 1 - k][1]) for k in est.sources_used if raw[n - 1 - k] is not None]
            assert len(against) == n - 1
            v, b = consistency_views(K, T, K, np.stack([a[1] for a in against]))
            checked = dr.depth_consistency(want[1], [a[0] for a in against], v, b, max_reproj_error=1.0, inv_depth_tol=est.plane_step(), rel_depth_tol=0.0,
                                           min_consistent=1, max_violations=0, fuse=True)
            np.testing.assert_array_equal(depth.view(np.uint32), checked[0].view(np.uint32))
            np.testing.assert_array_equal(est.counts_map, checked[1])
            np.testing.assert_array_equal(est.index_map, want[0])
            assert 0 < (depth > 0).sum() < (want[1] > 0).sum()
        frames.append((rgb, T))
        raw.append(None if want is None else want[1])


def test_checked_keyframes_reach_the_tsdf_through_the_front():
    """kVolumetricIntegrationDepthEstimatorType = "DEPTH_MVS_HIP" with the four consistency parameters: the first keyframe has nothing
    to match with, the second nothing to be checked against, the later ones -> hv_mvs_sgm -> hv_depth_consistency against the raw
    depths in the ring -> depth as a CUDA tensor -> shadow filter -> TSDF fusion."""
    import torch

    from pyslam_amd.dense.parameters import Parameters
    from pyslam_amd.dense.volumetric_integrator_base import VolumetricIntegrationKeyframeData
    from pyslam_amd.dense.volumetric_integrator_tsdf import VolumetricIntegratorTsdf
    from pyslam_amd.dense.volumetric_integrator_types import DatasetEnvironmentType, SensorType
    from pyslam_amd.depth_estimation import DepthEstimatorMvs
    from pyslam_amd.synthetic import SyntheticRGBD
    from pyslam_amd.volumetric import RGBDImage
    from tests import dense_helpers as dh

    values = dict(kVolumetricIntegrationUseDepthEstimator=True, kVolumetricIntegrationDepthEstimatorType="DEPTH_MVS_HIP",
                  kVolumetricIntegrationVoxelLength=0.02, kVolumetricIntegrationTSdfTrunc=0.08, kVolumetricIntegrationOutputTimeInterval=0.0,
                  kVolumetricIntegrationHipMaxBlocks=1 << 13, kVolumetricIntegrationMvsNumPlanes=32, kVolumetricIntegrationMvsMinDepth=1.0,
                  kVolumetricIntegrationMvsMinBaseline=0.1, kVolumetricIntegrationMvsMaxBaseline=0.3,
                  kVolumetricIntegrationMvsConsistencyMinViews=1, kVolumetricIntegrationMvsConsistencyInvDepthSteps=1.5,
                  kVolumetricIntegrationMvsConsistencyMaxReproj=0.75, kVolumetricIntegrationMvsConsistencyMaxViolations=1,
                  kVolumetricIntegrationDepthEstimationFilterShadowPoints=False)  # (the depth handed to the map is the check's own output)
    saved = {k: getattr(Parameters, k) for k in values}
    for k, val in values.items():
        setattr(Parameters, k, val)
    try:
        s = SyntheticRGBD(mc.TRUTH_CONFIG, noise=False, invalid_frac=0.0)
        cam = dh.FakeCamera(s)
        integ = VolumetricIntegratorTsdf.__new__(VolumetricIntegratorTsdf)
        integ.init(cam, DatasetEnvironmentType.INDOOR, SensorType.MONOCULAR, {}, {})
        for i in (120, 130, 140, 150):
            kf = dh.FakeKeyFrame(i, s, cam)
            kf.depth_img = None
            kd = VolumetricIntegrationKeyframeData(kf, kf.img, None, None)
            color, depth, _, _, _ = integ.estimate_depth_if_needed_and_rectify(kd)
            if i <= 130:
                assert color is None and depth is None  # skipped
                continue
            assert isinstance(depth, torch.Tensor) and depth.is_cuda
            rgbd = RGBDImage.create_from_color_and_depth(color, depth, depth_scale=1.0, depth_trunc=4.0, convert_rgb_to_intensity=False)
            integ.volume.integrate(rgbd, integ.o3d_camera, kd.pose)
            last = depth.cpu().numpy()
        est = integ.depth_estimator
        assert isinstance(est, DepthEstimatorMvs) and est.sources_used == (0, 1)
        assert (est.consistency_min_views, est.consistency_inv_depth_steps, est.consistency_max_reproj, est.consistency_max_violations) == (1, 1.5, 0.75, 1)
        assert est.counts_map.is_cuda and tuple(est.counts_map.shape) == (s.height, s.width, 4) and est.counts_map.dtype == torch.uint8
        # what the front integrated last is the checked depth: the restatement of the check on the ring's raw depths
        from pyslam_amd.prep import consistency_views

        (_, T, _, raw), a, b = est.ring[0], est.ring[1], est.ring[2]
        K = tuple(float(k) for k in s.intrinsics)
        v, back = consistency_views(K, T, K, np.stack([a[1], b[1]]))
        want = dr.depth_consistency(raw.cpu().numpy(), [a[3].cpu().numpy(), b[3].cpu().numpy()], v, back, max_reproj_error=0.75,
                                    inv_depth_tol=1.5 * est.plane_step(), rel_depth_tol=0.0, min_consistent=1, max_violations=1, fuse=True)
        np.testing.assert_array_equal(est.counts_map.cpu().numpy(), want[1])
        np.testing.assert_array_equal(last.view(np.uint32), want[0].view(np.uint32))
        assert 0 < int((want[0] > 0).sum()) < int((raw > 0).sum())
        assert integ.volume.num_blocks() > 10
    finally:
        for k, val in saved.items():
            setattr(Parameters, k, val)
