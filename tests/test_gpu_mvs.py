"""GPU: _Volume.multiview_sgm (hv_mvs_sgm) against the numpy restatement (tests/mvs_reference.py), bit for bit - the int16 index with
assert_array_equal, the depth as uint32 views - at the shapes where the kernels change form (mvs_cases.SHAPES), on the planted rule
cases, against stereo_sgm itself where the two must agree, and end to end into a TSDF map."""
import ctypes

import numpy as np
import pytest

from pyslam_amd import _lib as L
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
    (index, depth), (rindex, rdepth) = got, want
    assert index.dtype == np.int16 and index.shape == rindex.shape
    np.testing.assert_array_equal(index, rindex)
    assert depth.dtype == np.float32
    np.testing.assert_array_equal(depth.view(np.uint32), rdepth.view(np.uint32))


def _check(vol, ref, sources, views, **kw):
    want = mr.multiview_sgm(ref, sources, views, **kw)
    _same(vol.multiview_sgm(ref, sources, views, **kw), want)
    return want


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "%dx%d_D%d" % s)
def test_matches_the_restatement_at_every_kernel_form(vol, shape, N, paths):
    H, W, D = shape
    ref, sources, views, kw = mc.textured_views(H, W, D, N, seed=H * 1000 + W + D + N)
    index, _ = _check(vol, ref, sources, views, paths=paths, min_views=min(N, 2), **kw)
    if min(H, W) >= 19:
        assert (index >= 0).mean() > 0.2  # (the sources show the reference: the matcher finds something)


@pytest.mark.parametrize("name", ["stair_D64", "stair_D128", "stair_D256"])
def test_stereo_anchor_against_stereo_sgm(vol, name):
    """The volume-fed path kernels against the census-fed ones: one view with A = I, b = (-1, 0, 0) and w_k = k is a stereo pair."""
    left, right, stereo, kw = mc.stereo_anchor(name)
    disp, _ = vol.stereo_sgm(left, right, **{k: v for k, v in stereo.items() if k not in ("bf", "min_depth", "max_depth")})
    index, _ = _check(vol, left, right[None], mc.STEREO_VIEW, **kw)
    k_star = mr.multiview_sgm(left, right[None], mc.STEREO_VIEW, return_parts=True, **kw)[2]["k_star"]
    outside = (disp >= 0) & (np.arange(left.shape[1])[None, :] - k_star < 0)
    np.testing.assert_array_equal(index, np.where(outside, mr.INVALID, disp))
    assert (index >= 0).mean() > 0.5


def test_planted_rule_cases(vol):
    ref, sources, views, kw = mc.m3_edges()
    for paths in (4, 8):
        _check(vol, ref, sources, views, paths=paths, **kw)
        _check(vol, ref, sources[:2], views[:2], paths=paths, min_views=2, **kw)
    for N in (2, 3, 4):
        ref, sources, views, kw = mc.m4_rounding(N)
        for min_views in range(1, N + 1):
            _check(vol, ref, sources, views, min_views=min_views, **kw)
    ref, sources, views, kw = mc.m6_one_blind_view()
    index, depth = _check(vol, ref, sources, views, **kw)
    assert (index == mr.INVALID).all() and (depth == 0).all()
    left, right, _, kw = mc.stereo_anchor("left_of_image_maxdiff-1")
    _check(vol, left, [right], mc.STEREO_VIEW, **kw)


def test_three_channels_and_finite_far_plane(vol):
    ref, sources, views, kw = mc.textured_views(37, 83, 48, 2, channels=3, seed=7)
    _check(vol, ref, sources, views, **kw)
    _check(vol, ref, sources, views, **{**kw, "max_depth": np.inf, "uniqueness_ratio": 0, "p1": 1023, "p2": 1023})


@pytest.mark.parametrize("only", [None, "index", "depth"])
def test_speckle_filter(vol, only):
    """speckle_window_size = 50: the restatement followed by tests/speckle_reference.py, with both outputs and with either alone
    (the filter then works on the index in scratch of the handle)."""
    ref, sources, views, kw = mc.textured_views(37, 83, 64, 2, seed=11)
    kw = dict(kw, speckle_window_size=50, speckle_range=1)
    want = mr.multiview_sgm(ref, sources, views, **kw)
    plain = mr.multiview_sgm(ref, sources, views, **{**kw, "speckle_window_size": 0})
    assert ((want[0] == mr.INVALID) & (plain[0] >= 0)).sum() > 0  # the filter has something to remove
    if only is None:
        _same(vol.multiview_sgm(ref, sources, views, **kw), want)
    else:
        index, depth = vol.multiview_sgm(ref, sources, views, index=only == "index", depth=only == "depth", **kw)
        assert (index is None) == (only == "depth") and (depth is None) == (only == "index")
        if index is not None:
            np.testing.assert_array_equal(index, want[0])
        else:
            np.testing.assert_array_equal(depth.view(np.uint32), want[1].view(np.uint32))


def test_device_tensors_agree_with_host_arrays(vol):
    import torch

    ref, sources, views, kw = mc.textured_views(37, 83, 64, 3, channels=3, seed=9)
    host = _check(vol, ref, sources, views, **kw)
    dev = vol.multiview_sgm(torch.from_numpy(ref).cuda(), torch.from_numpy(sources).cuda(), views, **kw)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in dev)
    assert dev[0].dtype == torch.int16 and dev[1].dtype == torch.float32
    _same((dev[0].cpu().numpy(), dev[1].cpu().numpy()), host)
    as_list = vol.multiview_sgm(torch.from_numpy(ref).cuda(), [torch.from_numpy(s).cuda() for s in sources], views, **kw)
    _same((as_list[0].cpu().numpy(), as_list[1].cpu().numpy()), host)
    index, depth = vol.multiview_sgm(torch.from_numpy(ref).cuda(), torch.from_numpy(sources).cuda(), views, depth=False, **kw)
    assert depth is None
    np.testing.assert_array_equal(index.cpu().numpy(), host[0])
    index, depth = vol.multiview_sgm(ref, sources, views, index=False, **kw)
    assert index is None
    np.testing.assert_array_equal(depth.view(np.uint32), host[1].view(np.uint32))


def test_scratch_regrowth_and_sharing_with_stereo():
    """Calls of different sizes on one volume, stereo_sgm between them (the two share the handle's scratch), against the restatements."""
    from pyslam_amd.volumetric import VoxelBlockGrid
    from tests import stereo_cases as sc
    from tests import stereo_reference as sr

    one = VoxelBlockGrid(0.02)  # any mode: the matcher reads nothing of the volume
    try:
        for (H, W, D, N) in ((19, 70, 16, 1), (37, 83, 128, 3), (24, 40, 32, 2)):
            ref, sources, views, kw = mc.textured_views(H, W, D, N, seed=H)
            _check(one, ref, sources, views, **kw)
            left, right = sc.textured_pair(H + 3, W + 5, 1, seed=H)
            np.testing.assert_array_equal(one.stereo_sgm(left, right, num_disparities=D)[0], sr.stereo_sgm(left, right, num_disparities=D)[0])
            _check(one, ref, sources, views, **kw)
    finally:
        one.close()


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
        ref, sources, views, kw = mc.textured_views(37, 83, 32, 2, seed=3)
        _check(v, ref, sources, views, **kw)
        assert len(v.dirty_keys()) == 0
        for a, b in zip(before, v.dump()):
            np.testing.assert_array_equal(a, b)
    finally:
        v.close()


GOOD = dict(num_planes=32, p1=10, p2=120, uniqueness_ratio=15, min_views=1, paths=8, min_depth=0.5, max_depth=6.0, speckle_window_size=0,
            speckle_range=1)
BAD_PARAMS = [dict(num_planes=0), dict(num_planes=24), dict(num_planes=272), dict(p1=0), dict(p1=121), dict(p2=1024),
              dict(uniqueness_ratio=-1), dict(uniqueness_ratio=100), dict(paths=5), dict(paths=2), dict(min_views=0), dict(min_views=3),
              dict(min_depth=0.0), dict(min_depth=-1.0), dict(min_depth=np.inf), dict(min_depth=np.nan), dict(min_depth=1e-60),
              dict(max_depth=0.5), dict(max_depth=0.25), dict(max_depth=np.nan), dict(speckle_window_size=-1),
              dict(speckle_window_size=(1 << 30) + 1), dict(speckle_window_size=5, speckle_range=-1), dict(speckle_window_size=5, speckle_range=4096)]


def test_invalid_arguments_write_nothing(vol):
    H, W, N = 12, 40, 2
    ref, sources, views, _ = mc.textured_views(H, W, 32, N, seed=1)
    index = np.full((H, W), 0x5A5A, np.int16)
    depth = np.full((H, W), -77.0, np.float32)

    def call(prm, ref=ref, sources=sources, n=N, h=H, w=W, c=1, views=views, index=index, depth=depth):
        return vol._lib.hv_mvs_sgm(vol._h, L.ptr(ref), L.ptr(sources), n, h, w, c, L.ptr(views), ctypes.byref(prm) if prm is not None else None,
                                   L.ptr(index), L.ptr(depth), None, L.HV_HOST)

    def refused(rc):
        assert rc == -1, rc  # HV_ERR_INVALID
        assert (index == 0x5A5A).all() and (depth == -77.0).all()
        with pytest.raises(L.HipVolError):
            L.check(rc)

    for bad in BAD_PARAMS:
        refused(call(L.HvMvsParams(**{**GOOD, **bad})))
    good = L.HvMvsParams(**GOOD)
    refused(call(good, ref=None))
    refused(call(good, sources=None))
    refused(call(good, views=None))
    refused(call(None))
    refused(call(good, index=None, depth=None))
    for c in (0, 2, 4):
        refused(call(good, c=c))
    for n in (0, 5, -1):
        refused(call(good, n=n))
    for h, w in ((0, W), (H, 0), (-1, W), (32769, 1)):
        refused(call(good, h=h, w=w))
    for bad in (np.nan, np.inf, -np.inf):
        m = views.copy()
        m[1, 2, 3] = bad
        refused(call(good, views=m))
    # the good call goes through, with one output and with both
    assert call(good, depth=None) == 0
    want = mr.multiview_sgm(ref, sources, views, **GOOD)
    np.testing.assert_array_equal(index, want[0])
    assert (depth == -77.0).all()
    assert call(good) == 0
    np.testing.assert_array_equal(depth.view(np.uint32), want[1].view(np.uint32))
    for bad in (dict(num_planes=24), dict(paths=3), dict(p1=0), dict(uniqueness_ratio=100), dict(min_views=3), dict(min_depth=0.0),
                dict(max_depth=0.5), dict(speckle_range=4096)):
        with pytest.raises(ValueError):  # the binding refuses the same arguments before it calls
            vol.multiview_sgm(ref, sources, views, **{**GOOD, **bad})


def test_posed_keyframes_reach_the_tsdf_on_the_device():
    """End to end on the synthetic room: a reference pose with two earlier poses as sources, multiview_sgm from intrinsics and poses
    -> filter_shadow_points -> integrate, all on the device; the depth equals the restatement's and the volume ends with units."""
    import torch

    from pyslam_amd.prep import plane_sweep_views
    from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume

    rgb, sources, _, T_ref, T_src, s = mc.synthetic_triple()
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    v = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 12)
    try:
        index, depth = v.multiview_sgm(torch.from_numpy(rgb).cuda(), torch.from_numpy(sources).cuda(), intrinsic=K, T_ref=T_ref, T_sources=T_src,
                                       **mc.TRUTH_PARAMS)
        assert depth.is_cuda and index.is_cuda
        want = mr.multiview_sgm(rgb, sources, plane_sweep_views(K, T_ref, K, T_src), **mc.TRUTH_PARAMS)
        _same((index.cpu().numpy(), depth.cpu().numpy()), want)
        filtered = v.filter_shadow_points(depth)
        assert filtered.is_cuda
        v.integrate(RGBDImage(torch.from_numpy(rgb).cuda(), filtered, 1.0, 4.0), K, T_ref)
        assert v.num_blocks() > 10
    finally:
        v.close()


def test_monocular_keyframes_reach_the_tsdf_through_the_front():
    """kVolumetricIntegrationDepthEstimatorType = "DEPTH_MVS_HIP": keyframes without depth and without a right image -> the first is
    skipped (no earlier keyframe), the later ones -> hv_mvs_sgm against the ring -> depth as a CUDA tensor -> shadow filter -> TSDF
    fusion; the index of the last keyframe equals the restatement's on the same sources."""
    import torch

    from pyslam_amd.dense.parameters import Parameters
    from pyslam_amd.dense.volumetric_integrator_base import VolumetricIntegrationKeyframeData
    from pyslam_amd.dense.volumetric_integrator_tsdf import VolumetricIntegratorTsdf
    from pyslam_amd.dense.volumetric_integrator_types import DatasetEnvironmentType, SensorType
    from pyslam_amd.depth_estimation import DepthEstimatorMvs
    from pyslam_amd.prep import plane_sweep_views
    from pyslam_amd.synthetic import SyntheticRGBD
    from pyslam_amd.volumetric import RGBDImage
    from tests import dense_helpers as dh

    names = ("kVolumetricIntegrationUseDepthEstimator", "kVolumetricIntegrationDepthEstimatorType", "kVolumetricIntegrationVoxelLength",
             "kVolumetricIntegrationTSdfTrunc", "kVolumetricIntegrationOutputTimeInterval", "kVolumetricIntegrationHipMaxBlocks",
             "kVolumetricIntegrationMvsNumPlanes", "kVolumetricIntegrationMvsMinDepth", "kVolumetricIntegrationMvsMinBaseline",
             "kVolumetricIntegrationMvsMaxBaseline")
    saved = {k: getattr(Parameters, k) for k in names}
    Parameters.kVolumetricIntegrationVoxelLength, Parameters.kVolumetricIntegrationTSdfTrunc = 0.02, 0.08
    Parameters.kVolumetricIntegrationOutputTimeInterval, Parameters.kVolumetricIntegrationHipMaxBlocks = 0.0, 1 << 13
    Parameters.kVolumetricIntegrationUseDepthEstimator, Parameters.kVolumetricIntegrationDepthEstimatorType = True, "DEPTH_MVS_HIP"
    Parameters.kVolumetricIntegrationMvsNumPlanes, Parameters.kVolumetricIntegrationMvsMinDepth = 32, 1.0
    Parameters.kVolumetricIntegrationMvsMinBaseline, Parameters.kVolumetricIntegrationMvsMaxBaseline = 0.1, 0.3
    try:
        s = SyntheticRGBD(mc.TRUTH_CONFIG, noise=False, invalid_frac=0.0)
        cam = dh.FakeCamera(s)
        integ = VolumetricIntegratorTsdf.__new__(VolumetricIntegratorTsdf)
        integ.init(cam, DatasetEnvironmentType.INDOOR, SensorType.MONOCULAR, {}, {})
        assert integ.depth_estimator is None and integ.depth_estimator_pending
        frames = []
        for i in (130, 140, 150):
            kf = dh.FakeKeyFrame(i, s, cam)
            kf.depth_img = None
            kd = VolumetricIntegrationKeyframeData(kf, kf.img, None, None)
            color, depth, _, _, _ = integ.estimate_depth_if_needed_and_rectify(kd)
            frames.append((kf.img, kd.pose))
            if i == 130:
                assert color is None and depth is None  # nothing to match against yet: skipped
                continue
            assert isinstance(depth, torch.Tensor) and depth.is_cuda
            rgbd = RGBDImage.create_from_color_and_depth(color, depth, depth_scale=1.0, depth_trunc=4.0, convert_rgb_to_intensity=False)
            integ.volume.integrate(rgbd, integ.o3d_camera, kd.pose)
        est = integ.depth_estimator
        assert isinstance(est, DepthEstimatorMvs) and est.sources_used == (0, 1) and est.index_map.is_cuda
        (img_a, T_a), (img_b, T_b), (img_ref, T_ref) = frames
        views = plane_sweep_views(s.intrinsics, T_ref, s.intrinsics, np.stack([T_b, T_a]))
        want = mr.multiview_sgm(img_ref, [img_b, img_a], views, num_planes=32, min_depth=1.0)
        np.testing.assert_array_equal(est.index_map.cpu().numpy(), want[0])
        assert integ.volume.num_blocks() > 10
    finally:
        for k, val in saved.items():
            setattr(Parameters, k, val)


def test_ground_truth(vol):
    """The matcher against the synthetic room's true depth (mvs_cases.synthetic_triple: pose 150 with the poses 140 and 130 as
    sources, 32 planes down to 1 m).  Measured with the restatement, which the kernels equal bit for bit
    (tests/test_mvs_reference_cpu.py): valid 0.7723, off by more than one plane step 0.1205, median error 0.335 plane steps.
    Asserted with the margins of the stereo matcher's ground-truth test: valid >= measured - 0.05, off <= 1.5 measured."""
    from pyslam_amd.prep import plane_sweep_views

    rgb, sources, depth_true, T_ref, T_src, s = mc.synthetic_triple()
    views = plane_sweep_views(s.intrinsics, T_ref, s.intrinsics, T_src)
    index, _ = vol.multiview_sgm(rgb, sources, views, **mc.TRUTH_PARAMS)
    valid, off, median = mc.truth_figures(index, depth_true, mc.TRUTH_PARAMS["min_depth"], mc.TRUTH_PARAMS["max_depth"], mc.TRUTH_PARAMS["num_planes"])
    print(f"valid {valid:.4f}, off by > 1 plane step {off:.4f}, median error {median:.3f} steps")
    assert valid >= mc.TRUTH_MEASURED[0] - 0.05
    assert off <= 1.5 * mc.TRUTH_MEASURED[1]
    assert median <= 1.5 * mc.TRUTH_MEASURED[2]
