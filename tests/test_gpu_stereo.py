"""GPU: _Volume.stereo_sgm (hv_stereo_sgm) against the numpy restatement (tests/stereo_reference.py), bit for bit - the int16
disparity with assert_array_equal, the depth as uint32 views - at the shapes where the kernels change form (stereo_cases.SHAPES)."""
import ctypes

import numpy as np
import pytest

from pyslam_amd import _lib as L
from tests import stereo_cases as sc
from tests import stereo_reference as sr

pytestmark = pytest.mark.gpu

BF = 14.4375  # fx * baseline of the tiny synthetic pair, exactly representable in float32


@pytest.fixture(scope="module")
def vol():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    v = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)
    yield v
    v.close()


def _same(got, want):
    (disp, depth), (rdisp, rdepth) = got, want
    assert disp.dtype == np.int16 and disp.shape == rdisp.shape
    np.testing.assert_array_equal(disp, rdisp)
    if rdepth is None:
        assert depth is None
    else:
        assert depth.dtype == np.float32
        np.testing.assert_array_equal(depth.view(np.uint32), rdepth.view(np.uint32))


def _check(vol, left, right, **kw):
    _same(vol.stereo_sgm(left, right, **kw), sr.stereo_sgm(left, right, **kw))


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "%dx%d_D%d" % s)
def test_matches_the_restatement_at_every_kernel_form(vol, shape, channels, paths):
    H, W, D = shape
    left, right = sc.textured_pair(H, W, channels, seed=H * 1000 + W + D)
    _check(vol, left, right, num_disparities=D, paths=paths, bf=BF, min_depth=0.5, max_depth=6.0)


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("channels", [1, 3])
def test_golden_pair(vol, channels, paths):
    left, right, golden = sc.load_golden()
    if channels == 3:
        left, right = (np.ascontiguousarray(np.repeat(a[..., None], 3, axis=2)) for a in (left, right))  # rule 1: (g + 2 g + g + 2) >> 2 = g
    disp, depth = vol.stereo_sgm(left, right, paths=paths, bf=BF, **sc.GOLDEN_PARAMS)
    if paths == 8:
        np.testing.assert_array_equal(disp, golden)
    _same((disp, depth), sr.stereo_sgm(left, right, paths=paths, bf=BF, **sc.GOLDEN_PARAMS))


@pytest.mark.parametrize("kw", [dict(uniqueness_ratio=0), dict(max_diff=-1), dict(p1=1023, p2=1023), dict(uniqueness_ratio=99, max_diff=0)],
                         ids=["uniqueness0", "no_left_right", "penalties_1023", "strict"])
def test_rule_switches(vol, kw):
    left, right = sc.textured_pair(37, 83, 3, seed=5)
    _check(vol, left, right, num_disparities=48, bf=BF, **kw)


def test_constant_pair_takes_the_smallest_disparity(vol):
    """Every cost ties: rule 5's smallest d decides, for the left and for the right image."""
    left = np.full((21, 70), 117, np.uint8)
    want = sr.stereo_sgm(left, left, num_disparities=32, bf=BF)
    assert (want[0] == 0).all() and (want[1] == 0).all()  # d* = 0 everywhere: depth 0 by rule 10
    _same(vol.stereo_sgm(left, left, num_disparities=32, bf=BF), want)


def test_planted_shift_and_outputs_on_demand(vol):
    left, right = sc.planted_shift()
    disp, depth = vol.stereo_sgm(left, right, num_disparities=32)
    assert depth is None
    np.testing.assert_array_equal(disp, sr.stereo_sgm(left, right, num_disparities=32)[0])
    inner = disp[:, 11 + 4:left.shape[1] - 4].astype(np.int32)
    assert (inner >= 0).all() and np.abs(inner - 16 * 11).max() <= 8


def test_device_tensors_agree_with_host_arrays(vol):
    import torch

    left, right = sc.textured_pair(37, 83, 3, seed=9)
    kw = dict(num_disparities=64, bf=BF, min_depth=0.3)
    host = vol.stereo_sgm(left, right, **kw)
    dev = vol.stereo_sgm(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), **kw)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in dev)
    assert dev[0].dtype == torch.int16 and dev[1].dtype == torch.float32
    _same((dev[0].cpu().numpy(), dev[1].cpu().numpy()), host)
    _same(host, sr.stereo_sgm(left, right, **kw))
    only_disp = vol.stereo_sgm(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), num_disparities=64)
    assert only_disp[1] is None
    np.testing.assert_array_equal(only_disp[0].cpu().numpy(), host[0])


def test_scratch_regrowth():
    """Two calls of different (H, W, D) on one volume - the second needs more scratch, the third less - against fresh volumes."""
    from pyslam_amd.volumetric import VoxelBlockGrid

    calls = [((19, 70), 16), ((37, 83), 128), ((24, 40), 32)]
    pairs = [sc.textured_pair(h, w, 1, seed=h) for (h, w), _ in calls]
    one = VoxelBlockGrid(0.02)  # any mode: the matcher reads nothing of the volume
    try:
        for (left, right), (_, D) in zip(pairs, calls):
            fresh = VoxelBlockGrid(0.02)
            try:
                want = fresh.stereo_sgm(left, right, num_disparities=D, bf=BF)
            finally:
                fresh.close()
            _same(one.stereo_sgm(left, right, num_disparities=D, bf=BF), want)
            _same(want, sr.stereo_sgm(left, right, num_disparities=D, bf=BF))
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
        left, right = sc.textured_pair(37, 83, 3, seed=3)
        _check(v, left, right, num_disparities=32, bf=BF)
        assert len(v.dirty_keys()) == 0
        for a, b in zip(before, v.dump()):
            np.testing.assert_array_equal(a, b)
    finally:
        v.close()


def _raw_call(vol, left, right, H, W, C, prm, disp, depth):
    return vol._lib.hv_stereo_sgm(vol._h, L.ptr(left), L.ptr(right), H, W, C, ctypes.byref(prm) if prm is not None else None, L.ptr(disp),
                                  L.ptr(depth), L.HV_HOST)


GOOD = dict(num_disparities=32, p1=10, p2=120, uniqueness_ratio=15, max_diff=1, paths=8, bf=BF, min_depth=0.0, max_depth=np.inf)
BAD_PARAMS = [dict(num_disparities=0), dict(num_disparities=24), dict(num_disparities=272), dict(p1=0), dict(p1=121), dict(p2=1024),
              dict(uniqueness_ratio=-1), dict(uniqueness_ratio=100), dict(paths=5), dict(paths=2), dict(bf=0.0), dict(bf=-1.0),
              dict(bf=np.inf), dict(bf=np.nan)]


def test_invalid_arguments_write_nothing(vol):
    H, W = 12, 40
    left, right = sc.textured_pair(H, W, 1, seed=1)
    disp = np.full((H, W), 0x5A5A, np.int16)
    depth = np.full((H, W), -77.0, np.float32)

    def refused(rc):
        assert rc == -1, rc  # HV_ERR_INVALID
        assert (disp == 0x5A5A).all() and (depth == -77.0).all()
        with pytest.raises(L.HipVolError):
            L.check(rc)

    for bad in BAD_PARAMS:
        refused(_raw_call(vol, left, right, H, W, 1, L.HvStereoParams(**{**GOOD, **bad}), disp, depth))
    good = L.HvStereoParams(**GOOD)
    refused(_raw_call(vol, None, right, H, W, 1, good, disp, depth))
    refused(_raw_call(vol, left, None, H, W, 1, good, disp, depth))
    refused(_raw_call(vol, left, right, H, W, 1, None, disp, depth))
    refused(_raw_call(vol, left, right, H, W, 1, good, None, None))
    for C in (0, 2, 4):
        refused(_raw_call(vol, left, right, H, W, C, good, disp, depth))
    for h, w in ((0, W), (H, 0), (-1, W)):
        refused(_raw_call(vol, left, right, h, w, 1, good, disp, depth))
    # a bad bf is no error when no depth is asked for, and the good call goes through
    assert _raw_call(vol, left, right, H, W, 1, L.HvStereoParams(**{**GOOD, "bf": 0.0}), disp, None) == 0
    np.testing.assert_array_equal(disp, sr.stereo_sgm(left, right, num_disparities=32)[0])
    assert (depth == -77.0).all()
    for bad in (dict(num_disparities=24), dict(paths=3), dict(p1=0), dict(uniqueness_ratio=100), dict(bf=-1.0)):
        with pytest.raises(ValueError):  # the binding refuses the same arguments before it calls
            vol.stereo_sgm(left, right, **{**dict(num_disparities=32, bf=BF), **bad})


def test_stereo_keyframes_reach_the_tsdf_on_the_device():
    """kVolumetricIntegrationDepthEstimatorType = "DEPTH_SGM_HIP": a stereo keyframe without depth -> hv_stereo_sgm -> depth as a CUDA
    tensor -> shadow filter -> TSDF fusion; the volume equals the one fused from the restatement's depth taken through numpy."""
    import torch

    from pyslam_amd.dense.parameters import Parameters
    from pyslam_amd.dense.volumetric_integrator_base import VolumetricIntegrationKeyframeData
    from pyslam_amd.dense.volumetric_integrator_tsdf import VolumetricIntegratorTsdf
    from pyslam_amd.dense.volumetric_integrator_types import DatasetEnvironmentType, SensorType
    from pyslam_amd.depth_estimation import DepthEstimatorSgm
    from pyslam_amd.volumetric import RGBDImage
    from tests import dense_helpers as dh

    saved = {k: getattr(Parameters, k) for k in ("kVolumetricIntegrationUseDepthEstimator", "kVolumetricIntegrationDepthEstimatorType",
                                                 "kVolumetricIntegrationVoxelLength", "kVolumetricIntegrationTSdfTrunc",
                                                 "kVolumetricIntegrationOutputTimeInterval", "kVolumetricIntegrationHipMaxBlocks")}
    Parameters.kVolumetricIntegrationVoxelLength, Parameters.kVolumetricIntegrationTSdfTrunc = 0.02, 0.08
    Parameters.kVolumetricIntegrationOutputTimeInterval, Parameters.kVolumetricIntegrationHipMaxBlocks = 0.0, 1 << 13
    Parameters.kVolumetricIntegrationUseDepthEstimator = True
    Parameters.kVolumetricIntegrationDepthEstimatorType = "DEPTH_SGM_HIP"
    try:
        s = sc.synthetic_pair(0)[4]
        cam = dh.FakeCamera(s)
        cam.bf = BF

        class Restated:  # the same contract, through numpy
            disparity_map = None

            def infer(self, image, image_right=None):
                self.disparity_map, depth = sr.stereo_sgm(image, image_right, bf=BF)
                return depth, None

        dev = VolumetricIntegratorTsdf.__new__(VolumetricIntegratorTsdf)
        dev.init(cam, DatasetEnvironmentType.INDOOR, SensorType.STEREO, {}, {})
        host = VolumetricIntegratorTsdf.__new__(VolumetricIntegratorTsdf)
        host.init(cam, DatasetEnvironmentType.INDOOR, SensorType.STEREO, {}, dict(depth_estimator_factory=lambda c: Restated()))
        assert dev.depth_estimator is None and isinstance(host.depth_estimator, Restated)  # an injected factory keeps precedence
        for i in (0, 150):
            rgb_left, rgb_right, _, T_cw, _ = sc.synthetic_pair(i)
            kf = dh.FakeKeyFrame(i, s, cam)
            kf.depth_img = None
            kf.img, kf.img_right = np.ascontiguousarray(rgb_left[..., ::-1]), np.ascontiguousarray(rgb_right[..., ::-1])
            for integ in (dev, host):
                kd = VolumetricIntegrationKeyframeData(kf, kf.img, kf.img_right, None)
                color, depth, _, _, _ = integ.estimate_depth_if_needed_and_rectify(kd)
                assert (isinstance(depth, torch.Tensor) and depth.is_cuda) == (integ is dev)
                rgbd = RGBDImage.create_from_color_and_depth(color, depth, depth_scale=1.0, depth_trunc=4.0, convert_rgb_to_intensity=False)
                integ.volume.integrate(rgbd, integ.o3d_camera, kd.pose)
        assert isinstance(dev.depth_estimator, DepthEstimatorSgm)
        assert dev.depth_estimator.disparity_map.is_cuda
        np.testing.assert_array_equal(dev.depth_estimator.disparity_map.cpu().numpy(), host.depth_estimator.disparity_map)
        for a, b in zip(dev.volume.dump(), host.volume.dump()):
            np.testing.assert_array_equal(a, b)
        assert dev.volume.num_blocks() > 10
    finally:
        for k, val in saved.items():
            setattr(Parameters, k, val)
