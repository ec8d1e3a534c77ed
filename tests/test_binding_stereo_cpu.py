"""What stereo_sgm sends over the C ABI, pinned against the recording stand-in for the library (tests/recording_lib.py; no GPU), in
the manner of tests/test_binding_calls_cpu.py, whose list of exercised public methods these tests extend; DepthEstimatorSgm's
contract; and the dense front's choice of the estimator."""
import types

import numpy as np
import pytest

from pyslam_amd import _lib as L
from pyslam_amd import volumetric as V
from pyslam_amd import volumetric_semantic as S
from tests.recording_lib import ref, volume
from tests.test_binding_calls_cpu import ANY, P, REF, covers, expect, host, refused, shaped, tsdf  # noqa: F401 (host: a fixture)

H, W = 6, 20
FIELDS = ("num_disparities", "p1", "p2", "uniqueness_ratio", "max_diff", "paths", "bf", "min_depth", "max_depth")


def pair(channels=3, seed=0):
    rng = np.random.default_rng(seed)
    shape = (H, W) if channels == 1 else (H, W, channels)
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)


def params(call):
    p = ref(call[1][6])
    return {f: getattr(p, f) for f in FIELDS}


@pytest.mark.parametrize("channels", [1, 3])
@covers("stereo_sgm")
def test_stereo_sgm_defaults_and_result_kinds(channels):
    left, right = pair(channels)
    for vol in (tsdf(), volume(V.VoxelBlockGrid, voxel_size=0.05, block_size=8), volume(S.VoxelBlockSemanticGrid, voxel_size=0.05, block_size=8)):
        disp, depth = vol.stereo_sgm(left, right)
        call, = expect(vol, ("hv_stereo_sgm", P(left), P(right), H, W, channels, REF(L.HvStereoParams), P(disp), None, L.HV_HOST))
        assert depth is None  # no bf: no depth asked for
        shaped(disp, (H, W), np.int16)
        assert params(call) == dict(num_disparities=128, p1=10, p2=120, uniqueness_ratio=15, max_diff=1, paths=8, bf=0.0, min_depth=0.0,
                                    max_depth=np.inf)


@covers("stereo_sgm")
def test_stereo_sgm_marshals_every_argument(host):
    left, right = pair()
    a, b = host(left), host(right)
    vol = tsdf()
    disp, depth = vol.stereo_sgm(a, b, num_disparities=48, p1=7, p2=99, uniqueness_ratio=0, max_diff=-1, paths=4, bf=14.4375, min_depth=0.25,
                                 max_depth=6.5)
    call, = expect(vol, ("hv_stereo_sgm", P(left), P(right), H, W, 3, REF(L.HvStereoParams), P(disp), P(depth), L.HV_HOST))
    shaped(disp, (H, W), np.int16), shaped(depth, (H, W), np.float32)  # host operands of either kind: numpy results
    assert params(call) == dict(num_disparities=48, p1=7, p2=99, uniqueness_ratio=0, max_diff=-1, paths=4, bf=14.4375, min_depth=0.25,
                                max_depth=6.5)
    assert all(type(x) is int for x in call[1][3:6])
    # strided views are made contiguous for the call; numpy integers are plain ints by then
    wide = np.zeros((H, 2 * W, 3), np.uint8)
    disp, _ = vol.stereo_sgm(wide[:, ::2], wide[:, 1::2], num_disparities=np.int64(16), paths=np.int32(8))
    call, = expect(vol, ("hv_stereo_sgm", ANY, ANY, H, W, 3, REF(L.HvStereoParams), P(disp), None, L.HV_HOST))
    assert params(call)["num_disparities"] == 16 and params(call)["paths"] == 8


@covers("stereo_sgm")
def test_stereo_sgm_refusals_come_before_any_call():
    left, right = pair()
    vol = tsdf()
    for bad in (0, 8, 24, 272, -16):
        refused(vol, ValueError, "stereo_sgm: num_disparities must be a multiple of 16 in 16..256", vol.stereo_sgm, left, right, num_disparities=bad)
    for p1, p2 in ((0, 10), (-1, 10), (11, 10), (10, 1024)):
        refused(vol, ValueError, "stereo_sgm: need 0 < p1 <= p2 <= 1023", vol.stereo_sgm, left, right, p1=p1, p2=p2)
    for bad in (-1, 100):
        refused(vol, ValueError, "stereo_sgm: uniqueness_ratio must be in 0..99", vol.stereo_sgm, left, right, uniqueness_ratio=bad)
    for bad in (0, 2, 5, 16):
        refused(vol, ValueError, "stereo_sgm: paths must be 4 or 8", vol.stereo_sgm, left, right, paths=bad)
    for bad in (0.0, -1.0, np.inf, np.nan, 1e39):
        refused(vol, ValueError, "stereo_sgm: bf must be finite and positive", vol.stereo_sgm, left, right, bf=bad)
    refused(vol, ValueError, "stereo_sgm: images must have 1 or 3 channels, got 2", vol.stereo_sgm, left[..., :2], right[..., :2])
    refused(vol, ValueError, "stereo_sgm: images must have 1 or 3 channels, got 4", vol.stereo_sgm, np.zeros((H, W, 4), np.uint8),
            np.zeros((H, W, 4), np.uint8))
    refused(vol, ValueError, "stereo_sgm: empty image", vol.stereo_sgm, left[:0], right[:0])
    refused(vol, ValueError, "stereo_sgm: empty image", vol.stereo_sgm, left[:, :0], right[:, :0])
    refused(vol, ValueError, "must be two images of one shape", vol.stereo_sgm, left, right[:, :-1])
    refused(vol, ValueError, "must be two images of one shape", vol.stereo_sgm, left.ravel(), right.ravel())
    refused(vol, ValueError, "stereo_sgm: the images must be uint8", vol.stereo_sgm, left.astype(np.float32), right)
    refused(vol, ValueError, "stereo_sgm: the images must be uint8", vol.stereo_sgm, left, right.astype(np.int16))


def test_depth_estimator_sgm_contract():
    from pyslam_amd.depth_estimation import DepthEstimatorSgm, DepthEstimatorStereoTorch

    left, right = pair()
    vol = tsdf()
    cam = types.SimpleNamespace(bf=14.4375)
    est = DepthEstimatorSgm(vol, cam, keep_on_device=False, min_depth=0.5, max_depth=7.0, num_disparities=32, paths=4)
    assert est.disparity_map is None
    depth, pts3d = est.infer(left, right)
    call, = expect(vol, ("hv_stereo_sgm", P(left), P(right), H, W, 3, REF(L.HvStereoParams), P(est.disparity_map), P(depth), L.HV_HOST))
    assert pts3d is None
    shaped(depth, (H, W), np.float32), shaped(est.disparity_map, (H, W), np.int16)
    assert params(call) == dict(num_disparities=32, p1=10, p2=120, uniqueness_ratio=15, max_diff=1, paths=4, bf=14.4375, min_depth=0.5,
                                max_depth=7.0)
    with pytest.raises(ValueError) as e:
        est.infer(left)
    stub = DepthEstimatorStereoTorch.__new__(DepthEstimatorStereoTorch)
    with pytest.raises(ValueError) as e2:
        stub.infer(left, None)
    assert str(e.value) == str(e2.value) and vol._lib.calls == []


def test_dense_front_selects_the_estimator_by_type(monkeypatch):
    from pyslam_amd.dense.parameters import Parameters
    from pyslam_amd.dense.volumetric_integrator_base import VolumetricIntegratorBase
    from pyslam_amd.depth_estimation import DepthEstimatorSgm

    cam = types.SimpleNamespace(fx=100.0, fy=100.0, cx=10.0, cy=3.0, width=W, height=H, D=np.zeros(5), bf=14.4375)
    saved = Parameters.kVolumetricIntegrationUseDepthEstimator, Parameters.kVolumetricIntegrationDepthEstimatorType
    try:
        def front(kind, use=True, **kwargs):
            Parameters.kVolumetricIntegrationUseDepthEstimator, Parameters.kVolumetricIntegrationDepthEstimatorType = use, kind
            integ = VolumetricIntegratorBase.__new__(VolumetricIntegratorBase)
            integ.init(cam, None, None, {}, kwargs)
            return integ

        injected = object()
        assert front("DEPTH_SGM_HIP", depth_estimator_factory=lambda c: injected).depth_estimator is injected  # keeps precedence
        assert not front("DEPTH_SGM_HIP", depth_estimator_factory=lambda c: injected).depth_estimator_pending
        for kind in ("DEPTH_SGBM", "DEPTH_RAFT_STEREO"):  # as before: pySLAM's factory when it is importable, else none
            integ = front(kind)
            assert integ.depth_estimator is None and not integ.depth_estimator_pending
        assert not front("DEPTH_SGM_HIP", use=False).depth_estimator_pending
        integ = front("DEPTH_SGM_HIP")
        assert integ.depth_estimator is None and integ.depth_estimator_pending  # the volume does not exist yet
        integ.volume = tsdf()
        left, right = pair()
        kd = types.SimpleNamespace(img=left, img_right=right, depth=None, id=3, semantic_img=None, semantic_instances_img=None)
        seen = []
        # (the estimator the front makes keeps its images on the GPU: stand in for the upload and the call)
        monkeypatch.setattr(DepthEstimatorSgm, "infer", lambda self, img, img_right=None: (seen.append((img, img_right)), (np.ones((H, W), np.float32), None))[1])
        monkeypatch.setattr(Parameters, "kVolumetricIntegrationDepthEstimationFilterShadowPoints", False, raising=False)
        color, depth, pts3d, _, _ = integ.estimate_depth_if_needed_and_rectify(kd)
        assert isinstance(integ.depth_estimator, DepthEstimatorSgm) and integ.depth_estimator.volume is integ.volume
        assert integ.depth_estimator.camera is cam and integ.depth_estimator.keep_on_device
        assert not integ.depth_estimator_pending and 3 in integ.img_id_to_depth and seen[0][0] is left and seen[0][1] is right
        shaped(depth, (H, W), np.float32)
    finally:
        Parameters.kVolumetricIntegrationUseDepthEstimator, Parameters.kVolumetricIntegrationDepthEstimatorType = saved
