"""What filter_speckles and stereo_sgm's speckle arguments send over the C ABI, pinned against the recording stand-in for the library
(tests/recording_lib.py; no GPU), in the manner of tests/test_binding_stereo_cpu.py; DepthEstimatorSgm forwarding the two arguments;
the dense front reading its two parameters."""
import types

import numpy as np

from pyslam_amd import _lib as L
from pyslam_amd import volumetric as V
from pyslam_amd import volumetric_semantic as S
from tests.recording_lib import ref, volume
from tests.test_binding_calls_cpu import P, REF, covers, expect, host, refused, shaped, tsdf  # noqa: F401 (host: a fixture)
from tests.test_binding_stereo_cpu import pair, params

H, W = 6, 20


def images(seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(-16, 400, (H, W)).astype(np.int16), rng.random((H, W)).astype(np.float32)


@covers("filter_speckles")
def test_filter_speckles_defaults_and_result_kinds(host):
    disp, depth = images()
    for vol in (tsdf(), volume(V.VoxelBlockGrid, voxel_size=0.05, block_size=8), volume(S.VoxelBlockSemanticGrid, voxel_size=0.05, block_size=8)):
        out = vol.filter_speckles(host(disp), 50, 16)
        expect(vol, ("hv_filter_speckles", P(disp), L.HV_SPECKLE_I16, H, W, -16.0, 50, 16.0, P(out), None, None, None, L.HV_HOST))
        shaped(out, (H, W), np.int16)  # the image alone: an array, not a result object
        out = vol.filter_speckles(host(depth), 200, 0.05)
        expect(vol, ("hv_filter_speckles", P(depth), L.HV_SPECKLE_F32, H, W, 0.0, 200, 0.05, P(out), None, None, None, L.HV_HOST))
        shaped(out, (H, W), np.float32)


@covers("filter_speckles")
def test_filter_speckles_marshals_every_argument(host):
    disp, depth = images()
    before = depth.copy()
    vol = tsdf()
    vol._lib.script("hv_filter_speckles")
    r = vol.filter_speckles(host(disp), np.int64(7), np.float32(32.0), new_val=0, depth=host(depth), labels=True, stats=True)
    call, = expect(vol, ("hv_filter_speckles", P(disp), L.HV_SPECKLE_I16, H, W, 0.0, 7, 32.0, P(r.image), P(r.depth), P(r.labels),
                         REF(L.HvSpeckleStats), L.HV_HOST))
    assert isinstance(r, V.SpeckleResult) and isinstance(r.stats, V.SpeckleStats)
    assert [type(a) for a in call[1][2:8]] == [int, int, int, float, int, float]
    shaped(r.image, (H, W), np.int16), shaped(r.depth, (H, W), np.float32), shaped(r.labels, (H, W), np.int32)
    # the companion is written in place by the library: the caller's array is another one and keeps its bits
    assert r.depth is not depth and not np.shares_memory(r.depth, depth) and np.array_equal(r.depth, before) and np.array_equal(depth, before)
    # the stats arrive field by field under their own names
    st = ref(call[1][11])
    for i, (name, _) in enumerate(L.HvSpeckleStats._fields_):
        setattr(st, name, 100 + i)
    assert V._stats(V.SpeckleStats, st).as_tuple() == (100, 101, 102, 103, 104)
    assert V.SpeckleStats.__slots__ == tuple(name for name, _ in L.HvSpeckleStats._fields_)
    # each extra on its own gives the result object, with the others None
    r = vol.filter_speckles(disp, 7, 16, labels=True)
    expect(vol, ("hv_filter_speckles", P(disp), 0, H, W, -16.0, 7, 16.0, P(r.image), None, P(r.labels), None, L.HV_HOST))
    assert r.depth is None and r.stats is None
    r = vol.filter_speckles(disp, 7, 16, stats=True)
    expect(vol, ("hv_filter_speckles", P(disp), 0, H, W, -16.0, 7, 16.0, P(r.image), None, None, REF(L.HvSpeckleStats), L.HV_HOST))
    assert r.labels is None and r.stats == V.SpeckleStats()
    # a strided view is made contiguous for the call
    wide = np.zeros((H, 2 * W), np.float32)
    out = vol.filter_speckles(wide[:, ::2], 3, 0.5, new_val=-1.0)
    call, = expect(vol, ("hv_filter_speckles", ("p", "any"), L.HV_SPECKLE_F32, H, W, -1.0, 3, 0.5, P(out), None, None, None, L.HV_HOST))


@covers("filter_speckles")
def test_filter_speckles_refusals_come_before_any_call():
    disp, depth = images()
    vol = tsdf()
    f = vol.filter_speckles
    for bad in (disp.astype(np.int32), disp.astype(np.uint16), depth.astype(np.float64), disp.astype(np.uint8)):
        refused(vol, ValueError, "filter_speckles: the image must be int16 or float32", f, bad, 5, 16)
    refused(vol, ValueError, "filter_speckles: the image must be [H, W]", f, disp.ravel(), 5, 16)
    refused(vol, ValueError, "filter_speckles: the image must be [H, W]", f, disp[None], 5, 16)
    refused(vol, ValueError, "filter_speckles: bad image size", f, disp[:0], 5, 16)
    refused(vol, ValueError, "filter_speckles: bad image size", f, disp[:, :0], 5, 16)
    refused(vol, ValueError, "filter_speckles: bad image size", f, np.zeros((1, 32769), np.int16), 5, 16)
    for bad in (-1, 2.5):
        refused(vol, ValueError, "filter_speckles: max_speckle_size must be an integer >= 0", f, disp, bad, 16)
    for bad in (-1, -0.5, np.nan, np.inf):
        refused(vol, ValueError, "filter_speckles: max_diff must be finite and not negative", f, disp, 5, bad)
        refused(vol, ValueError, "filter_speckles: max_diff must be finite and not negative", f, depth, 5, bad)
    refused(vol, ValueError, "filter_speckles: max_diff must be finite and not negative", f, disp, 5, 65536)
    assert f(depth, 5, 65536.0) is not None and vol._lib.calls.pop()[0] == "hv_filter_speckles"  # (a float32 image has no such cap)
    assert f(disp, 5, 65535) is not None and vol._lib.calls.pop()[0] == "hv_filter_speckles"
    for bad in (0.5, 32768, -32769, np.nan):
        refused(vol, ValueError, "filter_speckles: new_val of an int16 image must be an integer in -32768..32767", f, disp, 5, 16, new_val=bad)
    refused(vol, ValueError, "filter_speckles: depth must be float32", f, disp, 5, 16, depth=depth.astype(np.float64))
    refused(vol, ValueError, "filter_speckles: depth (6, 19) must have the image's shape", f, disp, 5, 16, depth=depth[:, :-1])


@covers("stereo_sgm")
def test_stereo_sgm_window_chooses_the_entry_point(host):
    left, right = pair()
    vol = tsdf()
    # window 0, given or not: today's call, argument for argument
    for kw in ({}, dict(speckle_window_size=0), dict(speckle_window_size=0, speckle_range=7), dict(speckle_window_size=np.int32(0))):
        disp, depth = vol.stereo_sgm(host(left), host(right), bf=14.4375, **kw)
        call, = expect(vol, ("hv_stereo_sgm", P(left), P(right), H, W, 3, REF(L.HvStereoParams), P(disp), P(depth), L.HV_HOST))
        assert len(call[1]) == 10
    disp, depth = vol.stereo_sgm(host(left), host(right), num_disparities=32, bf=14.4375, speckle_window_size=50)
    call, = expect(vol, ("hv_stereo_sgm_speckle", P(left), P(right), H, W, 3, REF(L.HvStereoParams), 50, 1, P(disp), P(depth), None, L.HV_HOST))
    shaped(disp, (H, W), np.int16), shaped(depth, (H, W), np.float32)
    assert params(call)["num_disparities"] == 32 and params(call)["bf"] == 14.4375
    disp, depth = vol.stereo_sgm(left, right, speckle_window_size=np.int64(200), speckle_range=np.int32(2))
    call, = expect(vol, ("hv_stereo_sgm_speckle", P(left), P(right), H, W, 3, REF(L.HvStereoParams), 200, 2, P(disp), None, None, L.HV_HOST))
    assert depth is None and [type(a) for a in call[1][7:9]] == [int, int]
    for bad in (-1, 2.5, (1 << 30) + 1):
        refused(vol, ValueError, "stereo_sgm: speckle_window_size must be an integer in 0..2^30", vol.stereo_sgm, left, right, speckle_window_size=bad)
    for bad in (-1, 0.5, 4096):
        refused(vol, ValueError, "stereo_sgm: speckle_range must be an integer in 0..4095", vol.stereo_sgm, left, right, speckle_window_size=50,
                speckle_range=bad)


def test_depth_estimator_sgm_forwards_the_speckle_arguments():
    from pyslam_amd.depth_estimation import DepthEstimatorSgm

    left, right = pair()
    vol = tsdf()
    est = DepthEstimatorSgm(vol, types.SimpleNamespace(bf=14.4375), keep_on_device=False, num_disparities=32, speckle_window_size=50)
    depth, _ = est.infer(left, right)
    expect(vol, ("hv_stereo_sgm_speckle", P(left), P(right), H, W, 3, REF(L.HvStereoParams), 50, 1, P(est.disparity_map), P(depth), None,
                 L.HV_HOST))
    est = DepthEstimatorSgm(vol, types.SimpleNamespace(bf=14.4375), keep_on_device=False, speckle_window_size=9, speckle_range=3)
    depth, _ = est.infer(left, right)
    expect(vol, ("hv_stereo_sgm_speckle", P(left), P(right), H, W, 3, REF(L.HvStereoParams), 9, 3, P(est.disparity_map), P(depth), None, L.HV_HOST))


def test_dense_front_passes_the_speckle_parameters(monkeypatch):
    from pyslam_amd.dense.parameters import Parameters
    from pyslam_amd.dense.volumetric_integrator_base import VolumetricIntegratorBase
    from pyslam_amd.depth_estimation import DepthEstimatorSgm

    cam = types.SimpleNamespace(fx=100.0, fy=100.0, cx=10.0, cy=3.0, width=W, height=H, D=np.zeros(5), bf=14.4375)
    monkeypatch.setattr(Parameters, "kVolumetricIntegrationUseDepthEstimator", True)
    monkeypatch.setattr(Parameters, "kVolumetricIntegrationDepthEstimatorType", "DEPTH_SGM_HIP")
    monkeypatch.setattr(Parameters, "kVolumetricIntegrationDepthEstimationFilterShadowPoints", False, raising=False)
    monkeypatch.setattr(DepthEstimatorSgm, "infer", lambda self, img, img_right=None: (np.ones((H, W), np.float32), None))
    left, right = pair()

    def estimator(**parameters):
        for name, value in parameters.items():
            monkeypatch.setattr(Parameters, name, value, raising=False)
        integ = VolumetricIntegratorBase.__new__(VolumetricIntegratorBase)
        integ.init(cam, None, None, {}, {})
        integ.volume = tsdf()
        kd = types.SimpleNamespace(img=left, img_right=right, depth=None, id=3, semantic_img=None, semantic_instances_img=None)
        integ.estimate_depth_if_needed_and_rectify(kd)
        assert isinstance(integ.depth_estimator, DepthEstimatorSgm) and integ.depth_estimator.volume is integ.volume
        return integ.depth_estimator

    assert not hasattr(Parameters, "kVolumetricIntegrationSgmSpeckleWindowSize")  # read with getattr: the defaults are 0 and 1
    assert estimator().sgm_params == {}  # the construction of before
    assert estimator(kVolumetricIntegrationSgmSpeckleWindowSize=50).sgm_params == dict(speckle_window_size=50, speckle_range=1)
    assert estimator(kVolumetricIntegrationSgmSpeckleWindowSize=50, kVolumetricIntegrationSgmSpeckleRange=4).sgm_params == dict(
        speckle_window_size=50, speckle_range=4)
    assert estimator(kVolumetricIntegrationSgmSpeckleWindowSize=0).sgm_params == {}  # the range alone does nothing
