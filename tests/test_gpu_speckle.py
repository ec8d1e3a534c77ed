"""GPU: _Volume.filter_speckles (hv_filter_speckles) and stereo_sgm's speckle arguments (hv_stereo_sgm_speckle) against the numpy
restatement (tests/speckle_reference.py), bit for bit: image, labels, depth companion and the five counts, on the planted cases of
tests/speckle_cases.py - regions inside a tile of the labelling kernel, across its seams and around a corner of four tiles."""
import ctypes
import functools
import types

import numpy as np
import pytest

from pyslam_amd import _lib as L
from tests import speckle_cases as pc
from tests import speckle_reference as pr
from tests import stereo_cases as sc
from tests import stereo_reference as sr
from tests.speckle_cases import BASE, INV

pytestmark = pytest.mark.gpu

BF = 14.4375  # fx * baseline of the tiny synthetic pair, exactly representable in float32


@pytest.fixture(scope="module")
def vol():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    v = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)
    yield v
    v.close()


@functools.lru_cache(maxsize=None)
def want_of(name):
    image, params = pc.planted(name)
    return pr.filter_speckles(image, method="union", **params)


def same(got, want):
    """got: a SpeckleResult of numpy arrays; want: the restatement's Result"""
    assert pr.same_bits(got.image, want.image), int((got.image != want.image).sum())
    np.testing.assert_array_equal(got.labels, want.labels)
    assert got.labels.dtype == np.int32
    assert got.stats.as_tuple() == pr.stats_tuple(want.stats), (got.stats, want.stats)
    if want.depth is None:
        assert got.depth is None
    else:
        assert pr.same_bits(got.depth, want.depth)


def check(vol, name):
    image, params = pc.planted(name)
    before = image.copy()
    got = vol.filter_speckles(image, labels=True, stats=True, **params)
    same(got, want_of(name))
    assert pr.same_bits(image, before)
    return got


def names(*prefixes):
    return [c[0] for c in pc.PLANTED if c[0].startswith(prefixes)]


# 1: the edges of the image and of the tile
@pytest.mark.parametrize("name", names("edges_"))
def test_edges_of_the_image_and_of_the_tile(vol, name):
    check(vol, name)


# 2 - 6, 8: the planted regions
@pytest.mark.parametrize("name", ["size_threshold", "diff_threshold", "ramp", "checkerboard_s1", "checkerboard_s0", "snake", "snake_raised",
                                  "snake_step", "comb", "extremes_d65535", "extremes_d65534", "extremes_newval_min", "near_invalid"])
def test_planted_regions(vol, name):
    got = check(vol, name)
    if name == "size_threshold":  # blobs of K go, of K + 1 stay: inside a tile, across either seam, around a corner of four tiles
        for small, large in pc.size_threshold()[1].values():
            assert all(got.image[p] == INV for p in small) and all(got.image[p] == BASE for p in large)
    if name == "ramp":
        assert got.stats.components == 1 and got.stats.removed_pixels == 0
    if name == "snake":
        assert got.stats.as_tuple() == (len(pc.snake()[1]), 1, len(pc.snake()[1]), 0, 0)


# 7: one component, kept at H W - 1 and removed at H W; once at a full frame, where the size passes 65535
@pytest.mark.parametrize("name", names("one_component_"))
def test_one_component(vol, name):
    got = check(vol, name)
    n = got.image.size
    assert got.stats.components == 1 and got.stats.largest == n
    assert got.stats.removed_pixels == (n if name.endswith("removed") else 0)


# 9: float32 with NaN, +inf and -0.0 against new_val 0.0
def test_float32(vol):
    got = check(vol, "float_depth")
    image = pc.planted("float_depth")[0]
    for p in ((2, 3), (2, 4), (5, 7), (6, 7), (9, 9), (11, 2)):  # NaN and inf: valid, alone, removed
        assert got.labels[p] == p[0] * image.shape[1] + p[1] and got.image[p] == 0.0
    assert got.labels[4, 20] == -1 and np.signbit(got.image[4, 20])
    for new_val, size, md in ((1.5, 3, 0.25), (np.nan, 2, 0.5), (0.0, 0, 0.0), (-1.0, 4, 1e30)):
        want = pr.filter_speckles(image, size, md, new_val=new_val, method="union")
        same(vol.filter_speckles(image, size, md, new_val=new_val, labels=True, stats=True), want)


# 10: the depth companion
def test_depth_companion(vol):
    image, params = pc.planted("companion")
    depth_before = params["depth"].copy()
    got = check(vol, "companion")
    assert pr.same_bits(params["depth"], depth_before)  # the caller's array is not written
    gone = (image != INV) & (got.image == INV)
    bits, before = got.depth.view(np.uint32), depth_before.view(np.uint32)
    assert gone.any() and (bits[gone] == 0).all() and np.array_equal(bits[~gone], before[~gone])
    assert (bits[~gone] == pc.NAN_PAYLOAD).any()
    only = vol.filter_speckles(image, params["max_speckle_size"], params["max_diff"], depth=params["depth"])  # no labels, no stats
    assert only.labels is None and only.stats is None and pr.same_bits(only.depth, got.depth) and pr.same_bits(only.image, got.image)


# 11: host arrays and device tensors; repeated calls
def test_device_tensors_agree_with_host_arrays(vol):
    import torch

    for name in ("companion", "float_depth", "snake"):
        image, params = pc.planted(name)
        kw = dict(params)
        depth = kw.pop("depth", None)
        d_image = torch.from_numpy(image.copy()).cuda()
        d_depth = torch.from_numpy(depth.copy()).cuda() if depth is not None else None
        runs = [vol.filter_speckles(d_image, depth=d_depth, labels=True, stats=True, **kw) for _ in range(3)]
        for r in runs:
            assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (r.image, r.labels)) and r.labels.dtype == torch.int32
            assert r.image.dtype == d_image.dtype and (r.depth is None) == (depth is None)
            host = types.SimpleNamespace(image=r.image.cpu().numpy(), labels=r.labels.cpu().numpy(), stats=r.stats,
                                         depth=None if r.depth is None else r.depth.cpu().numpy())
            same(host, want_of(name))
        assert pr.same_bits(d_image.cpu().numpy(), image)  # the inputs are never written
        if depth is not None:
            assert pr.same_bits(d_depth.cpu().numpy(), depth)
        plain = vol.filter_speckles(d_image, kw["max_speckle_size"], kw["max_diff"], new_val=kw["new_val"])
        assert isinstance(plain, torch.Tensor) and pr.same_bits(plain.cpu().numpy(), want_of(name).image)


# 12: scratch regrowth, the map, invalid arguments
def test_scratch_regrowth_and_a_map_left_alone():
    from pyslam_amd.synthetic import SyntheticRGBD
    from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume, VoxelBlockGrid

    s = SyntheticRGBD("tiny_160x120_2cm")
    v = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 12)
    g = VoxelBlockGrid(0.02)  # any mode: the filter reads nothing of the volume
    try:
        K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
        for i in range(2):
            depth, rgb, T = s[i]
            v.integrate(RGBDImage(rgb, depth, 1.0, 4.0), K, T)
        v.mark_merged()
        before = v.dump()
        assert len(before[0]) > 10
        for name in ("edges_1x7_s1_d16", "one_component_full_frame", "diff_threshold", "edges_1x1_s0_d0"):  # small, large, small
            check(v, name)
            check(g, name)
        assert len(v.dirty_keys()) == 0
        for a, b in zip(before, v.dump()):
            np.testing.assert_array_equal(a, b)
    finally:
        v.close()
        g.close()


def _raw(vol, image, kind, H, W, new_val, size, md, out, depth=None, labels=None, stats=None):
    return vol._lib.hv_filter_speckles(vol._h, L.ptr(image) if not isinstance(image, int) else image, kind, H, W, new_val, size, md,
                                       L.ptr(out) if not isinstance(out, int) else out, L.ptr(depth) if not isinstance(depth, int) else depth,
                                       L.ptr(labels) if not isinstance(labels, int) else labels, ctypes.byref(stats) if stats is not None else None,
                                       L.HV_HOST)


def test_invalid_arguments_write_nothing(vol):
    H, W = 12, 40
    image = pc.levels(H, W, seed=3)
    out = np.full((H, W), 0x5A5A, np.int16)
    depth = np.full((H, W), -77.0, np.float32)
    labels = np.full((H, W), 0x5A5A5A5A, np.int32)
    stats = L.HvSpeckleStats(7, 7, 7, 7, 7)
    I16, F32 = L.HV_SPECKLE_I16, L.HV_SPECKLE_F32

    def refused(rc):
        assert rc == -1, rc  # HV_ERR_INVALID
        assert (out == 0x5A5A).all() and (depth == -77.0).all() and (labels == 0x5A5A5A5A).all() and stats.valid_pixels == 7
        with pytest.raises(L.HipVolError):
            L.check(rc)

    good = dict(kind=I16, H=H, W=W, new_val=-16.0, size=5, md=16.0)
    call = lambda image=image, out=out, **kw: _raw(vol, image, out=out, depth=depth, labels=labels, stats=stats, **{**good, **kw})
    refused(call(image=None))
    refused(call(out=None))
    refused(vol._lib.hv_filter_speckles(None, L.ptr(image), I16, H, W, -16.0, 5, 16.0, L.ptr(out), None, None, None, L.HV_HOST))
    for kind in (-1, 2, 7):
        refused(call(kind=kind))
    for h, w in ((0, W), (H, 0), (-1, W), (32769, 1), (1, 32769), (32768, 32768)):
        refused(call(H=h, W=w))
    refused(call(size=-1))
    for md in (-1.0, -1e-30, np.nan, np.inf, -np.inf, 65536.0):
        refused(call(md=md))
    for nv in (0.5, 32768.0, -32769.0, np.nan):
        refused(call(new_val=nv))
    fimage = image.astype(np.float32)
    fout = np.full((H, W), -77.0, np.float32)
    for md in (-1.0, np.nan, np.inf):
        assert _raw(vol, fimage, F32, H, W, 0.0, 5, md, fout) == -1 and (fout == -77.0).all()
    # an output that overlaps the image, other than out == image exactly
    buf = np.zeros(2 * H * W + 8, np.int16)
    base = buf[:H * W]
    base[:] = image.ravel()
    address = lambda a, byte=0: a.ctypes.data + byte
    for shift in (2, 2 * W, 2 * H * W - 2):
        refused(call(image=base, out=address(base, shift)))
    refused(_raw(vol, base, I16, H, W, -16.0, 5, 16.0, out, depth=address(base), labels=labels, stats=stats))
    refused(_raw(vol, base, I16, H, W, -16.0, 5, 16.0, out, depth=depth, labels=address(base, 4), stats=stats))
    np.testing.assert_array_equal(base, image.ravel())
    # the good call goes through, and in place (out == image) it gives the same image
    want = pr.filter_speckles(image, 5, 16, method="union")
    assert call() == 0
    np.testing.assert_array_equal(out, want.image)
    np.testing.assert_array_equal(labels, want.labels)
    assert tuple(getattr(stats, k) for k in pr.STATS) == pr.stats_tuple(want.stats)
    assert _raw(vol, base, I16, H, W, -16.0, 5, 16.0, address(base)) == 0
    np.testing.assert_array_equal(base.reshape(H, W), want.image)
    for bad in (dict(max_speckle_size=-1), dict(max_diff=-1), dict(max_diff=np.nan), dict(max_diff=65536), dict(new_val=0.5)):
        with pytest.raises(ValueError):  # the binding refuses the same arguments before it calls
            vol.filter_speckles(image, **{**dict(max_speckle_size=5, max_diff=16), **bad})


# 13: stereo_sgm with the speckle arguments
@functools.lru_cache(maxsize=None)
def synthetic():
    rgb_left, rgb_right = sc.synthetic_pair(0)[:2]
    disp, depth = sr.stereo_sgm(rgb_left, rgb_right, num_disparities=32, bf=BF)
    return rgb_left, rgb_right, disp, depth, pr.filter_speckles(disp, 50, 16, depth=depth, method="union")


def test_stereo_sgm_filters_the_synthetic_pair(vol):
    rgb_left, rgb_right, disp, depth, want = synthetic()
    # the figures of the matcher's output on this pair: the case is not vacuous
    assert (want.stats["components"], want.stats["removed_components"], want.stats["removed_pixels"]) == (79, 75, 206)
    got = vol.stereo_sgm(rgb_left, rgb_right, num_disparities=32, bf=BF, speckle_window_size=50, speckle_range=1)
    np.testing.assert_array_equal(got[0], want.image)
    assert pr.same_bits(got[1], want.depth)
    assert (got[0] != disp).sum() == 206
    # the counts of the call itself
    out, stats = np.empty_like(disp), L.HvSpeckleStats()
    prm = L.HvStereoParams(32, 10, 120, 15, 1, 8, BF, 0.0, np.inf)
    L.check(vol._lib.hv_stereo_sgm_speckle(vol._h, L.ptr(rgb_left), L.ptr(rgb_right), disp.shape[0], disp.shape[1], 3, ctypes.byref(prm), 50, 1,
                                           L.ptr(out), None, ctypes.byref(stats), L.HV_HOST))
    np.testing.assert_array_equal(out, want.image)
    assert tuple(getattr(stats, k) for k in pr.STATS) == pr.stats_tuple(want.stats)
    # depth alone: the disparity is filtered in scratch of the handle
    only = np.empty_like(depth)
    L.check(vol._lib.hv_stereo_sgm_speckle(vol._h, L.ptr(rgb_left), L.ptr(rgb_right), disp.shape[0], disp.shape[1], 3, ctypes.byref(prm), 50, 1,
                                           None, L.ptr(only), None, L.HV_HOST))
    assert pr.same_bits(only, want.depth)
    for window, rng in ((0, 1), (-1, 1), ((1 << 30) + 1, 1), (50, -1), (50, 4096)):
        assert vol._lib.hv_stereo_sgm_speckle(vol._h, L.ptr(rgb_left), L.ptr(rgb_right), disp.shape[0], disp.shape[1], 3, ctypes.byref(prm),
                                              window, rng, L.ptr(out), None, None, L.HV_HOST) == -1
    np.testing.assert_array_equal(out, want.image)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("shape,paths", [((37, 83, 48), 4), ((19, 70, 128), 8)], ids=["37x83_D48_p4", "19x70_D128_p8"])
def test_stereo_sgm_speckle_at_other_shapes(vol, shape, paths, device):
    import torch

    assert shape in sc.SHAPES
    H, W, D = shape
    left, right = sc.textured_pair(H, W, 3, seed=H * 1000 + W + D)
    kw = dict(num_disparities=D, paths=paths, bf=BF, min_depth=0.5, max_depth=6.0)
    disp, depth = sr.stereo_sgm(left, right, **kw)
    # (the textured pairs' disparity is one region at a range of one pixel: range 0 cuts it into regions of equal disparity)
    want = pr.filter_speckles(disp, 3, 0, depth=depth, method="union")
    assert 0 < want.stats["removed_pixels"] < want.stats["valid_pixels"] and want.stats["largest"] > 3
    a, b = (torch.from_numpy(x).cuda() for x in (left, right)) if device else (left, right)
    got = vol.stereo_sgm(a, b, speckle_window_size=3, speckle_range=0, **kw)
    if device:
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got)
        got = tuple(t.cpu().numpy() for t in got)
    np.testing.assert_array_equal(got[0], want.image)
    assert pr.same_bits(got[1], want.depth)


def test_window_zero_is_the_plain_call(vol):
    rgb_left, rgb_right, disp, depth, _ = synthetic()
    kw = dict(num_disparities=32, bf=BF)

    def launches(**more):
        vol.profile_enable(True)
        try:
            out = vol.stereo_sgm(rgb_left, rgb_right, **kw, **more)
            return out, len(vol.profile_launches())
        finally:
            vol.profile_enable(False)

    plain, n_plain = launches()
    zero, n_zero = launches(speckle_window_size=0, speckle_range=3)
    filtered, n_filtered = launches(speckle_window_size=50)
    np.testing.assert_array_equal(plain[0], disp)
    np.testing.assert_array_equal(zero[0], plain[0])
    assert pr.same_bits(zero[1], plain[1]) and pr.same_bits(plain[1], depth)
    assert n_zero == n_plain > 0 and n_filtered > n_plain


# 14: through DepthEstimatorSgm to the TSDF, on the device
def test_filtered_stereo_depth_reaches_the_tsdf():
    import torch

    from pyslam_amd.depth_estimation import DepthEstimatorSgm
    from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume

    rgb_left, rgb_right, _, T_cw, s = sc.synthetic_pair(0)
    _, _, disp, depth, want = synthetic()
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    dev, host = (ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 12) for _ in range(2))
    try:
        est = DepthEstimatorSgm(dev, types.SimpleNamespace(bf=BF), num_disparities=32, speckle_window_size=50)
        got, _ = est.infer(rgb_left, rgb_right)
        assert isinstance(got, torch.Tensor) and got.is_cuda and est.disparity_map.is_cuda
        np.testing.assert_array_equal(est.disparity_map.cpu().numpy(), want.image)
        dev.integrate(RGBDImage.create_from_color_and_depth(torch.from_numpy(rgb_left).cuda(), got, depth_scale=1.0, depth_trunc=4.0, convert_rgb_to_intensity=False), K, T_cw)
        host.integrate(RGBDImage.create_from_color_and_depth(rgb_left, want.depth, depth_scale=1.0, depth_trunc=4.0, convert_rgb_to_intensity=False),
                       K, T_cw)
        for a, b in zip(dev.dump(), host.dump()):
            np.testing.assert_array_equal(a, b)
        assert dev.num_blocks() > 10
        # and the filter mattered: the unfiltered depth fuses another map
        assert not pr.same_bits(want.depth, depth)
    finally:
        dev.close()
        host.close()
