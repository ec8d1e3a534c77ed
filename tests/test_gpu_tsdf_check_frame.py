"""GPU: ScalableTSDFVolume.check_frame (hv_tsdf_check_frame, hv_sample.hip's image form: a wave per 8 x 8 pixel tile) held to the
numpy restatement (tests/sample_reference.py) on the volume's OWN dump(): sdf and class bit for bit off the fragile pixels, whose
share is capped at 1e-4 (tests/test_sample_reference_cpu.py asserts it is 0.0 for every frame used here), and the five counts equal
both to np.bincount of the library's own classes and to the restatement's.

Image sizes 1 x 1, 5 x 3, 8 x 8, 9 x 70 and 70 x 9 put partial tiles at the right edge, the bottom edge and both; depth float32 (scale
1) and uint16 (scale 5000); planted_states' exact-inverse poses and one generic rigid pose.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import sample_cases as sc
from tests import sample_reference as sr
from tests.test_gpu_tsdf_edges import intrinsic, tiny_frames, volume
from tests.test_gpu_tsdf_sample import FRAGILE_SHARE, bits, planted

pytestmark = pytest.mark.gpu

VOX, TRUNC = sc.VOX, sc.TRUNC


def camera(H, W):
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    return PinholeCameraIntrinsic(W, H, *sc.intrinsics(H, W))


@functools.lru_cache(maxsize=None)
def walls(pose):
    states, T = sc.wall_scene(pose)
    vol = planted(states)
    return vol, vol.dump(), T


def assert_equals_restatement(chk, ref, label):
    keep = ~ref["fragile"]
    assert ref["fragile"].mean() <= FRAGILE_SHARE, (label, ref["fragile"].mean())
    sdf, cls = np.asarray(chk.sdf), np.asarray(chk.cls)
    assert sdf.shape == ref["sdf"].shape and sdf.dtype == np.float32 and cls.shape == ref["cls"].shape and cls.dtype == np.uint8, label
    assert np.array_equal(cls[keep], ref["cls"][keep]), (label, int((cls != ref["cls"]).sum()))
    assert np.array_equal(bits(sdf[keep]), bits(ref["sdf"][keep])), label
    counts = (chk.invalid, chk.unknown, chk.consistent, chk.in_front, chk.behind)
    assert counts == tuple(np.bincount(cls.reshape(-1), minlength=5)), (label, counts)
    if keep.all():
        assert counts == tuple(ref["count"]), (label, counts, ref["count"])


@pytest.mark.parametrize("kind,scale", sc.DEPTH_KINDS, ids=[k for k, _ in sc.DEPTH_KINDS])
@pytest.mark.parametrize("H,W", sc.IMAGE_SIZES, ids=[f"{h}x{w}" for h, w in sc.IMAGE_SIZES])
@pytest.mark.parametrize("pose", list(sc.POSES))
def test_planted_walls(pose, H, W, kind, scale):
    vol, dump, T = walls(pose)
    depth = sc.wall_depth(H, W, kind, scale)
    chk = vol.check_frame(depth, camera(H, W), T, depth_scale=scale)
    assert isinstance(chk.sdf, np.ndarray) and isinstance(chk.cls, np.ndarray)
    ref = sr.check_frame(dump, VOX, TRUNC, depth, sc.intrinsics(H, W), T, scale)
    assert_equals_restatement(chk, ref, (pose, H, W, kind))
    assert not chk.sdf[chk.cls <= sr.UNKNOWN].any()
    # another tolerance and threshold move the classes as the restatement says
    chk = vol.check_frame(depth, camera(H, W), T, depth_scale=scale, weight_threshold=4.0, tolerance=0.01)
    assert_equals_restatement(chk, sr.check_frame(dump, VOX, TRUNC, depth, sc.intrinsics(H, W), T, scale, weight_threshold=4.0, tolerance=0.01),
                              (pose, H, W, kind, "threshold 4"))
    assert chk.consistent == chk.in_front == chk.behind == 0  # (every planted weight is 4)


def test_every_class_occurs_and_the_empty_map_knows_nothing():
    vol, dump, T = walls("generic")
    H, W = 70, 9
    depth = sc.wall_depth(H, W, "float32", 1.0)
    chk = vol.check_frame(depth, camera(H, W), T)
    assert min(chk.invalid, chk.unknown, chk.consistent, chk.in_front, chk.behind) > 0
    empty = volume(VOX, TRUNC).check_frame(depth, camera(H, W), T)
    assert empty.invalid == chk.invalid and empty.unknown == H * W - chk.invalid and not empty.sdf.any()
    assert np.array_equal(empty.cls == sr.INVALID, chk.cls == sr.INVALID)


def test_depth_edge_values():
    """0, NaN, +-inf and depth_min exactly are invalid, depth_max exactly is valid."""
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    vol, dump, T = walls("+z")
    depth = np.array([[0.0, np.nan, np.inf, 0.25, 0.5, -np.inf, np.nextafter(np.float32(0.25), np.float32(1)), np.nextafter(np.float32(0.5), np.float32(1))]],
                     np.float32)
    intr = (40.0, 40.0, 3.5, 0.0)
    chk = vol.check_frame(depth, PinholeCameraIntrinsic(8, 1, *intr), T, depth_min=0.25, depth_max=0.5)
    assert (chk.cls[0] == sr.INVALID).tolist() == [True, True, True, True, False, True, False, True]
    assert chk.cls[0, 4] == sr.CONSISTENT
    assert_equals_restatement(chk, sr.check_frame(dump, VOX, TRUNC, depth, intr, T, 1.0, 0.25, 0.5), "edge values")
    # uint16: 0 is invalid, depth_min and depth_max in raw units behave the same
    raw = np.array([[0, 1250, 1251, 2500, 2501, 65535]], np.uint16)
    chk = vol.check_frame(raw, PinholeCameraIntrinsic(6, 1, 40.0, 40.0, 2.5, 0.0), T, depth_scale=5000.0, depth_min=0.25, depth_max=0.5)
    assert (chk.cls[0] == sr.INVALID).tolist() == [True, True, False, False, True, True]
    assert_equals_restatement(chk, sr.check_frame(dump, VOX, TRUNC, raw, (40.0, 40.0, 2.5, 0.0), T, 5000.0, 0.25, 0.5), "edge values u16")


@functools.lru_cache(maxsize=None)
def fused():
    s, frames = tiny_frames(0, sc.FUSED_FRAMES)
    vol = volume(VOX, TRUNC)
    for d, c, T in frames:
        vol.integrate_batch(d[None], c[None], intrinsic(s), T[None], 1.0, 4.0)
    return s, frames, vol, vol.dump()


def test_fused_scene_tells_the_pulled_rectangle_apart():
    s, frames, vol, dump = fused()
    depth, _, T = frames[sc.FUSED_FRAME]
    K = intrinsic(s)
    moved = sc.pulled(depth)
    chk = vol.check_frame(moved, K, T, depth_max=4.0)
    assert_equals_restatement(chk, sr.check_frame(dump, VOX, TRUNC, moved, K.as_array(), T, 1.0, 0.1, 4.0), "pulled")
    rect = chk.cls[sc.PULL_RECT]
    valid = int((rect != sr.INVALID).sum())
    print(f"pulled rectangle: {valid} valid pixels, classes {np.bincount(rect.reshape(-1), minlength=5).tolist()}")
    assert valid > 1000 and (rect == sr.CONSISTENT).sum() == 0 and (rect == sr.IN_FRONT).sum() >= valid / 2
    # the frame as it was fused agrees with the map
    same = vol.check_frame(depth, K, T, depth_max=4.0)
    assert same.consistent > 0.95 * (same.consistent + same.unknown + same.in_front + same.behind)
    # the dynamic-pixel mask: zero what floats in seen-free space, and nothing of it is left
    moved[chk.cls == sr.IN_FRONT] = 0
    again = vol.check_frame(moved, K, T, depth_max=4.0)
    assert again.in_front == 0 and again.invalid == chk.invalid + chk.in_front


def test_without_stats_the_call_is_queued_and_gives_the_same_values():
    import torch

    from pyslam_amd import _lib as L

    vol, dump, T = walls("generic")
    H, W = 70, 9
    depth = sc.wall_depth(H, W, "uint16", 5000.0)
    want = vol.check_frame(depth, camera(H, W), T, depth_scale=5000.0)
    prm = L.HvCheckParams()
    prm.depth_scale, prm.depth_min, prm.depth_max, prm.weight_threshold, prm.tolerance = 5000.0, 0.1, 3.0, 0.0, 0.5 * TRUNC
    d = torch.from_numpy(depth).cuda()
    sdf = torch.full((H, W), 7.5, dtype=torch.float32, device="cuda")
    cls = torch.full((H, W), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    intr, Tc = np.array(sc.intrinsics(H, W)), np.ascontiguousarray(T)
    L.check(vol._lib.hv_tsdf_check_frame(vol._h, L.ptr(d), L.HV_DEPTH_U16, H, W, L.ptr(intr), L.ptr(Tc), ctypes.byref(prm), L.ptr(sdf), L.ptr(cls),
                                         None, L.HV_DEVICE))
    vol.synchronize()
    assert np.array_equal(bits(sdf.cpu().numpy()), bits(want.sdf)) and np.array_equal(cls.cpu().numpy(), want.cls)
    # torch CUDA in, torch CUDA out through the method; only the counts when no array is asked for
    dev = vol.check_frame(d, camera(H, W), T, depth_scale=5000.0)
    assert dev.sdf.is_cuda and dev.cls.is_cuda and dev.stats == want.stats
    assert np.array_equal(bits(dev.sdf.cpu().numpy()), bits(want.sdf)) and np.array_equal(dev.cls.cpu().numpy(), want.cls)
    st = L.HvCheckStats()
    L.check(vol._lib.hv_tsdf_check_frame(vol._h, L.ptr(depth), L.HV_DEPTH_U16, H, W, L.ptr(intr), L.ptr(Tc), ctypes.byref(prm), None, None,
                                         ctypes.byref(st), L.HV_HOST))
    assert tuple(st.count) == want.stats.as_tuple()


def test_errors():
    from pyslam_amd import _lib as L
    from pyslam_amd.volumetric import ScalableTSDFVolume, VoxelBlockGrid

    vol, dump, T = walls("+z")
    H, W = 8, 8
    depth, K = sc.wall_depth(H, W, "float32", 1.0), camera(H, W)
    grid = VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12)
    with pytest.raises(L.HipVolError, match="TSDF"):
        ScalableTSDFVolume.check_frame(grid, depth, K, T, tolerance=0.04)
    owner = volume(VOX, TRUNC)
    owner.set_owner(0, 2)
    with pytest.raises(L.HipVolError, match="owner-sharded"):
        owner.check_frame(depth, K, T)
    tiled = volume(VOX, TRUNC)
    tiled.set_tile(0, 0, 4, 8)
    with pytest.raises(L.HipVolError, match="tile-sharded"):
        tiled.check_frame(depth, K, T)
    for kw, match in (({"tolerance": 0.0}, "tolerance"), ({"tolerance": -0.01}, "tolerance"), ({"tolerance": float("inf")}, "tolerance"),
                      ({"weight_threshold": -1.0}, "weight_threshold"), ({"depth_min": 1.0, "depth_max": 1.0}, "depth range"),
                      ({"depth_min": -0.1}, "depth range"), ({"depth_scale": 0.0}, "scale")):
        with pytest.raises(L.HipVolError, match=match):
            vol.check_frame(depth, K, T, **kw)
    sheared = T.copy()
    sheared[0, 1] += 0.01
    with pytest.raises(L.HipVolError, match="not rigid"):
        vol.check_frame(depth, K, sheared)
    mirrored = T.copy()
    mirrored[0, :3] *= -1.0
    with pytest.raises(L.HipVolError, match="not rigid"):
        vol.check_frame(depth, K, mirrored)
    with pytest.raises(RuntimeError):
        vol.check_frame(depth, K, np.eye(3))
    with pytest.raises(RuntimeError):
        vol.check_frame(depth[:, :7], K, T)  # the image is not the intrinsic's size
    with pytest.raises(RuntimeError):
        vol.check_frame(depth.astype(np.complex64), K, T)
