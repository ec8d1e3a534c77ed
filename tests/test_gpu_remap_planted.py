"""GPU: pyslam_amd/csrc/hv_prep.hip - k_remap_nearest<u8|f32|i32>, k_remap_linear_u8, k_remap_linear_f32 and the batched
k_rectify_frames<u16|f32> - on the planted maps and images of tests/remap_cases.py, against the restatement of
tests/remap_reference.py (tests/test_remap_reference_cpu.py proves that these cases tell every named wrong reading apart).

Bars: nearest and linear uint8 bit for bit; linear float32 bit for bit on the exact images (integers below 2^13: no float32
operation rounds) and within GAMMA4 * sum w|p| elsewhere (derived: four products, three additions); NaN / inf pixels as IEEE has
them.  The batched kernel is seen through fusion: a volume with rectify maps against a volume without, fed the frames the restatement
rectified - both run the same kernels after the rectify step, so dump() must agree bit for bit.
"""
import numpy as np
import pytest

from tests import remap_cases as rc
from tests import remap_reference as rr
from tests.test_gpu_tsdf_edges import odd_config

pytestmark = pytest.mark.gpu

VOX, TRUNC = 0.02, 0.08
HV_ERR_INVALID, HV_ERR_MODE = -1, -4
KIND = {np.dtype(np.uint8): 0, np.dtype(np.float32): 1, np.dtype(np.int32): 2}

# (operation, image kind, channels): every kernel at every channel count
NEAREST = [("nearest", k, C) for k in ("u8", "f32_special", "i32") for C in (1, 2, 3, 4)]
LINEAR_U8 = [("linear", "u8", C) for C in (1, 2, 3, 4)] + [("linear", "u8_white", 3)]
LINEAR_F32 = [("linear", k, C) for k in ("f32_exact", "f32_random") for C in (1, 2, 3, 4)] + [("linear", "f32_special", 1), ("linear", "f32_special", 3)]
_REF = {}


def reference(c, op, kind, C):
    """-> (expected, bound or None), computed once per (case, operation, image) for the module."""
    key = (c.name, op, kind, C)
    if key not in _REF:
        img = rc.image(kind, c.H, c.W, C)
        if op == "nearest":
            _REF[key] = (rr.remap_nearest(img, c.map_x, c.map_y), None)
        elif img.dtype == np.uint8:
            _REF[key] = (rr.remap_linear_u8(img, c.map_x, c.map_y), None)
        else:
            _REF[key] = rr.remap_linear_f32(img, c.map_x, c.map_y)
    return _REF[key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check(got, c, op, kind, C, what):
    want, bound = reference(c, op, kind, C)
    img = rc.image(kind, c.H, c.W, C)
    msg = f"{what}: {c.name} {op} {kind} C={C}"
    assert got.shape == img.shape and got.dtype == img.dtype, msg
    if op == "nearest":
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=msg)  # copied, never converted: NaN payloads and -0.0 too
    elif bound is None:
        np.testing.assert_array_equal(got, want, err_msg=msg)
    elif kind == "f32_exact":
        assert rr.is_exact_image(img)
        np.testing.assert_array_equal(got.astype(np.float64), want, err_msg=msg)
    elif kind == "f32_special":
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=msg)
        fin = np.isfinite(want)
        np.testing.assert_array_equal(got[~fin], want[~fin].astype(np.float32), err_msg=msg)
        assert (np.abs(got[fin].astype(np.float64) - want[fin]) <= bound[fin]).all(), msg
    else:
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), f"{msg}: error {err.max()}, bound there {bound.ravel()[err.argmax()]}"


def tsdf_volume(**kw):
    from pyslam_amd.volumetric import ScalableTSDFVolume

    return ScalableTSDFVolume(VOX, TRUNC, max_blocks=1 << 10, **kw)


def grid_volume():
    from pyslam_amd.volumetric import VoxelBlockGrid

    return VoxelBlockGrid(VOX, 8, max_blocks=1 << 8, max_points=1 << 12)


def cuda(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


@pytest.fixture(scope="module", params=["grid", "tsdf"])
def vol(request):
    return grid_volume() if request.param == "grid" else tsdf_volume()


# ---- 1. single-image remap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("ops", [NEAREST, LINEAR_U8, LINEAR_F32], ids=["nearest", "linear_u8", "linear_f32"])
def test_every_kernel_on_every_planted_map(vol, ops, form):
    n = 0
    for c in rc.maps():
        maps = (c.map_x, c.map_y) if form == "host" else (cuda(c.map_x), cuda(c.map_y))
        for op, kind, C in ops:
            img = rc.image(kind, c.H, c.W, C)
            got = vol.remap(img if form == "host" else cuda(img), *maps, linear=op == "linear")
            check(got if form == "host" else got.cpu().numpy(), c, op, kind, C, form)
            n += 1
    assert n == len(rc.maps()) * len(ops)  # no case is skipped


# ---- 2. the device form depends on this call's arguments alone -------------------------------------------------------------------
def test_fresh_maps_in_a_loop_are_the_maps_that_are_used():
    """Map arrays built per call: the old ones are freed, so their ids come back.  Nothing may be remembered under them."""
    vol = grid_volume()
    for rnd in range(2):
        for c in rc.maps():
            mx, my = np.array(c.map_x), np.array(c.map_y)  # fresh host arrays
            got = vol.remap(cuda(rc.image("u8", c.H, c.W, 3)), mx, my, linear=True)
            check(got.cpu().numpy(), c, "linear", "u8", 3, f"fresh maps, round {rnd}")
            del mx, my


@pytest.mark.parametrize("maps_on", ["host", "device"])
def test_a_map_changed_in_place_is_read_again(maps_on):
    vol = tsdf_volume()
    a, b = rc.case("permutation_5x7"), rc.case("border_5x7")
    img = cuda(rc.image("i32", 5, 7, 2))
    col = cuda(rc.image("u8", 5, 7, 3))
    mx, my = (np.array(a.map_x), np.array(a.map_y)) if maps_on == "host" else (cuda(a.map_x), cuda(a.map_y))
    check(vol.remap(img, mx, my).cpu().numpy(), a, "nearest", "i32", 2, "before the change")
    check(vol.remap(img, mx, my).cpu().numpy(), a, "nearest", "i32", 2, "the same arrays again")
    if maps_on == "host":
        mx[...], my[...] = b.map_x, b.map_y
    else:
        mx.copy_(cuda(b.map_x)), my.copy_(cuda(b.map_y))
    check(vol.remap(img, mx, my).cpu().numpy(), b, "nearest", "i32", 2, "changed in place")
    check(vol.remap(col, mx, my, linear=True).cpu().numpy(), b, "linear", "u8", 3, "changed in place")
    check(vol.remap(img, mx, my).cpu().numpy(), b, "nearest", "i32", 2, "unchanged since")


def test_device_images_refuse_maps_of_another_shape():
    vol = grid_volume()
    c = rc.case("identity_5x7")
    img = cuda(rc.image("u8", 5, 7, 3))
    for mx, my in ((c.map_x[:4], c.map_y), (c.map_x, cuda(c.map_y.T)), (cuda(c.map_x.ravel()), cuda(c.map_y.ravel()))):
        with pytest.raises(RuntimeError, match="the image is 5x7"):
            vol.remap(img, mx, my, linear=True)
    check(vol.remap(img, c.map_x, c.map_y, linear=True).cpu().numpy(), c, "linear", "u8", 3, "after the refusals")


def test_rectify_maps_object_keeps_one_device_copy():
    """prep.RectifyMaps (what Undistorter and the integrators hold): host maps for host images, one device pair per device for
    device images - the same tensors on every call, no upload per frame."""
    from pyslam_amd.prep import RectifyMaps

    vol = grid_volume()
    c = rc.case("border_17x31")
    maps = RectifyMaps(c.map_x, c.map_y)
    img = rc.image("u8", 17, 31, 3)
    assert maps.for_image(img)[0] is maps.map_x
    first = maps.for_image(cuda(img))
    assert first[0].is_cuda and all(x is y for x, y in zip(first, maps.for_image(cuda(img))))
    check(vol.remap(cuda(img), *maps.for_image(cuda(img)), linear=True).cpu().numpy(), c, "linear", "u8", 3, "RectifyMaps, device")
    check(vol.remap(img, *maps.for_image(img), linear=True), c, "linear", "u8", 3, "RectifyMaps, host")
    with pytest.raises(ValueError):
        maps.map_x[0, 0] = 1.0  # the host maps cannot drift away from the device copy


# ---- 3. the batched kernel, observed through fusion ------------------------------------------------------------------------------
CAMERAS = {"7x5": (7, 5), "31x17": (31, 17)}
ENTRIES = ("integrate", "integrate_batch_host", "integrate_batch_device", "integrate_frames", "deintegrate_batch", "reintegrate_batch")


def camera(W, H):
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    cfg = odd_config(W, H, VOX)
    return PinholeCameraIntrinsic(W, H, cfg["fx"], cfg["fy"], cfg["cx"], cfg["cy"])


def poses(B):
    T = np.tile(np.eye(4), (B, 1, 1))
    T[:, 0, 3] = 0.013 * np.arange(B)
    T[:, 1, 3] = -0.007 * np.arange(B)
    return T


def fuse(v, entry, d, c, K, T, scale):
    from pyslam_amd.volumetric import RGBDImage

    B = len(d)
    if entry == "integrate":
        for f in range(B):
            v.integrate(RGBDImage(c[f], d[f], scale, 4.0), K, T[f])
    elif entry == "integrate_batch_device":
        v.integrate_batch(cuda(d), cuda(c), K, T, depth_scale=scale)
    elif entry == "integrate_frames":
        v.integrate_frames([np.array(x) for x in d], [np.array(x) for x in c], K, T, depth_scale=scale)
    else:
        v.integrate_batch(d, c, K, T, depth_scale=scale)
        if entry == "deintegrate_batch":
            n = (B + 1) // 2
            return v.deintegrate_batch(d[:n], c[:n], K, T[:n], depth_scale=scale)
        if entry == "reintegrate_batch":  # old pose == new pose: out and in again, the map as it was
            return v.reintegrate_batch(d, c, K, T, T, depth_scale=scale)
    return None


def assert_same_dump(a, b, msg):
    assert len(a[0]) == len(b[0]) and len(a[0]) > 0, msg
    for x, y, name in zip(a, b, ("keys", "tsdf", "weight", "colour")):
        np.testing.assert_array_equal(bits(x), bits(y), err_msg=f"{msg}: {name}")


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("cam", list(CAMERAS))
def test_rectified_fusion_equals_fusion_of_rectified_frames(cam, u16):
    W, H = CAMERAS[cam]
    K = camera(W, H)
    scale = 40000.0 if u16 else 1.0
    vol, twin = tsdf_volume(depth_sampling_stride=1), tsdf_volume(depth_sampling_stride=1)
    for name, (mx, my) in rc.camera_maps(H, W).items():
        vol.set_rectify_maps(mx, my)
        for B in (1, 2, 5):
            d, c = rc.batch(B, H, W, u16)
            dr, cr = rr.rectify_frames(d, c, mx, my)
            if name == "nonfinite":
                bad = ~(np.isfinite(mx) & np.isfinite(my)) | (np.abs(mx) > 1e9) | (np.abs(my) > 1e9)
                assert bad.any() and not dr[:, bad].any() and not cr[:, bad].any() and dr[:, ~bad].all()
            T = poses(B)
            for entry in ENTRIES:
                vol.reset(), twin.reset()
                st, st2 = fuse(vol, entry, d, c, K, T, scale), fuse(twin, entry, dr, cr, K, T, scale)
                assert st == st2
                assert_same_dump(vol.dump(), twin.dump(), f"{cam} {'u16' if u16 else 'f32'} {name} B={B} {entry}")


@pytest.mark.parametrize("name", ["half_pixel", "border"])
def test_one_fused_frame_shows_the_blended_pixels(name):
    """One frame: a voxel of weight 1 holds exactly the colour of the rectified pixel it projects to.  Among them are colours that
    only a blended pixel has, and (border) colours that only a pixel blended with the border has."""
    from pyslam_amd.volumetric import RGBDImage

    W, H = CAMERAS["31x17"]
    mx, my = rc.camera_maps(H, W)[name]
    d, c = rc.batch(1, H, W, False)
    dr, cr = rr.rectify_frames(d, c, mx, my)
    iy, ix, fy, fx, ok = rr.linear_taps(mx, my)
    blended = ((fx > 0) | (fy > 0)).reshape(H, W)
    outside = np.zeros(H * W, bool)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        out = ~((ix + dx >= 0) & (ix + dx < W) & (iy + dy >= 0) & (iy + dy < H))
        outside |= out & ((fx if dx else 32 - fx) * (fy if dy else 32 - fy) > 0)
    outside = outside.reshape(H, W)
    seen = dr[0] > 0
    colours = lambda mask: {tuple(int(v) for v in p) for p in cr[0][mask & seen]}
    vol = tsdf_volume(depth_sampling_stride=1)
    vol.set_rectify_maps(mx, my)
    vol.integrate(RGBDImage(np.array(c[0]), np.array(d[0]), 1.0, 4.0), camera(W, H), np.eye(4))
    keys, tsdf, weight, colour = vol.dump()
    assert len(keys) > 0 and set(np.unique(weight)) <= {0.0, 1.0}
    fused = {tuple(int(v) for v in p) for p in colour[weight == 1.0]}
    assert (colour[weight == 1.0] == np.rint(colour[weight == 1.0])).all()
    assert fused <= colours(np.ones((H, W), bool))
    assert fused & (colours(blended) - colours(~blended)), "no fused colour comes from a blended pixel"
    if name == "border":
        assert outside.any() and (fused & (colours(outside) - colours(~outside))), "no fused colour comes from a border-blended pixel"


# ---- 4. map handling -------------------------------------------------------------------------------------------------------------
def rectified_twin(d, c, mx, my, K, T, scale=1.0):
    twin = tsdf_volume(depth_sampling_stride=1)
    dr, cr = rr.rectify_frames(d, c, mx, my) if mx is not None else (d, c)
    twin.integrate_batch(dr, cr, K, T, depth_scale=scale)
    return twin.dump()


def test_maps_replaced_by_smaller_larger_device_and_cleared():
    from pyslam_amd import _lib as L

    vol = tsdf_volume(depth_sampling_stride=1)
    T = poses(2)
    for (W, H), name, where in (((7, 5), "border", "host"), ((5, 4), "permutation", "host"), ((31, 17), "half_pixel", "host"),
                                ((7, 5), "nonfinite", "device"), ((31, 17), "border", "device"), ((7, 5), "permutation", "host")):
        mx, my = rc.camera_maps(H, W)[name]
        if where == "host":
            vol.set_rectify_maps(mx, my)
        else:
            dx, dy = cuda(mx), cuda(my)
            L.check(vol._lib.hv_tsdf_set_rectify_maps(vol._h, L.ptr(dx), L.ptr(dy), H, W, L.HV_DEVICE))
            dx.zero_(), dy.zero_()  # copied: the volume keeps nothing of the caller's
        d, c = rc.batch(2, H, W, False)
        vol.reset()
        vol.integrate_batch(d, c, camera(W, H), T)
        assert_same_dump(vol.dump(), rectified_twin(d, c, mx, my, camera(W, H), T), f"{W}x{H} {name} maps from the {where}")
    vol.set_rectify_maps(None, None)  # cleared: frames are fused as they come, of any size
    for W, H in ((7, 5), (31, 17)):
        d, c = rc.batch(2, H, W, True)
        vol.reset()
        vol.integrate_batch(cuda(d), cuda(c), camera(W, H), T, depth_scale=40000.0)
        assert_same_dump(vol.dump(), rectified_twin(d, c, None, None, camera(W, H), T, 40000.0), f"{W}x{H} maps cleared")


def test_frames_of_another_size_than_the_maps_are_refused():
    from pyslam_amd import _lib as L
    from pyslam_amd._lib import HipVolError
    from pyslam_amd.volumetric import RGBDImage

    vol = tsdf_volume(depth_sampling_stride=1)
    mx, my = rc.camera_maps(5, 7)["border"]
    vol.set_rectify_maps(mx, my)
    T = poses(2)
    d, c = rc.batch(2, 5, 7, False)
    vol.integrate_batch(d, c, camera(7, 5), T)
    before = vol.dump()
    for W, H in ((5, 7), (7, 4), (31, 17)):
        d2, c2 = (np.array(a) for a in rc.batch(2, H, W, False))
        K = camera(W, H)
        for call in (lambda: vol.integrate(RGBDImage(c2[0], d2[0], 1.0, 4.0), K, T[0]), lambda: vol.integrate_batch(d2, c2, K, T),
                     lambda: vol.integrate_batch(cuda(d2), cuda(c2), K, T), lambda: vol.integrate_frames(list(d2), list(c2), K, T),
                     lambda: vol.deintegrate_batch(d2, c2, K, T), lambda: vol.reintegrate_batch(d2, c2, K, T, T)):
            with pytest.raises(HipVolError, match="rectify maps"):
                call()
        intr, T0 = K.as_array(), np.ascontiguousarray(T[0])
        rc_ = vol._lib.hv_tsdf_integrate(vol._h, L.ptr(d2[0]), L.HV_DEPTH_F32, L.ptr(c2[0]), H, W, L.ptr(intr), L.ptr(T0), 1.0, 4.0, L.HV_HOST)
        assert rc_ == HV_ERR_INVALID
        vol.synchronize()
        assert_same_dump(vol.dump(), before, f"after refused {W}x{H} frames")
    vol.integrate_batch(d, c, camera(7, 5), T)  # and the maps still stand
    twin = tsdf_volume(depth_sampling_stride=1)
    dr, cr = rr.rectify_frames(d, c, mx, my)
    for _ in range(2):
        twin.integrate_batch(dr, cr, camera(7, 5), T)
    assert_same_dump(vol.dump(), twin.dump(), "a good batch after the refusals")


def test_a_block_grid_has_no_rectify_maps():
    from pyslam_amd import _lib as L

    grid = grid_volume()
    mx, my = rc.camera_maps(5, 7)["border"]
    assert grid._lib.hv_tsdf_set_rectify_maps(grid._h, L.ptr(mx), L.ptr(my), 5, 7, L.HV_HOST) == HV_ERR_MODE
    assert grid._lib.hv_tsdf_set_rectify_maps(grid._h, None, None, 0, 0, L.HV_HOST) == HV_ERR_MODE
    c = rc.case("border_5x7")
    check(grid.remap(rc.image("u8", 5, 7, 3), c.map_x, c.map_y, linear=True), c, "linear", "u8", 3, "the grid still remaps")


# ---- 5. hv_remap's refusals through the C ABI ------------------------------------------------------------------------------------
def test_hv_remap_refusals_leave_the_next_call_correct(vol):
    from pyslam_amd import _lib as L

    c = rc.case("border_5x7")
    H, W = 5, 7
    u8, i32 = rc.image("u8", H, W, 3), rc.image("i32", H, W, 1)
    out_u8, out_i32 = np.full_like(u8, 7), np.full_like(i32, 7)
    p = L.ptr

    def call(src, kind, C, h, w, mx, my, linear, dst):
        return vol._lib.hv_remap(vol._h, src, kind, C, h, w, mx, my, linear, dst, L.HV_HOST)

    good = (p(u8), 0, 3, H, W, p(c.map_x), p(c.map_y), 1, p(out_u8))
    refusals = {"channels 0": {2: 0}, "channels 5": {2: 5}, "height 0": {3: 0}, "width 0": {4: 0}, "height -1": {3: -1}, "width -7": {4: -7},
                "kind 3": {1: 3}, "kind -1": {1: -1}, "null src": {0: None}, "null map_x": {5: None}, "null map_y": {6: None}, "null dst": {8: None}}
    for what, change in refusals.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert call(*args) == HV_ERR_INVALID, what
        assert (out_u8 == 7).all(), what
        assert call(*good) == 0, what
        np.testing.assert_array_equal(out_u8, reference(c, "linear", "u8", 3)[0], err_msg=f"after {what}")
        out_u8[...] = 7
    assert call(p(i32), 2, 1, H, W, p(c.map_x), p(c.map_y), 1, p(out_i32)) == HV_ERR_INVALID  # labels are not interpolated
    assert (out_i32 == 7).all()
    assert call(p(i32), 2, 1, H, W, p(c.map_x), p(c.map_y), 0, p(out_i32)) == 0
    np.testing.assert_array_equal(out_i32, reference(c, "nearest", "i32", 1)[0])
    assert vol._lib.hv_remap(None, *good, L.HV_HOST) == HV_ERR_INVALID
    assert b"null argument" in vol._lib.hv_last_error()
