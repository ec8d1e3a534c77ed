"""GPU: the TSDF kernels against oracle.PortTsdf at the inputs the other parity tests never feed them - image shapes that are not
multiples of 8 (scalar pack fallback, partial touch patches, partial ray-cast tiles), depth sampling strides other than 4, calls
split into several 64-frame sweeps, shape and intrinsics changes inside a running batch chain, NaN / inf / subnormal / truncation
edge depth values, a world far from the origin, and operands in the wrong layout.

Bars (the suite's own, tests/test_gpu_tsdf.py): unit keys, touched sets and weights exact; tsdf bitwise on the online path and under
HV_TSDF_SWEEP=2, within FOLD_TSDF_TOL on the fold form; colour within 1e-4.  Cameras are tiny_160x120_2cm's scaled to the shape,
with the principal point off centre (0.37 W, 0.61 H) and fx != fy, so that the image borders in u and v differ.
"""
import functools

import numpy as np
import pytest

import oracle
from tests.conftest import assert_dumps_match, canonical_mesh, sort_rows
from tests.test_gpu_tsdf import TOL, assert_same_volume

pytestmark = pytest.mark.gpu

SWEEP_FORMS = ("4", "2")  # fold (production), bitwise


def odd_config(W, H, voxel=0.02):
    """tiny_160x120_2cm's camera scaled to W x H (same angular resolution on the larger side), principal point off centre."""
    scale = max(W / 160.0, H / 120.0)
    return dict(width=W, height=H, fx=131.25 * scale * 1.04, fy=131.25 * scale * 0.97, cx=0.37 * W, cy=0.61 * H, voxel=voxel)


@functools.lru_cache(maxsize=None)
def _frames_cached(key, start, count, depth_dtype, depth_map_factor):
    from pyslam_amd.synthetic import SyntheticRGBD

    cfg = dict(key) if isinstance(key, tuple) else key
    s = SyntheticRGBD(cfg, depth_dtype=depth_dtype, depth_map_factor=depth_map_factor)
    return s, s.frames(start, count, workers=1)


def frames_of(cfg, start, count, depth_dtype="float32", depth_map_factor=5000.0):
    key = tuple(sorted(cfg.items())) if isinstance(cfg, dict) else cfg
    s, fr = _frames_cached(key, start, count, depth_dtype, depth_map_factor)
    return s, [(d.copy(), c.copy(), T.copy()) for d, c, T in fr]


def tiny_frames(start, count):
    """tiny_160x120_2cm frames, rendered once for the module."""
    s, frames = frames_of("tiny_160x120_2cm", 0, 200)
    return s, frames[start:start + count]


def intrinsic(s):
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    return PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)


def volume(voxel, trunc, **kw):
    from pyslam_amd.volumetric import ScalableTSDFVolume

    return ScalableTSDFVolume(voxel, trunc, max_blocks=1 << 12, **kw)


def stack(frames):
    return tuple(np.stack([f[k] for f in frames]) for k in range(3))


def cuda(*arrays):
    import torch

    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def oracle_of(s, frames, voxel, trunc, depth_scale=1.0, depth_trunc=4.0, stride=4, cpu=None):
    cpu = cpu or oracle.PortTsdf(voxel, trunc, depth_sampling_stride=stride, threads=8)
    K = intrinsic(s).as_array()
    for d, c, T in frames:
        cpu.integrate(d, c, K, T, depth_scale, depth_trunc)
    return cpu


def assert_meshes_match(gpu, cpu):
    m = gpu.extract_triangle_mesh()
    vb, tb, cb = cpu.extract_triangle_mesh()
    assert m.vertices.shape == vb.shape and m.triangles.shape == tb.shape
    va, ca, ta = canonical_mesh(m.vertices, m.triangles, m.vertex_colors)
    vb, cb, tb = canonical_mesh(vb, tb, cb)
    np.testing.assert_allclose(va, vb, rtol=0, atol=1e-9)
    np.testing.assert_allclose(ca, cb, rtol=0, atol=TOL)
    np.testing.assert_allclose(ta, tb, rtol=0, atol=1e-9)
    pc = gpu.extract_point_cloud()
    pb, qb = cpu.extract_point_cloud()
    assert pc.points.shape == pb.shape
    pa, qa = sort_rows(np.round(pc.points, 9), pc.colors)
    pb, qb = sort_rows(np.round(pb, 9), qb)
    np.testing.assert_allclose(pa, pb, rtol=0, atol=1e-9)
    np.testing.assert_allclose(qa, qb, rtol=0, atol=TOL)
    return len(m.triangles)


def check_every_entry_point(monkeypatch, s, frames, voxel, trunc, depth_scale=1.0, depth_trunc=4.0, stride=4, mesh=False):
    """The same frames through integrate (touched keys per frame), integrate_batch on device tensors (both sweep forms) and on host
    arrays, and integrate_frames: every volume equal to the oracle's.  -> (oracle, online volume)."""
    from pyslam_amd.volumetric import RGBDImage

    K = intrinsic(s)
    cpu = oracle.PortTsdf(voxel, trunc, depth_sampling_stride=stride, threads=8)
    online = volume(voxel, trunc, depth_sampling_stride=stride)
    for d, c, T in frames:
        online.integrate(RGBDImage(c, d, depth_scale, depth_trunc), K, T)
        cpu.integrate(d, c, K.as_array(), T, depth_scale, depth_trunc)
        np.testing.assert_array_equal(online.touched_keys(), cpu.touched_keys())
    assert cpu.num_units() > 0
    assert_same_volume(online, cpu)
    d, c, T = stack(frames)
    for form in SWEEP_FORMS:
        monkeypatch.setenv("HV_TSDF_SWEEP", form)
        dev = volume(voxel, trunc, depth_sampling_stride=stride)
        dev.integrate_batch(*cuda(d, c), K, T, depth_scale=depth_scale, depth_trunc=depth_trunc)
        assert_same_volume(dev, cpu, swept=True)
    monkeypatch.delenv("HV_TSDF_SWEEP", raising=False)
    host = volume(voxel, trunc, depth_sampling_stride=stride)
    host.integrate_batch(d, c, K, T, depth_scale=depth_scale, depth_trunc=depth_trunc)
    assert_same_volume(host, cpu, swept=True)
    staged = volume(voxel, trunc, depth_sampling_stride=stride)
    staged.integrate_frames([f[0] for f in frames], [f[1] for f in frames], K, T, depth_scale=depth_scale, depth_trunc=depth_trunc)
    for x, y in zip(staged.dump(), host.dump()):
        np.testing.assert_array_equal(x, y)
    if mesh:
        assert_meshes_match(online, cpu)
    return cpu, online


# ---- 1. shape x entry point matrix ---------------------------------------------------------------------------------------
SHAPES = [(161, 119, 0.02), (162, 118, 0.02), (7, 5, 0.02), (1, 240, 0.02), (320, 1, 0.02), (641, 479, 0.01)]


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("W,H,voxel", SHAPES, ids=[f"{w}x{h}" for w, h, _ in SHAPES])
def test_odd_shapes_match_the_oracle_on_every_entry_point(W, H, voxel, u16, monkeypatch):
    """H*W odd (the pack role's scalar fallback), W % 8 != 0 (partial touch patches), images smaller than one patch, a single
    column / row, and many partial patches at 641x479."""
    s, frames = frames_of(odd_config(W, H, voxel), 3, 4, "uint16" if u16 else "float32")
    cpu, online = check_every_entry_point(monkeypatch, s, frames, voxel, 0.08, depth_scale=5000.0 if u16 else 1.0, mesh=not u16)
    if W * H >= 1000:
        assert cpu.num_units() > 20


# ---- 2. depth sampling stride --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box_bits", [None, "0"], ids=["box_default", "box_0"])
@pytest.mark.parametrize("stride", [1, 2, 3, 5, 8])
def test_depth_sampling_stride_opens_the_oracles_units(stride, box_bits, monkeypatch):
    """ScalableTSDFVolume(depth_sampling_stride=s) against PortTsdf(depth_sampling_stride=s): online (touched keys per frame) then
    a multi-frame batch into the same volume, with the touch pass's bitmap path and (HV_TSDF_TOUCH_BOX_BITS=0) its general path,
    including a truncation band wider than a unit."""
    from pyslam_amd.volumetric import RGBDImage

    if box_bits is not None:
        monkeypatch.setenv("HV_TSDF_TOUCH_BOX_BITS", box_bits)  # (read at volume creation)
    for W, H in ((161, 119), (640, 480)):
        s, frames = frames_of(odd_config(W, H), 2, 4)
        K = intrinsic(s)
        for voxel, trunc in ((0.02, 0.08), (0.01, 0.2)):
            gpu = volume(voxel, trunc, depth_sampling_stride=stride)
            cpu = oracle.PortTsdf(voxel, trunc, depth_sampling_stride=stride, threads=8)
            for d, c, T in frames[:2]:
                gpu.integrate(RGBDImage(c, d, 1.0, 4.0), K, T)
                cpu.integrate(d, c, K.as_array(), T, 1.0, 4.0)
                np.testing.assert_array_equal(gpu.touched_keys(), cpu.touched_keys())
            d, c, T = stack(frames[2:])
            gpu.integrate_batch(*cuda(d, c), K, T, depth_scale=1.0, depth_trunc=4.0)
            oracle_of(s, frames[2:], voxel, trunc, cpu=cpu)
            assert gpu.dropped_points() == 0
            assert_same_volume(gpu, cpu, swept=True)


# ---- 3. batch splits and call sequences -----------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 128, 129])
def test_batch_split_into_sweeps_matches_the_oracle(F, sweep_form):
    """One integrate_batch call of F frames = ceil(F / 64) sweeps (a 1-frame tail at 65 and 129, an odd number of sweeps at 129)."""
    s, frames = tiny_frames(0, F)
    cpu = oracle_of(s, frames, 0.02, 0.08)
    d, c, T = stack(frames)
    gpu = volume(0.02, 0.08)
    gpu.integrate_batch(*cuda(d, c), intrinsic(s), T, depth_scale=1.0, depth_trunc=4.0)
    assert_same_volume(gpu, cpu, swept=True)


def test_batch_split_without_the_pipeline_and_through_integrate_frames(monkeypatch):
    """129 frames with the two-stream chain off (HV_TSDF_PIPELINE=0), and integrate_frames (host staging + chunking) of 65 and 129."""
    s, frames = tiny_frames(0, 129)
    K = intrinsic(s)
    d, c, T = stack(frames)
    cpu = oracle_of(s, frames, 0.02, 0.08)
    monkeypatch.setenv("HV_TSDF_PIPELINE", "0")
    gpu = volume(0.02, 0.08)
    gpu.integrate_batch(*cuda(d, c), K, T, depth_scale=1.0, depth_trunc=4.0)
    assert_same_volume(gpu, cpu, swept=True)
    monkeypatch.delenv("HV_TSDF_PIPELINE")
    staged = volume(0.02, 0.08)
    staged.integrate_frames([f[0] for f in frames], [f[1] for f in frames], K, T, depth_scale=1.0, depth_trunc=4.0)
    assert_same_volume(staged, cpu, swept=True)
    staged = volume(0.02, 0.08)
    staged.integrate_frames([f[0] for f in frames[:65]], [f[1] for f in frames[:65]], K, T[:65], depth_scale=1.0, depth_trunc=4.0)
    assert_same_volume(staged, oracle_of(s, frames[:65], 0.02, 0.08), swept=True)


def test_call_sequence_with_odd_sweep_counts_and_online_frames(sweep_form):
    """Batches of 65, 1 (the online path inside a running chain), 63 and 64 frames into one volume; the oracle after every call."""
    s, frames = tiny_frames(0, 193)
    K = intrinsic(s)
    gpu = volume(0.02, 0.08)
    cpu = oracle.PortTsdf(0.02, 0.08, threads=8)
    lo = 0
    for n in (65, 1, 63, 64):
        d, c, T = stack(frames[lo:lo + n])
        gpu.integrate_batch(*cuda(d, c), K, T, depth_scale=1.0, depth_trunc=4.0)
        oracle_of(s, frames[lo:lo + n], 0.02, 0.08, cpu=cpu)
        assert_same_volume(gpu, cpu, swept=True)
        lo += n


def test_shape_and_intrinsics_changes_inside_a_running_chain(sweep_form):
    """Extends test_sweep_multiplier_table_follows_intrinsics: device batches and online frames mixed, the image shape and the
    intrinsics changing between calls (multiplier table cache, batch buffer regrowth, chain reset)."""
    from pyslam_amd.volumetric import RGBDImage

    other = dict(odd_config(160, 120), fx=140.0, cx=70.25)
    steps = [("tiny_160x120_2cm", 0, 5, "batch"), (odd_config(161, 119), 5, 3, "online"), (odd_config(161, 119), 8, 6, "batch"),
             (other, 14, 1, "batch"), (other, 15, 7, "batch"), ("tiny_160x120_2cm", 22, 2, "online"),
             (odd_config(161, 119), 24, 70, "batch"), ("tiny_160x120_2cm", 94, 9, "batch")]
    gpu = volume(0.02, 0.08)
    cpu = oracle.PortTsdf(0.02, 0.08, threads=8)
    for cfg, start, n, how in steps:
        s, frames = tiny_frames(start, n) if cfg == "tiny_160x120_2cm" else frames_of(cfg, start, n)
        K = intrinsic(s)
        if how == "online":
            for d, c, T in frames:
                gpu.integrate(RGBDImage(*cuda(c, d), 1.0, 4.0), K, T)
        else:
            d, c, T = stack(frames)
            gpu.integrate_batch(*cuda(d, c), K, T, depth_scale=1.0, depth_trunc=4.0)
        oracle_of(s, frames, 0.02, 0.08, cpu=cpu)
        assert_same_volume(gpu, cpu, swept=True)


# ---- 4. bad depth values, far from the origin -----------------------------------------------------------------------------
def _plant(frames, values, dtype):
    """Each value at a few fixed pixels of every frame: on stride-4 sample positions (i % 4 == 0 and j % 4 == 0) and off them."""
    rng = np.random.default_rng(11)
    out = []
    H, W = frames[0][0].shape
    for f, (d, c, T) in enumerate(frames):
        d = d.copy()
        for k, val in enumerate(values):
            for _ in range(3):
                i, j = 4 * int(rng.integers(0, H // 4)), 4 * int(rng.integers(0, W // 4))
                d[i, j] = val
                d[min(i + 1 + k % 3, H - 1), min(j + 2, W - 1)] = val
        assert d.dtype == dtype
        out.append((d, c, T))
    return out


@pytest.mark.parametrize("depth_trunc", [4.0, 3.7])
def test_planted_float_depth_values(depth_trunc, monkeypatch):
    """0, -0, -1, NaN, +-inf, the smallest subnormal, FLT_MAX, exactly depth_trunc and the float below it: Open3D's
    `p /= scale; if (p >= trunc) p = 0; skip unless p > 0`, bit for bit, including the units the subnormal sample opens."""
    f32 = np.float32
    tr = f32(depth_trunc)
    values = [f32(0.0), f32(-0.0), f32(-1.0), f32(np.nan), f32(np.inf), f32(-np.inf), np.nextafter(f32(0), f32(1)),
              np.finfo(f32).max, tr, np.nextafter(tr, f32(0))]
    s, frames = frames_of(odd_config(161, 119), 0, 4)
    frames = _plant(frames, values, np.float32)
    assert np.isnan(frames[0][0]).any() and (frames[0][0] == np.nextafter(f32(0), f32(1))).any()
    check_every_entry_point(monkeypatch, s, frames, 0.02, 0.08, depth_trunc=depth_trunc)


@pytest.mark.parametrize("scale", [1000.0, 5000.0])
@pytest.mark.parametrize("above", [True, False], ids=["trunc_above_max", "trunc_below_max"])
def test_planted_u16_depth_values(scale, above, monkeypatch):
    """uint16 0, 1 and 65535 with depth_trunc just above / just below 65535 / scale."""
    s, frames = frames_of(odd_config(161, 119), 0, 4, "uint16", scale)
    frames = _plant(frames, [np.uint16(0), np.uint16(1), np.uint16(65535)], np.uint16)
    depth_trunc = 65535.0 / scale + (1e-3 if above else -1e-3)
    check_every_entry_point(monkeypatch, s, frames, 0.02, 0.08, depth_scale=scale, depth_trunc=depth_trunc)


OFFSET = np.array([-301.7, 203.3, -52.9])


@pytest.mark.parametrize("voxel,trunc", [(0.02, 0.08), (0.005, 0.04)])
def test_world_far_from_the_origin(voxel, trunc, monkeypatch):
    """The world translated by ~(-302, 203, -53) m (every T_cw post-multiplied by the translation: same depth images, large negative
    unit keys): online, both sweep forms and extraction against the oracle, whose float32 operation order holds at any magnitude."""
    from pyslam_amd.volumetric import RGBDImage

    s, frames = frames_of("synthetic_640x480_5mm", 30, 3)
    shift = np.eye(4)
    shift[:3, 3] = -OFFSET  # p_world' = p_world + OFFSET  ->  T_cw' = T_cw @ translate(-OFFSET)
    frames = [(d, c, T @ shift) for d, c, T in frames]
    K = intrinsic(s)
    cpu = oracle_of(s, frames, voxel, trunc)
    online = volume(voxel, trunc)
    for d, c, T in frames:
        online.integrate(RGBDImage(c, d, 1.0, 4.0), K, T)
    keys = online.unit_keys()
    assert (keys[:, 0] < -900 * 0.005 / voxel).all() and (keys[:, 2] < 0).all()
    assert_same_volume(online, cpu)
    assert assert_meshes_match(online, cpu) > 1000
    d, c, T = stack(frames)
    for form in SWEEP_FORMS:
        monkeypatch.setenv("HV_TSDF_SWEEP", form)
        dev = volume(voxel, trunc)
        dev.integrate_batch(*cuda(d, c), K, T, depth_scale=1.0, depth_trunc=4.0)
        assert_same_volume(dev, cpu, swept=True)


# ---- 5. operands in the wrong layout --------------------------------------------------------------------------------------
def test_wrong_layout_operands_fuse_like_the_canonical_arrays(monkeypatch):
    """A cropped depth view, an RGBA buffer sliced to RGB, float64 depth (numpy and torch), non-contiguous device tensors: the
    volume equals the one fused from the canonical arrays, bit for bit, on every entry point.  (Every wrong-layout operand is a
    view into an allocation at least as large as the canonical operand: read from its bare pointer it gives wrong values, never
    an access outside the allocation.)"""
    import torch

    from pyslam_amd.volumetric import RGBDImage

    monkeypatch.setenv("HV_TSDF_SWEEP", "2")
    s, frames = frames_of(odd_config(161, 119), 0, 3)
    K = intrinsic(s)
    d, c, T = stack(frames)
    F, H, W = d.shape
    big = np.zeros((F, H + 5, W + 7), np.float32)
    big[:, 2:2 + H, 3:3 + W] = d
    crop = big[:, 2:2 + H, 3:3 + W]
    rgba = np.full((F, H, W, 4), 200, np.uint8)
    rgba[..., :3] = c
    rgb_view = rgba[..., :3]
    d64 = d.astype(np.float64)
    assert not crop.flags.c_contiguous and not rgb_view.flags.c_contiguous

    def online(depths, colors):
        v = volume(0.02, 0.08)
        for k in range(F):
            v.integrate(RGBDImage(colors[k], depths[k], 1.0, 4.0), K, T[k])
        return v.dump()

    def batch(depths, colors):
        v = volume(0.02, 0.08)
        v.integrate_batch(depths, colors, K, T, depth_scale=1.0, depth_trunc=4.0)
        return v.dump()

    def staged(depths, colors):
        v = volume(0.02, 0.08)
        v.integrate_frames([depths[k] for k in range(F)], [colors[k] for k in range(F)], K, T, depth_scale=1.0, depth_trunc=4.0)
        return v.dump()

    want_online, want_batch = online(d, c), batch(d, c)
    cpu = oracle_of(s, frames, 0.02, 0.08)
    assert_dumps_match(want_online, cpu.dump())
    for depths, colors in ((crop, rgb_view), (d64, rgb_view), (crop, c)):
        for x, y in zip(online(depths, colors), want_online):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(batch(depths, colors), want_batch):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(staged(depths, colors), want_batch):
            np.testing.assert_array_equal(x, y)
    # device tensors: float64 depth, a crop of a larger depth tensor, RGBA sliced to RGB, frames taken with a step
    bigd = torch.from_numpy(big).cuda()
    rgbad = torch.from_numpy(rgba).cuda()
    d64d = torch.from_numpy(d64).cuda()
    pairs = [(bigd[:, 2:2 + H, 3:3 + W], rgbad[..., :3]), (d64d, rgbad[..., :3]),
             (torch.from_numpy(np.repeat(d, 2, axis=0)).cuda()[::2], torch.from_numpy(np.repeat(c, 2, axis=0)).cuda()[::2])]
    for depths, colors in pairs:
        assert not (depths.is_contiguous() and depths.dtype == torch.float32 and colors.is_contiguous())
        for x, y in zip(batch(depths, colors), want_batch):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(online(depths, colors), want_online):
            np.testing.assert_array_equal(x, y)


def test_mismatched_operands_are_refused_before_the_library():
    """Refusals on the device: colour / intrinsic shape, pose count, depth and colour on different devices.  Every operand is at
    least as large as the correct one."""
    import torch

    from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage

    s, frames = tiny_frames(0, 3)
    K = intrinsic(s)
    d, c, T = stack(frames)
    dd, cd = cuda(d, c)
    v = volume(0.02, 0.08)
    rgba = torch.zeros((3, 120, 160, 4), dtype=torch.uint8, device="cuda")
    bad_batch = [(dd, rgba, K, T), (dd, cd, PinholeCameraIntrinsic(159, 120, *s.intrinsics), T), (dd, cd, K, np.concatenate([T, T[:1]])),
                 (dd, c, K, T), (d, cd, K, T), (dd, cd.float(), K, T)]
    for args in bad_batch:
        with pytest.raises(RuntimeError, match="Unsupported image format"):
            v.integrate_batch(*args, depth_scale=1.0, depth_trunc=4.0)
    for img, k in ((RGBDImage(rgba[0], dd[0], 1.0, 4.0), K), (RGBDImage(c[0], dd[0], 1.0, 4.0), K),
                   (RGBDImage(cd[0], dd[0], 1.0, 4.0), PinholeCameraIntrinsic(160, 119, *s.intrinsics))):
        with pytest.raises(RuntimeError, match="Unsupported image format"):
            v.integrate(img, k, T[0])
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        v.integrate_frames(list(dd), list(cd), K, T, depth_scale=1.0, depth_trunc=4.0)  # integrate_frames takes host frames
    v.integrate_batch(dd[:0], cd[:0], K, T[:0])
    v.synchronize()
    assert v.num_blocks() == 0


# ---- 6. ray cast at odd shapes, tile sharding at odd widths ---------------------------------------------------------------
@pytest.fixture(scope="module")
def closed_form_volume():
    from pyslam_amd.volumetric import RGBDImage
    from tests import tsdf_closed_form as cf

    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    v = volume(cf.VOXEL, cf.TRUNC)
    K = PinholeCameraIntrinsic(cf.W, cf.H, *cf.K)
    for d, c, T in cf.frames():
        v.integrate(RGBDImage(c, d, 1.0, cf.DEPTH_TRUNC), K, T)
    v.synchronize()
    return v


@pytest.mark.parametrize("W,H", [(161, 119), (7, 5), (1, 1), (643, 481)])
def test_ray_cast_at_odd_shapes(closed_form_volume, W, H):
    from pyslam_amd.volumetric import PinholeCameraIntrinsic
    from tests import raycast_reference as rr
    from tests import tsdf_closed_form as cf
    from tests.test_gpu_tsdf_raycast import assert_agrees

    f = cf.K[0] * max(1.0, max(W, H) / 640.0)  # (small images: a narrow view of the scene's centre, every ray near a surface)
    intr = (f * 1.02, f * 0.98, 0.37 * W, 0.61 * H)
    vol = closed_form_volume
    gpu = vol.ray_cast(PinholeCameraIntrinsic(W, H, *intr), cf.POSES[1], 0.1, 3.0, weight_threshold=0.5)
    ref = rr.ray_cast(vol.dump(), cf.VOXEL, cf.TRUNC, intr, cf.POSES[1], H, W, 0.1, 3.0, 0.5)
    assert gpu["depth"].shape == (H, W) and gpu["color"].shape == (H, W, 3)
    assert_agrees(gpu, ref, f"{W}x{H}")


@pytest.mark.parametrize("W,H", [(161, 119), (164, 120)])
def test_tile_sharding_at_odd_widths_sums_to_the_oracle(W, H):
    """3 in-process ranks, tile-sharded (tile_bounds: 54 / 109 at W = 164, not multiples of 4; W = 161 leaves the pack role's tile
    skip off): the ranks' exported numerators sum to the oracle's and their unit sets together are exactly its set."""
    from pyslam_amd.distributed import tile_bounds

    s, frames = frames_of(odd_config(W, H), 0, 12)
    K = intrinsic(s)
    cpu = oracle_of(s, frames, 0.02, 0.08)
    keys, tsdf, w, colour = cpu.dump()
    ranks = [volume(0.02, 0.08) for _ in range(3)]
    for r, v in enumerate(ranks):
        v.set_tile(*tile_bounds(r, 3, W, H))
    d, c, T = stack(frames)
    dd, cd = cuda(d, c)
    for lo in (0, 5):
        hi = 12 if lo else 5
        for v in ranks:
            v.integrate_batch(dd[lo:hi], cd[lo:hi], K, T[lo:hi], depth_scale=1.0, depth_trunc=4.0)
    held = [{tuple(k) for k in v.unit_keys().tolist()} for v in ranks]
    assert set().union(*held) == {tuple(k) for k in keys.tolist()}
    total = np.zeros((len(keys), 4096, 5), np.float64)
    for v in ranks:
        assert v.dropped_points() == 0
        total += v.export_numerators(np.ascontiguousarray(keys))
    total = total.reshape(len(keys), 16, 16, 16, 5).transpose(0, 2, 3, 1, 4).reshape(len(keys), 4096, 5)
    np.testing.assert_array_equal(total[..., 1], w)
    ww = np.maximum(w, 1.0)
    assert np.abs(total[..., 0] / ww - tsdf * (w > 0)).max() <= TOL
    assert np.abs(total[..., 2:] / ww[..., None] - colour * (w > 0)[..., None]).max() / 255.0 <= TOL
