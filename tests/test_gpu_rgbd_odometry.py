"""GPU: frame-to-frame RGB-D odometry, _Volume.rgbd_odometry / rgbd_odometry_model (hv_rgbd_odometry[_model]) and the stream class
pyslam_amd.odometry.VisualOdometryRgbd: the target model bit for bit against the numpy restatement (tests/odometry_reference.py),
the whole call step by step against it, its accuracy on the synthetic room and the textured wall (the conditions of
tests/test_odometry_reference_cpu.py), and its API promises.

The restatement, not the kernel, is the yardstick.  Parameters are passed explicitly where a result depends on them."""
import types

import numpy as np
import pytest
import torch

from tests import odometry_cases as oc
from tests import odometry_reference as od

pytestmark = pytest.mark.gpu

ITERATIONS = (10, 5, 4)
HYBRID = dict(intensity_weight=0.01, intensity_huber_delta=0.1)


def _K(w, h, k):
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    return PinholeCameraIntrinsic(w, h, *k)


def same(a, b, photometric=True):
    """Bitwise the same call result."""
    assert np.array_equal(a.transformation, b.transformation) and np.array_equal(a.information, b.information)
    assert a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse and a.success == b.success
    assert a.iterations == b.iterations and a.degenerate == b.degenerate and a.inliers == b.inliers and a.valid == b.valid
    if photometric:
        assert a.photometric_inliers == b.photometric_inliers and a.intensity_rmse == b.intensity_rmse


@pytest.fixture(scope="module")
def vol():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    return ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 12)


@pytest.fixture(scope="module")
def tiny():
    """Frames 40 .. 44 of the 160x120 stream: (stream, K, {i: (depth, rgb, T_cw)})"""
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD("tiny_160x120_2cm")
    return s, _K(s.width, s.height, s.intrinsics), {i: s[i] for i in range(40, 45)}


@pytest.fixture(scope="module")
def room():
    """(intrinsics, camera, {i: (depth, rgb, T_cw)}) of the noisy 640x480 room and of its noise-free twin, for oc.ROOM_PAIRS"""
    from pyslam_amd.synthetic import SyntheticRGBD

    out = {}
    for noise in (True, False):
        s = SyntheticRGBD("synthetic_640x480_5mm", noise=noise)
        wanted = sorted({i for pair in oc.ROOM_PAIRS for i in pair}) if noise else [40, 44]
        out[noise] = (s.intrinsics, _K(s.width, s.height, s.intrinsics), {i: s[i] for i in wanted})
    return out


# -- 1. the model, bit for bit ---------------------------------------------------------------------------------------------------------

def check_model(vol, depth, rgb, h, w, level=0, trunc=0.07, depth_scale=1.0, depth_min=0.1, depth_max=3.0, device=False):
    K = oc.intrinsics(h, w)
    got = vol.rgbd_odometry_model(depth, _K(w, h, K), color=rgb, level=level, depth_scale=depth_scale, depth_min=depth_min,
                                  depth_max=depth_max, depth_outlier_trunc=trunc, device=device)
    if device:
        got = {k: (None if v is None else v.cpu().numpy()) for k, v in got.items()}
    host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else a
    ref = od.model_level(host(depth), host(rgb), K, level, depth_scale, depth_min, depth_max, trunc)
    assert got["depth"].shape == (h >> level, w >> level) and got["mask"].dtype == np.bool_
    for key in ("depth", "normal", "mask", "record"):
        if ref[key] is None:
            assert got[key] is None, key
        else:
            assert np.array_equal(got[key], ref[key]), (key, h, w, level, int((got[key] != ref[key]).sum()))
    return got


@pytest.mark.parametrize("h,w,level", oc.SHAPES, ids=str)
def test_model_matches_reference_bit_for_bit(vol, h, w, level):
    """uint16 and float32 depths of the same values, with and without colour: depth, normal, mask and record equal the restatement's."""
    u16 = np.round(oc.surface(h, w, seed=h * w).astype(np.float64) * 5000.0).astype(np.uint16)
    f32 = u16.astype(np.float32) / np.float32(5000.0)
    rgb = oc.image(h, w)
    a = check_model(vol, f32, rgb, h, w, level)
    b = check_model(vol, u16, rgb, h, w, level, depth_scale=5000.0)
    c = check_model(vol, f32, None, h, w, level)
    d = check_model(vol, torch.from_numpy(f32).cuda(), torch.from_numpy(rgb).cuda(), h, w, level, device=True)
    for key in ("depth", "normal", "mask"):
        assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]) and np.array_equal(a[key], d[key]), key
    assert np.array_equal(a["record"], b["record"]) and np.array_equal(a["record"], d["record"])
    interior = max((h >> level) - 2, 0) * max((w >> level) - 2, 0)
    assert a["mask"].sum() <= interior and (interior == 0 or a["mask"].any())


def test_model_on_planted_depths(vol):
    rgb5, rgb3 = oc.image(5, 5), oc.image(3, 3)
    for k in range(4):  # each of the four neighbours invalid in turn
        got = check_model(vol, oc.neighbour_invalid(k), rgb5, 5, 5)
        assert not got["mask"][2, 2] and got["mask"].sum() == 5  # the centre, the hole and the hole's two other neighbours
    trunc, kept, dropped = oc.trunc_edge()  # a neighbour at exactly trunc, and one float32 further
    assert check_model(vol, kept, rgb3, 3, 3, trunc=trunc)["mask"][1, 1]
    assert not check_model(vol, dropped, rgb3, 3, 3, trunc=trunc)["mask"].any()
    z, dmin, dmax = oc.bad_values()  # NaN, inf, out of range
    got = check_model(vol, z, oc.image(7, 9), 7, 9, depth_min=dmin, depth_max=dmax)
    assert got["depth"][5, 2] == 3.0 and not got["depth"][[1, 1, 1, 3, 3, 3, 5, 5], [1, 4, 7, 2, 4, 6, 4, 6]].any()
    check_model(vol, z, oc.image(7, 9), 7, 9, level=1, depth_min=dmin, depth_max=dmax)


# -- 2. step by step -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hybrid", [False, True], ids=["depth-only", "hybrid"])
def test_call_matches_reference_step_by_step(vol, tiny, hybrid):
    _, K, f = tiny
    (dt, ct, _), (ds, cs, _) = f[40], f[44]
    kw = dict(source_color=cs, target_color=ct, **HYBRID) if hybrid else {}
    out = vol.rgbd_odometry(ds, dt, K, iterations=ITERATIONS, trace=True, **kw)
    assert out.success and len(out.trace) == sum(out.iterations)
    ref_kw = dict(source_rgb=cs, target_rgb=ct, lam=HYBRID["intensity_weight"], idelta=HYBRID["intensity_huber_delta"]) if hybrid else {}
    rep = od.check_call(out, ds, dt, tiny[0].intrinsics, iterations=ITERATIONS, **ref_kw)
    print("step by step (%s): %d rows, max xi rel %.3g, near pivots %s" % ("hybrid" if hybrid else "depth only", rep["rows"], rep["xi_rel"],
                                                                         rep["near_pivot"]))
    assert not rep["near_pivot"]
    if hybrid:
        assert out.photometric_inliers == out.inliers > 0 and all(r["photometric_inliers"] == r["inliers"] for r in out.trace)
    else:
        assert out.photometric_inliers is None and out.intensity_rmse is None


# -- 3. accuracy -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", oc.ROOM_PAIRS, ids=str)
def test_noisy_room_pairs(vol, room, pair):
    """Depth only, identity start, defaults: success, fitness > 0.5, error <= 10 % of the pair's true motion."""
    _, K, f = room[True]
    (dt, _, Tt), (ds, _, Ts) = f[pair[0]], f[pair[1]]
    true = od.relative_pose(Tt, Ts)
    out = vol.rgbd_odometry(ds, dt, K, iterations=ITERATIONS)
    (em, ed), (mm, md) = od.pose_error(out.transformation, true), od.motion(true)
    print("room %s: motion %.4g m %.3g deg, error %.3g m %.3g deg, fitness %.3f, iterations %s" % (pair, mm, md, em, ed, out.fitness,
                                                                                                out.iterations))
    assert out.success and out.fitness > 0.5, out
    assert em <= 0.10 * mm and ed <= 0.10 * md, (em, ed, mm, md)


@pytest.mark.parametrize("case", oc.wall_cases(), ids=lambda c: c[0])
def test_textured_wall(vol, case):
    """Depth only is degenerate at every level and returns init; hybrid at weights 0.01 and 0.1 is within 1e-4 m and 5e-3 deg."""
    name, scale, T_target, T_source = case
    Kw, W, H = oc.wall_intrinsics(scale)
    (dt, ct), (ds, cs) = oc.wall_frame(T_target, scale), oc.wall_frame(T_source, scale)
    true = od.relative_pose(T_target, T_source)
    plain = vol.rgbd_odometry(ds, dt, _K(W, H, Kw), iterations=ITERATIONS)
    assert not plain.success and plain.degenerate == 7 and np.array_equal(plain.transformation, np.eye(4)), plain
    for weight in (0.01, 0.1):
        out = vol.rgbd_odometry(ds, dt, _K(W, H, Kw), source_color=cs, target_color=ct, iterations=ITERATIONS, intensity_weight=weight,
                                intensity_huber_delta=0.1)
        em, ed = od.pose_error(out.transformation, true)
        print("wall %s weight %g: error %.3g m %.3g deg, iterations %s" % (name, weight, em, ed, out.iterations))
        assert out.success and out.degenerate == 0 and out.photometric_inliers == out.inliers, out
        assert em <= 1e-4 and ed <= 5e-3, (em, ed)


# -- 4. weight zero ----------------------------------------------------------------------------------------------------------------------

def test_weight_zero_is_the_depth_only_call_bit_for_bit(vol, tiny):
    _, K, f = tiny
    for t, s in ((40, 44), (41, 42)):
        (dt, ct, _), (ds, cs, _) = f[t], f[s]
        plain = vol.rgbd_odometry(ds, dt, K, iterations=ITERATIONS, trace=True)
        zero = vol.rgbd_odometry(ds, dt, K, source_color=cs, target_color=ct, iterations=ITERATIONS, intensity_weight=0.0,
                                 intensity_huber_delta=0.1, trace=True)
        same(plain, zero, photometric=False)
        assert plain.success and zero.photometric_inliers == zero.inliers and zero.intensity_rmse > 0.0
        assert len(plain.trace) == len(zero.trace)
        for x, y in zip(plain.trace, zero.trace):
            for key in x:
                assert np.array_equal(x[key], y[key]), key


# -- 5. init -----------------------------------------------------------------------------------------------------------------------------

def test_init(vol, tiny, room):
    _, K, f = tiny
    (dt, _, _), (ds, _, _) = f[40], f[44]
    first = vol.rgbd_odometry(ds, dt, K, iterations=ITERATIONS)
    again = vol.rgbd_odometry(ds, dt, K, init=first.transformation, iterations=ITERATIONS, trace=True)
    em, ed = od.pose_error(again.transformation, first.transformation)
    print("restart: %.3g m %.3g deg apart, level-0 iterations %d then %d" % (em, ed, first.iterations[0], again.iterations[0]))
    assert first.success and again.success and em <= 1e-6 and ed <= 1e-5 and again.iterations[0] <= first.iterations[0]
    assert np.array_equal(again.trace[0]["A"], first.transformation)
    # noise-free 640x480 pair started at the truth: stays within the noise-free bound (1 % of the motion)
    _, Kr, fr = room[False]
    (dt, _, Tt), (ds, _, Ts) = fr[40], fr[44]
    true = od.relative_pose(Tt, Ts)
    out = vol.rgbd_odometry(ds, dt, Kr, init=true, iterations=ITERATIONS)
    (em, ed), (mm, md) = od.pose_error(out.transformation, true), od.motion(true)
    print("noise-free from the truth: error %.3g m %.3g deg, iterations %s" % (em, ed, out.iterations))
    assert out.success and em <= 0.01 * mm and ed <= 0.01 * md


# -- 6. operands -------------------------------------------------------------------------------------------------------------------------

def test_operands_determinism_and_read_only(tiny):
    from pyslam_amd.volumetric import RGBDImage, ScalableTSDFVolume, VoxelBlockGrid

    _, K, f = tiny
    (dt, ct, Tt), (ds, cs, Ts) = f[40], f[44]
    fused = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 12)
    for depth, rgb, T in (f[40], f[41]):
        fused.integrate(RGBDImage.create_from_color_and_depth(rgb, depth, 1.0, 4.0, False), K, T)
    blocks, dirty = fused.num_blocks(), fused.dirty_keys()
    su, tu = (np.round(d * 5000.0).clip(0, 65535).astype(np.uint16) for d in (ds, dt))
    sf, tf = (u.astype(np.float32) / np.float32(5000.0) for u in (su, tu))
    kw = dict(iterations=ITERATIONS, **HYBRID)
    cuda = lambda a: torch.from_numpy(a).cuda()
    outs = [fused.rgbd_odometry(sf, tf, K, source_color=cs, target_color=ct, **kw),
            fused.rgbd_odometry(su, tu, K, source_color=cs, target_color=ct, depth_scale=5000.0, **kw),
            fused.rgbd_odometry(torch.from_numpy(sf), torch.from_numpy(tf), K, source_color=torch.from_numpy(cs), target_color=torch.from_numpy(ct), **kw),
            fused.rgbd_odometry(cuda(sf), cuda(tf), K, source_color=cuda(cs), target_color=cuda(ct), **kw),
            fused.rgbd_odometry(cuda(su), cuda(tu), K, source_color=cuda(cs), target_color=cuda(ct), depth_scale=5000.0, **kw),
            fused.rgbd_odometry(sf.astype(np.float64), tf.astype(np.float64), K, source_color=cs, target_color=np.asfortranarray(ct), **kw)]
    outs += [fused.rgbd_odometry(sf, tf, K, source_color=cs, target_color=ct, **kw) for _ in range(3)]
    grid = VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12)  # another mode as context
    outs.append(grid.rgbd_odometry(sf, tf, K, source_color=cs, target_color=ct, **kw))
    for o in outs[1:]:
        same(o, outs[0])
    assert outs[0].success and outs[0].photometric_inliers > 0
    plain = [fused.rgbd_odometry(sf, tf, K, iterations=ITERATIONS), fused.rgbd_odometry(cuda(su), cuda(tu), K, depth_scale=5000.0, iterations=ITERATIONS),
             grid.rgbd_odometry(sf, tf, K, iterations=ITERATIONS)]
    for o in plain[1:]:
        same(o, plain[0])
    assert fused.num_blocks() == blocks and np.array_equal(fused.dirty_keys(), dirty)
    assert grid.num_blocks() == 0


# -- 7. empty and bad inputs -------------------------------------------------------------------------------------------------------------

def test_empty_frames_and_errors(vol, tiny):
    from pyslam_amd import _lib as L

    _, K, f = tiny
    (dt, ct, _), (ds, cs, _) = f[40], f[44]
    T0 = od.relative_pose(f[40][2], f[44][2])
    zero = np.zeros_like(ds)
    for a, b in ((zero, dt), (ds, zero), (zero, zero)):
        for kw in ({}, dict(source_color=cs, target_color=ct, **HYBRID)):
            out = vol.rgbd_odometry(a, b, K, init=T0, iterations=ITERATIONS, **kw)
            assert not out.success and np.array_equal(out.transformation, T0) and out.fitness == 0.0 and out.inliers == 0
            assert out.degenerate == 7 and out.iterations == (1, 1, 1)
            if kw:
                assert out.photometric_inliers == 0 and out.intensity_rmse == 0.0
    vol.synchronize()
    vol.profile_enable(True)
    vol.profile_read()
    with pytest.raises(ValueError, match="both source_color and target_color"):
        vol.rgbd_odometry(ds, dt, K, source_color=cs)
    with pytest.raises(ValueError, match="both source_color and target_color"):
        vol.rgbd_odometry(ds, dt, K, target_color=ct)
    with pytest.raises(ValueError, match="same shape"):
        vol.rgbd_odometry(ds, dt[:-1], K)
    with pytest.raises(ValueError, match="same dtype"):
        vol.rgbd_odometry(ds, (dt * 1000).astype(np.uint16), K)
    with pytest.raises(ValueError, match="same place"):
        vol.rgbd_odometry(torch.from_numpy(ds).cuda(), dt, K)
    with pytest.raises(RuntimeError):
        vol.rgbd_odometry(ds[:-1], dt[:-1], K)
    for bad in (np.full((4, 4), np.nan), np.diag([1.0, 1.0, 1.0, np.inf])):
        with pytest.raises(ValueError, match="init"):
            vol.rgbd_odometry(ds, dt, K, init=bad)
    with pytest.raises(L.HipVolError, match="bad image size"):
        vol.rgbd_odometry(ds, dt, K, iterations=(4, 1, 1, 1, 1, 1, 1, 1))  # 120 >> 7 == 0
    with pytest.raises(L.HipVolError, match="level"):
        vol.rgbd_odometry(ds, dt, K, iterations=(1,) * 9)
    with pytest.raises(L.HipVolError, match="level 0"):
        vol.rgbd_odometry(ds, dt, K, iterations=(0, 3))
    with pytest.raises(L.HipVolError, match="depth range"):
        vol.rgbd_odometry(ds, dt, K, depth_min=2.0, depth_max=1.0)
    with pytest.raises(L.HipVolError, match="positive"):
        vol.rgbd_odometry(ds, dt, K, depth_outlier_trunc=0.0)
    with pytest.raises(L.HipVolError, match="intensity"):
        vol.rgbd_odometry(ds, dt, K, source_color=cs, target_color=ct, intensity_weight=-1.0)
    # the C ABI itself: exactly one colour, a bad bottom row
    prm, _ = vol._odometry_params(1.0, 0.1, 3.0, (1,), 0.07, 0.05, 0.01, 0.1)
    res = L.HvOdometryResult()
    intr = K.as_array()

    def call(sc, tc, T=None):
        return vol._lib.hv_rgbd_odometry(vol._h, L.ptr(ds), L.ptr(dt), L.HV_DEPTH_F32, sc, tc, 120, 160, L.ptr(intr), L.ptr(T), L.ctypes.byref(prm),
                                         L.ctypes.byref(res), None, 0, None, L.HV_HOST)

    with pytest.raises(L.HipVolError, match="both colour images"):
        L.check(call(L.ptr(cs), None))
    with pytest.raises(L.HipVolError, match="both colour images"):
        L.check(call(None, L.ptr(ct)))
    with pytest.raises(L.HipVolError, match="bottom row"):
        L.check(call(None, None, np.ones((4, 4))))
    _, launches, _ = vol.profile_read()
    vol.profile_enable(False)
    assert launches == 0, "a refused call queued a launch"
    L.check(call(None, None, np.eye(4)))
    assert res.success == 1 and res.photometric_inliers == 0


# -- 8. ordering -------------------------------------------------------------------------------------------------------------------------

def test_call_is_ordered_after_async_torch_work(vol, tiny):
    """A CUDA depth written by an asynchronous torch op on the current stream just before the call is read after that write."""
    _, K, f = tiny
    (dt, _, _), (ds, _, _) = f[40], f[44]
    src, tgt = torch.from_numpy(ds).cuda(), torch.from_numpy(dt).cuda()
    buf = torch.zeros_like(src)
    x = torch.full((2048, 2048), 1e-3, device="cuda")
    torch.cuda.synchronize()
    for _ in range(20):  # work the write has to wait behind
        x = (x @ x).clamp_(-1.0, 1.0)
    buf.copy_(src)
    early = vol.rgbd_odometry(buf, tgt, K, iterations=ITERATIONS)
    torch.cuda.synchronize()
    late = vol.rgbd_odometry(buf, tgt, K, iterations=ITERATIONS)
    assert late.success and late.fitness > 0.5
    same(early, late)


# -- 9. the stream class -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["hybrid", "point_to_plane"])
def test_stream_class_is_the_product_of_the_pairwise_results(vol, tiny, method):
    from pyslam_amd.odometry import VisualOdometryRgbd

    s, K, f = tiny
    cam = types.SimpleNamespace(fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, width=s.width, height=s.height)
    vo = VisualOdometryRgbd(vol, cam, method=method, keep_on_device=True, iterations=ITERATIONS, **HYBRID)
    want = np.eye(4)
    for i in range(40, 45):
        depth, rgb, _ = f[i]
        T = vo.track(rgb, depth)
        if i > 40:
            kw = dict(source_color=rgb, target_color=f[i - 1][1]) if method == "hybrid" else {}
            pair = vol.rgbd_odometry(depth, f[i - 1][0], K, iterations=ITERATIONS, **HYBRID, **kw)
            assert pair.success and not vo.lost
            same(vo.last_result, pair, photometric=method == "hybrid")
            want = want @ pair.transformation
        assert np.array_equal(T, want), i
    print("stream %s over 40..44: %.3g m %.3g deg from the truth" % (method, *od.pose_error(want, od.relative_pose(f[40][2], f[44][2]))))
    # an all-zero depth frame: lost, the pose stays; the frame after it has an empty target and is lost too
    T = vo.track(f[44][1], np.zeros_like(f[44][0]))
    assert vo.lost and not vo.last_result.success and np.array_equal(T, want)
    T = vo.track(f[44][1], f[44][0])
    assert vo.lost and np.array_equal(T, want)
    T = vo.track(f[43][1], f[43][0])
    assert not vo.lost and vo.last_result.success and not np.array_equal(T, want)
