"""GPU: ScalableTSDFVolume.track_frame_to_model (hv_tsdf_track) at the edges - odd shapes and pyramid depths, the grid-stride tail,
schedules, parameters that reach the Huber branch, planted source values at every compare, degenerate levels, operand forms and
scratch reuse - each call held step by step to tests/track_reference.py by track_reference.check_call: counts exact, H, g and the
squared error within a float64 summation bound, solve, schedule and outputs as the contract says.

The map is the closed-form plane-and-sphere scene (tests/tsdf_closed_form.py) fused at 640x480.  Source frames are rendered from
it at other sizes, with intrinsics scaled to the size (so the scene stays in view and cx, cy are fractional), at a pose 1 deg /
2 cm off the initial one.
"""
import warnings

import numpy as np
import pytest
import torch

from tests import raycast_reference as rr
from tests import track_reference as tr
from tests import tsdf_closed_form as cf
from tests.test_gpu_tsdf_raycast import assert_agrees

pytestmark = pytest.mark.gpu

WT = 0.5  # the map has 3 frames: the weight threshold the other closed-form tests use
T_INIT = cf.POSES[0]


def _K(w, h, k):
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    return PinholeCameraIntrinsic(w, h, *k)


def scaled_K(W, H):
    return np.array([cf.K[0] * W / cf.W, cf.K[1] * H / cf.H, cf.K[2] * W / cf.W, cf.K[3] * H / cf.H])


def perturbed(T_cw, axis_r, axis_t, deg, metres):
    xi = np.concatenate([np.radians(deg) * np.asarray(axis_r, float) / np.linalg.norm(axis_r),
                         metres * np.asarray(axis_t, float) / np.linalg.norm(axis_t)])
    return np.linalg.inv(np.linalg.inv(T_cw) @ tr.exp_twist(xi))


T_SRC = perturbed(T_INIT, (1, 1, 0), (0, 1, -1), 1.0, 0.02)  # where the source frames are rendered


def frame(W, H, T=T_SRC):
    """float32 z-depth of the closed-form scene at W x H, and its intrinsics."""
    K = scaled_K(W, H)
    return cf.render(T, cf.camera(W, H, K))[0], K


@pytest.fixture(scope="module")
def vol():
    return fused()


def fused():
    from pyslam_amd.volumetric import RGBDImage, ScalableTSDFVolume

    v = ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 14)
    for depth, rgb, T in cf.frames():
        v.integrate(RGBDImage(rgb, depth, 1.0, cf.DEPTH_TRUNC), _K(cf.W, cf.H, cf.K), T)
    v.synchronize()
    return v


def track(v, depth, K, iterations, T0=T_INIT, check=True, depth_scale=1.0, depth_min=0.1, depth_max=3.0, weight_threshold=WT,
          depth_outlier_trunc=0.07, depth_huber_delta=0.05):
    """One traced call, held to the reference step by step (check=True).  depth: a host array."""
    H, W = depth.shape
    out = v.track_frame_to_model(depth, _K(W, H, K), T0, depth_scale=depth_scale, depth_min=depth_min, depth_max=depth_max,
                                 weight_threshold=weight_threshold, iterations=iterations, depth_outlier_trunc=depth_outlier_trunc,
                                 depth_huber_delta=depth_huber_delta, trace=True)
    if not check:
        return out

    def model(level, Kl, h, w):
        m = v.ray_cast(_K(w, h, Kl), T0, depth_min, depth_max, weight_threshold, render_attributes=("depth", "normal", "mask"))
        return m["depth"], m["normal"], m["mask"]

    rep = tr.check_call(out, depth, K, T0, model, tuple(iterations), depth_scale=depth_scale, depth_min=depth_min, depth_max=depth_max,
                        trunc=depth_outlier_trunc, delta=depth_huber_delta)
    if rep["near_pivot"]:
        warnings.warn(f"degenerate decision not compared: a pivot within rounding of the threshold at rows {rep['near_pivot']}")
    print(f"{W}x{H} {tuple(iterations)}: rows {rep['rows']}, iterations {out.iterations}, degenerate {out.degenerate}, "
          f"success {out.success}, max xi rel {rep['xi_rel']:.3g}")
    return out


def same(a, b):
    """Bitwise the same call result."""
    assert np.array_equal(a.transformation, b.transformation) and np.array_equal(a.information, b.information)
    assert a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse and a.success == b.success
    assert a.iterations == b.iterations and a.degenerate == b.degenerate and a.inliers == b.inliers and a.valid == b.valid
    if a.trace is not None and b.trace is not None:
        assert len(a.trace) == len(b.trace)
        for x, y in zip(a.trace, b.trace):
            for key in x:
                assert np.array_equal(x[key], y[key]), key


# -- shapes x levels ---------------------------------------------------------------------------------------------------------------

SHAPES = [(641, 479, (10, 5, 4, 3, 2)), (641, 479, (4,) * 8), (161, 119, (10, 5, 4)), (7, 5, (10,)), (64, 1, (10,)),
          (511, 513, (10, 5)),  # 262 143 pixels: 1024 workgroups, the last one short of one pixel
          (513, 512, (10, 5)),  # 262 656 pixels: over the 1024-workgroup cap, so 512 pixels take a second lap
          (1280, 960, (10, 5, 4))]  # ~4.7 pixels per thread at level 0


@pytest.mark.parametrize("W,H,iterations", SHAPES, ids=[f"{w}x{h}-{len(it)}" for w, h, it in SHAPES])
def test_shapes_and_levels(vol, W, H, iterations):
    depth, K = frame(W, H)
    out = track(vol, depth, K, iterations)
    if W * H >= 161 * 119:
        assert out.success and out.fitness > 0.5, out
    if len(iterations) == 8:
        assert out.trace[0]["level"] == 7 and tr.pyramid(depth, 8)[7].shape == (3, 5)


def test_level_models_match_the_raycast_reference(vol):
    """The maps the call casts for 641x479 / 5 levels (fractional cx, cy, small images) agree with the numpy ray cast."""
    dump = vol.dump()
    K = scaled_K(641, 479)
    for level in range(5):
        Kl = tr.level_intrinsics(K, level)
        h, w = 479 >> level, 641 >> level
        gpu = vol.ray_cast(_K(w, h, Kl), T_INIT, 0.1, 3.0, WT)
        ref = rr.ray_cast(dump, cf.VOXEL, cf.TRUNC, Kl, T_INIT, h, w, 0.1, 3.0, WT)
        assert_agrees(gpu, ref, (level, w, h))


# -- schedules ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations", [(1,), (3, 0, 2), (2, 0, 0, 5), (4,) * 8], ids=str)
def test_schedules(vol, iterations):
    depth, K = frame(641, 479)
    track(vol, depth, K, iterations)


def test_iteration_cap_beyond_convergence_is_a_no_op(vol):
    depth, K = frame(641, 479, T_INIT)  # starts at the pose the frame was rendered at: converges within a few steps
    a = track(vol, depth, K, (50,))
    assert a.iterations[0] < 50 and a.trace[-1]["status"] == 1
    b = track(vol, depth, K, (10000,), check=False)
    same(a, b)


@pytest.mark.parametrize("iterations,shape", [((0, 3), (641, 479)), ((4,) * 9, (641, 479)), ((3, -1, 2), (641, 479)),
                                              ((10001,), (641, 479)), ((2, 2, 2, 2), (7, 5)), ((2, 2), (64, 1))],
                         ids=["level0-zero", "nine-levels", "negative", "10001", "7x5-4-levels", "64x1-2-levels"])
def test_bad_schedules_are_refused_and_change_nothing(vol, iterations, shape):
    from pyslam_amd import _lib as L

    depth, K = frame(641, 479)
    before = track(vol, depth, K, (10, 5, 4), check=False)
    d, Kd = frame(*shape)
    with pytest.raises(L.HipVolError):
        vol.track_frame_to_model(d, _K(shape[0], shape[1], Kd), T_INIT, iterations=iterations, weight_threshold=WT, trace=True)
    same(before, track(vol, depth, K, (10, 5, 4), check=False))


# -- parameters --------------------------------------------------------------------------------------------------------------------

PARAMS = [dict(depth_huber_delta=0.002), dict(depth_huber_delta=1e-4), dict(depth_outlier_trunc=0.01), dict(depth_outlier_trunc=0.2),
          dict(weight_threshold=2.5), dict(weight_threshold=5.0), dict(depth_min=1.5, depth_max=2.2)]


@pytest.mark.parametrize("kw", PARAMS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_parameters(vol, kw):
    depth, K = frame(641, 479)
    out = track(vol, depth, K, (10, 5, 4), **kw)
    if "depth_huber_delta" in kw:
        # most inliers are on the Huber branch at the first step
        row = out.trace[0]
        src = tr.pyramid(depth, 3)[2]
        m = vol.ray_cast(_K(src.shape[1], src.shape[0], tr.level_intrinsics(K, 2)), T_INIT, 0.1, 3.0, WT,
                         render_attributes=("depth", "normal", "mask"))
        _, a = tr.associate(src, (m["depth"], m["normal"], m["mask"]), tr.level_intrinsics(K, 2), row["A"], T_INIT[:3, :3], 0.07)
        r, _ = tr.residuals(row["A"], a["pc"], a["q"], a["n"])
        assert (np.abs(r) > kw["depth_huber_delta"]).mean() > 0.5
    if kw.get("weight_threshold") == 5.0:  # no voxel of a 3-frame map reaches it: nothing to track against
        assert out.degenerate == 7 and not out.success and out.inliers == 0


# -- planted source values ---------------------------------------------------------------------------------------------------------

def _plant(depth, values, step=(29, 31), at=(3, 5)):
    """values scattered over the frame, each at many pixels."""
    d = depth.copy()
    v, u = np.mgrid[at[0]:d.shape[0]:step[0], at[1]:d.shape[1]:step[1]]
    vals = np.asarray(values, d.dtype)
    d[v.ravel(), u.ravel()] = vals[np.arange(v.size) % len(vals)]
    return d


def _plant_blocks(depth, pairs, step=(34, 38)):
    """2x2 blocks at even coordinates: the left column gets pair[0], the right pair[1]."""
    d = depth.copy()
    v, u = np.mgrid[4:d.shape[0] - 1:step[0], 6:d.shape[1] - 1:step[1]]
    for k, (y, x) in enumerate(zip(v.ravel(), u.ravel())):
        a, b = pairs[k % len(pairs)]
        d[y:y + 2, x] = a
        d[y:y + 2, x + 1] = b
    return d


f32 = np.float32
SUBNORMAL = f32(1e-40)
TINY = np.nextafter(f32(0), f32(1))  # the smallest subnormal
# name -> (call parameters, [(planted value, valid at level 0)])
PLANTED = {
    "nonfinite-and-signs": (dict(), [(np.nan, False), (np.inf, False), (-np.inf, False), (-1.0, False), (-0.0, False),
                                     (SUBNORMAL, False)]),
    "depth_min-0.25": (dict(depth_min=0.25), [(0.25, False), (np.nextafter(f32(0.25), f32(1)), True)]),
    "depth_min-0.1": (dict(depth_min=0.1), [(f32(0.1), True), (np.nextafter(f32(0.1), f32(0)), False)]),  # compared in float64
    "depth_max-3": (dict(depth_max=3.0), [(3.0, True), (np.nextafter(f32(3.0), f32(np.inf)), False)]),
    "depth_min-0": (dict(depth_min=0.0), [(SUBNORMAL, True), (TINY, True), (-0.0, False), (0.0, False)]),
}


@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_float_values(vol, name):
    kw, planted = PLANTED[name]
    values = [x for x, _ in planted]
    src = tr.source_level0(np.array([values], f32), 1.0, kw.get("depth_min", 0.1), kw.get("depth_max", 3.0))
    assert (src[0] > 0).tolist() == [ok for _, ok in planted]
    depth, K = frame(641, 479)
    depth = _plant(depth, values)
    out = track(vol, depth, K, (10, 5, 4), **kw)
    assert out.success


def test_planted_subnormal_blocks(vol):
    """2x2 blocks of subnormals at depth_min = 0: valid at level 0 and (a float32 mean of subnormals) at level 1."""
    depth, K = frame(641, 479)
    depth = _plant_blocks(depth, [(SUBNORMAL, SUBNORMAL), (SUBNORMAL, np.nextafter(f32(0), f32(1)))])
    lv = tr.pyramid(depth, 3, depth_min=0.0)
    assert ((lv[1] > 0) & (lv[1] < 1e-30)).sum() > 50
    track(vol, depth, K, (10, 5, 4), depth_min=0.0)


def test_planted_blocks_at_the_outlier_trunc(vol):
    """depth_outlier_trunc = 0.0625: children 1.0 and 1.0625 make a valid parent, 1.0 and the next float32 above 1.0625 do not."""
    depth, K = frame(641, 479)
    bad = np.nextafter(f32(1.0625), f32(np.inf))
    depth = _plant_blocks(depth, [(1.0, 1.0625), (1.0, bad)])
    lv = tr.pyramid(depth, 2, trunc=0.0625)
    v, u = np.mgrid[4:478:34, 6:640:38]
    parents = lv[1][v.ravel() // 2, u.ravel() // 2]
    assert (parents[0::2] == f32(1.03125)).all() and not parents[1::2].any()
    track(vol, depth, K, (10, 5, 4), depth_outlier_trunc=0.0625)


@pytest.mark.parametrize("scale", [1000.0, 5000.0, 5000.1])
def test_planted_u16(vol, scale):
    depth, K = frame(641, 479)
    u16 = np.round(depth.astype(np.float64) * scale).clip(0, 65535).astype(np.uint16)
    u16 = _plant(u16, [0, 65535])
    out = track(vol, u16, K, (10, 5, 4), depth_scale=scale)
    assert out.success
    if scale == 5000.1:  # the scale is divided as a float32
        src = tr.source_level0(u16, scale)
        ok = src > 0
        assert float(f32(scale)) != scale and (src[ok] != (u16[ok] / scale).astype(f32)).any()


# -- degenerate paths --------------------------------------------------------------------------------------------------------------

def test_all_zero_frame(vol):
    depth = np.zeros((479, 641), np.float32)
    K = scaled_K(641, 479)
    out = track(vol, depth, K, (10, 5, 4, 3, 2))
    assert [(r["level"], r["status"]) for r in out.trace] == [(l, 2) for l in range(4, -1, -1)]
    assert out.degenerate == (1 << 5) - 1 and not out.success
    assert np.array_equal(out.transformation, T_INIT)
    assert out.fitness == 0.0 and out.inlier_rmse == 0.0 and not out.information.any()


def test_camera_facing_away(vol):
    depth, K = frame(641, 479)
    turn = np.eye(4)
    turn[:3, :3] = tr.exp_twist(np.array([0.0, np.pi, 0.0, 0.0, 0.0, 0.0]))[:3, :3]
    T0 = turn @ T_INIT
    out = track(vol, depth, K, (10, 5, 4), T0=T0)
    assert all(r["valid"] > 0 and r["inliers"] == 0 for r in out.trace)
    assert out.degenerate == 7 and not out.success


def test_tiny_frame_with_a_1x1_top_level(vol):
    depth, K = frame(7, 5)
    out = track(vol, depth, K, (10, 5, 4))
    assert out.degenerate & 4 and out.trace[0]["level"] == 2 and out.trace[0]["status"] == 2


# -- wrapper operands --------------------------------------------------------------------------------------------------------------

def _call(v, depth, K, W=641, H=479, T0=T_INIT, iterations=(10, 5, 4), **kw):
    kw.setdefault("weight_threshold", WT)
    return v.track_frame_to_model(depth, _K(W, H, K), T0, iterations=iterations, trace=True, **kw)


def test_operand_forms(vol):
    depth, K = frame(641, 479)
    base = track(vol, depth, K, (10, 5, 4))
    assert base.success
    same(base, _call(vol, np.asfortranarray(depth), K))
    same(base, _call(vol, depth.astype(np.float64), K))
    same(base, _call(vol, torch.from_numpy(depth), K))
    same(base, _call(vol, torch.from_numpy(depth.astype(np.float64)).cuda(), K))
    same(base, _call(vol, torch.from_numpy(np.ascontiguousarray(depth.T)).cuda().t(), K))  # transposed: strides (1, H)
    same(base, _call(vol, depth, K, iterations=np.array([10, 5, 4])))
    same(base, _call(vol, depth, K, iterations=np.array([10, 5, 4], np.int32)))
    same(base, _call(vol, depth, K, T0=torch.from_numpy(T_INIT.copy())))
    same(base, _call(vol, depth, K, T0=T_INIT.tolist()))
    T32 = T_INIT.astype(np.float32)
    ref32 = _call(vol, depth, K, T0=T32.astype(np.float64))
    same(ref32, _call(vol, depth, K, T0=T32))
    same(ref32, _call(vol, depth, K, T0=torch.from_numpy(T32)))


def test_cropped_views(vol):
    """A window of a larger frame, with the window's intrinsics: numpy view, CUDA view."""
    big, Kb = frame(700, 520)
    y0, x0 = 17, 29
    view = big[y0:y0 + 479, x0:x0 + 641]
    K = Kb - np.array([0.0, 0.0, x0, y0])
    assert not view.flags.c_contiguous
    base = track(vol, np.ascontiguousarray(view), K, (10, 5, 4))
    assert base.success
    same(base, _call(vol, view, K))
    cuda_view = torch.from_numpy(big).cuda()[y0:y0 + 479, x0:x0 + 641]
    assert not cuda_view.is_contiguous()
    same(base, _call(vol, cuda_view, K))


def test_integer_operands(vol):
    depth, K = frame(641, 479)
    mm = np.round(depth.astype(np.float64) * 1000.0).astype(np.int32)
    base = track(vol, mm.astype(np.float32), K, (10, 5, 4), depth_scale=1000.0)
    same(base, _call(vol, mm, K, depth_scale=1000.0))
    u16 = mm.astype(np.uint16)
    base16 = track(vol, u16, K, (10, 5, 4), depth_scale=1000.0)
    same(base16, _call(vol, u16.astype(np.float32), K, depth_scale=1000.0))  # u16 -> float32 is exact


def test_torch_uint16_operands(vol):
    if not hasattr(torch, "uint16"):
        pytest.skip(f"torch {torch.__version__} has no torch.uint16 (added in 2.3)")
    depth, K = frame(641, 479)
    u16 = np.round(depth.astype(np.float64) * 1000.0).astype(np.uint16)
    base = _call(vol, u16, K, depth_scale=1000.0)
    t16 = torch.from_numpy(u16.astype(np.int32)).to(torch.uint16)
    same(base, _call(vol, t16, K, depth_scale=1000.0))
    same(base, _call(vol, t16.cuda(), K, depth_scale=1000.0))


# -- scratch reuse -----------------------------------------------------------------------------------------------------------------

def test_scratch_reuse_across_sizes():
    v = fused()
    runs = [(641, 479, (10, 5, 4, 3, 2)), (7, 5, (10,)), (1280, 960, (10, 5, 4)), (641, 479, (10, 5, 4, 3, 2))]
    outs = []
    for W, H, it in runs:
        depth, K = frame(W, H)
        outs.append(track(v, depth, K, it, check=(W, H) != (1280, 960)))
    same(outs[0], outs[-1])
