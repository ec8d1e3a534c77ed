"""CPU: the numpy restatement of hv_tsdf_track (tests/track_reference.py) against an analytic scene - a back wall, two tilted panels
and a sphere - whose depth and normal maps are exact.  It must recover known perturbations, its H must be the Jacobian of its
residuals, and a single plane must be reported as degenerate.

What is left of the error is the sphere's: the association rounds to the nearest model pixel, and on a curved surface that leaves a
residual of about |p - q|^2 / (2 r) per pixel.  At 640 x 480 that keeps the recovered pose within 1e-5 m / 1e-4 deg (planes alone:
~1e-8 m)."""
import numpy as np
import pytest

from tests import track_reference as tr

W, H = 640, 480
K = np.array([525.0, 525.0, 319.5, 239.5])


def _unit(v):
    return np.asarray(v, float) / np.linalg.norm(v)


# Three non-parallel planes (n . x = c, hit kept where `keep(x)`) and a sphere.  The two front panels end in mid-air well in front of
# the back wall and the sphere floats in front of both, so every depth edge is a jump of more than depth_outlier_trunc: no pixel
# pairs two different surfaces, and the pixel-rounded association leaves no bias on the planes.
PLANES = [(_unit((0.1, -0.2, -1.0)), float(_unit((0.1, -0.2, -1.0)) @ (0.0, 0.0, 2.4)), lambda x: np.ones(x.shape[:-1], bool)),
          (_unit((0.7, 0.1, -0.7)), float(_unit((0.7, 0.1, -0.7)) @ (-0.35, 0.0, 1.3)), lambda x: x[..., 0] < -0.08),
          (_unit((-0.6, 0.35, -0.75)), float(_unit((-0.6, 0.35, -0.75)) @ (0.35, 0.0, 1.4)), lambda x: x[..., 0] > 0.08)]
SPHERE_C, SPHERE_R = np.array([0.0, 0.18, 0.95]), 0.14
T_TRUE = np.linalg.inv(tr.exp_twist(np.array([0.05, -0.08, 0.03, 0.04, -0.03, 0.02])))


def render(T_cw, Kl, h, w, planes=PLANES, sphere=True):
    """Exact z-depth (float32), world normal (float32, towards the camera) and hit mask of the scene."""
    fx, fy, cx, cy = Kl
    T_wc = np.linalg.inv(T_cw)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ T_wc[:3, :3].T
    o = T_wc[:3, 3]
    t = np.full((h, w), np.inf)
    nrm = np.zeros((h, w, 3))
    for n, c, keep in planes:
        with np.errstate(divide="ignore", invalid="ignore"):
            tp = (c - o @ n) / (d @ n)
            hit = np.isfinite(tp) & (tp > 0) & (tp < t)
        hit &= keep(o + np.where(hit, tp, 0.0)[..., None] * d)
        t = np.where(hit, tp, t)
        nrm[hit] = n
    if sphere:
        oc = o - SPHERE_C
        a = (d * d).sum(-1)
        b = 2.0 * (d @ oc)
        disc = b * b - 4 * a * (oc @ oc - SPHERE_R ** 2)
        with np.errstate(invalid="ignore"):
            ts = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        hit = (ts > 0) & (ts < t)
        t = np.where(hit, ts, t)
        p = o + np.where(hit, ts, 0.0)[..., None] * d
        nrm[hit] = ((p - SPHERE_C) / SPHERE_R)[hit]
    mask = np.isfinite(t)
    depth = np.where(mask, t, 0.0).astype(np.float32)
    return depth, np.where(mask[..., None], nrm, 0.0).astype(np.float32), mask


def model_of(T_init, **kw):
    return lambda level, Kl, h, w: render(T_init, Kl, h, w, **kw)


def perturbed(T_cw, axis_r, axis_t, deg, metres):
    """The camera moved by a rotation of `deg` about axis_r and a translation of `metres` along axis_t (camera frame)."""
    xi = np.concatenate([np.radians(deg) * np.asarray(axis_r, float) / np.linalg.norm(axis_r),
                         metres * np.asarray(axis_t, float) / np.linalg.norm(axis_t)])
    return np.linalg.inv(np.linalg.inv(T_cw) @ tr.exp_twist(xi))


DIRECTIONS = [((1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0)), ((1, 1, 0), (-1, 0, 1)), ((0, -1, 1), (1, 1, 1)),
              ((-1, 1, 1), (1, -1, 0))]


@pytest.mark.parametrize("deg,metres", [(1.0, 0.02), (3.0, 0.05)])
@pytest.mark.parametrize("direction", range(len(DIRECTIONS)))
def test_recovers_known_perturbations(direction, deg, metres):
    depth = render(T_TRUE, K, H, W)[0]
    T0 = perturbed(T_TRUE, *DIRECTIONS[direction], deg, metres)
    out = tr.track(depth, K, T0, model_of(T0))
    dt, dr = tr.pose_error(out["T_cw"], T_TRUE)
    assert out["success"] and out["degenerate"] == 0, out["iterations"]
    assert dt < 1e-5 and dr < 1e-4, (dt, dr, out["iterations"])
    assert out["fitness"] > 0.8 and out["inlier_rmse"] < 1e-4  # (the model is cast at the perturbed start: it misses a margin)
    # the trace: coarse to fine, states chained by exp(xi)
    levels = [r["level"] for r in out["trace"]]
    assert levels == sorted(levels, reverse=True) and levels[-1] == 0
    for a, b in zip(out["trace"], out["trace"][1:]):
        assert np.allclose(tr.exp_twist(a["xi"]) @ a["A"], b["A"], atol=1e-15)


def test_start_at_the_true_pose_stays():
    depth = render(T_TRUE, K, H, W)[0]
    out = tr.track(depth, K, T_TRUE, model_of(T_TRUE))
    dt, dr = tr.pose_error(out["T_cw"], T_TRUE)
    assert out["success"] and dt < 1e-6 and dr < 1e-5, (dt, dr)


def test_hessian_matches_finite_differences():
    """With the associations held fixed, H = sum w J^T J and g = sum w J^T r for J the derivative of r along exp(xi) A."""
    depth = render(T_TRUE, K, H, W)[0]
    T0 = perturbed(T_TRUE, (1, 2, 0), (0, 1, -1), 2.0, 0.03)
    src = tr.source_level0(depth)
    model = render(T0, K, H, W)
    R0 = T0[:3, :3]
    A = tr.exp_twist(np.array([0.004, -0.003, 0.002, 0.005, 0.004, -0.006]))
    valid, a = tr.associate(src, model, K, A, R0, 0.07)
    pc, q, n = a["pc"], a["q"], a["n"]
    assert valid > 50000 and len(pc) > 40000
    r0, J = tr.residuals(A, pc, q, n)
    eps = 1e-6
    Jfd = np.zeros_like(J)
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = eps
        rp, _ = tr.residuals(tr.exp_twist(xi) @ A, pc, q, n)
        rm, _ = tr.residuals(tr.exp_twist(-xi) @ A, pc, q, n)
        Jfd[:, k] = (rp - rm) / (2 * eps)
    assert np.abs(Jfd - J).max() < 1e-7
    w = tr.huber(r0, 0.05)
    lin = tr.linearise(src, model, K, A, R0, 0.07, 0.05)
    assert lin["inliers"] == len(r0) and lin["valid"] == valid
    Hfd = (w[:, None] * Jfd).T @ Jfd
    assert np.allclose(lin["H"], Hfd, rtol=1e-6, atol=1e-9 * np.abs(Hfd).max())
    assert np.allclose(lin["g"], (w[:, None] * Jfd).T @ r0, rtol=1e-6, atol=1e-9 * np.abs(lin["g"]).max())


def test_single_plane_is_degenerate():
    plane = PLANES[:1]
    depth = render(T_TRUE, K, H, W, planes=plane, sphere=False)[0]
    T0 = perturbed(T_TRUE, (1, 0, 0), (0, 1, 0), 1.0, 0.02)
    out = tr.track(depth, K, T0, model_of(T0, planes=plane, sphere=False))
    assert not out["success"] and out["degenerate"] & 1
    assert out["trace"][-1]["status"] == 2


def test_pyramid_rules():
    d = np.array([[1.0, 1.02, 0.0, 2.0], [1.04, 0.0, 2.5, 2.0]], np.float32)
    lv = tr.pyramid(d, 2, trunc=0.07)
    assert lv[1].shape == (1, 2)
    assert lv[1][0, 0] == np.float32((np.float32(1.0) + np.float32(1.02) + np.float32(1.04))) / np.float32(3)
    assert lv[1][0, 1] == 0.0  # 2.5 - 2.0 > trunc
    src = tr.source_level0(np.array([[np.nan, np.inf, 0.05, 0.1001], [3.0, 3.0001, -1.0, 1.0]], np.float32))
    assert src.tolist()[0][:3] == [0.0, 0.0, 0.0] and src[0, 3] > 0 and src[1, 0] == np.float32(3.0) and not src[1, 1:3].any()
    u16 = tr.source_level0(np.array([[5000, 65535]], np.uint16), depth_scale=5000.0, depth_max=20.0)
    assert u16[0, 0] == 1.0 and u16[0, 1] == np.float32(65535) / np.float32(5000)
    assert np.allclose(tr.level_intrinsics(K, 1), [262.5, 262.5, 159.5, 119.5])


# -- the source pyramid against plain per-pixel loops -----------------------------------------------------------------------------

_f32 = np.float32


def scalar_source(depth, depth_scale=1.0, depth_min=0.1, depth_max=3.0):
    """hv_tsdf_track's level 0, one pixel at a time: float32 divide, compares in float64."""
    h, w = depth.shape
    out = np.zeros((h, w), _f32)
    s = _f32(depth_scale)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for v in range(h):
            for u in range(w):
                d = _f32(_f32(depth[v, u]) / s)
                if np.isfinite(d) and float(d) > depth_min and float(d) <= depth_max:
                    out[v, u] = d
    return out


def scalar_downsample(d, trunc):
    """One level down, one parent at a time: the valid children in the order (2u,2v), (2u+1,2v), (2u,2v+1), (2u+1,2v+1)."""
    h, w = d.shape[0] // 2, d.shape[1] // 2
    out = np.zeros((h, w), _f32)
    for v in range(h):
        for u in range(w):
            s, n, mx, mn = _f32(0.0), 0, _f32(-np.inf), _f32(np.inf)
            for c in (d[2 * v, 2 * u], d[2 * v, 2 * u + 1], d[2 * v + 1, 2 * u], d[2 * v + 1, 2 * u + 1]):
                if c > 0:
                    s = _f32(s + c)
                    mx, mn = max(mx, c), min(mn, c)
                    n += 1
            if n > 0 and float(_f32(mx - mn)) <= trunc:
                out[v, u] = _f32(s / _f32(n))
    return out


SUB = _f32(1e-40)
PLANTED = [np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, SUB, np.nextafter(_f32(0), _f32(1)), 0.25, np.nextafter(_f32(0.25), _f32(1)),
           _f32(0.1), np.nextafter(_f32(0.1), _f32(0)), 3.0, np.nextafter(_f32(3.0), _f32(np.inf)), 1.0, 1.0625,
           np.nextafter(_f32(1.0625), _f32(np.inf))]


def _closed_form_frame(W, H):
    from tests import tsdf_closed_form as cf

    K = np.array([cf.K[0] * W / cf.W, cf.K[1] * H / cf.H, cf.K[2] * W / cf.W, cf.K[3] * H / cf.H])
    return cf.render(cf.POSES[0], cf.camera(W, H, K))[0]


def _planted_frame(h, w, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.05, 3.5, (h, w)).astype(_f32)
    pick = rng.random((h, w)) < 0.4
    d[pick] = np.asarray(PLANTED, _f32)[rng.integers(0, len(PLANTED), int(pick.sum()))]
    return d


def _pairs_frame(h, w, seed):
    """2x2 blocks of 1.0 and 1.0625 / the next float above (the trunc = 0.0625 edge), some children invalid."""
    rng = np.random.default_rng(seed)
    choices = np.asarray([0.0, 1.0, 1.0625, np.nextafter(_f32(1.0625), _f32(np.inf)), 1.03125], _f32)
    return choices[rng.integers(0, len(choices), (h, w))]


SHAPES_CPU = [(1, 9), (1, 64), (9, 1), (64, 1), (5, 7), (7, 5), (2, 2), (3, 3), (33, 17)]


@pytest.mark.parametrize("h,w", SHAPES_CPU)
@pytest.mark.parametrize("dmin,dmax", [(0.1, 3.0), (0.25, 3.0), (0.0, 2.5), (1.0, 1.0625)])
def test_source_level0_matches_scalar_loop(h, w, dmin, dmax):
    d = _planted_frame(h, w, h * 100 + w)
    assert np.array_equal(tr.source_level0(d, 1.0, dmin, dmax), scalar_source(d, 1.0, dmin, dmax), equal_nan=False)


@pytest.mark.parametrize("scale", [1000.0, 5000.0, 5000.1])
@pytest.mark.parametrize("h,w", [(1, 64), (64, 1), (7, 5), (33, 17)])
def test_source_level0_u16_matches_scalar_loop(h, w, scale):
    rng = np.random.default_rng(h * 7 + w)
    d = rng.integers(0, 20000, (h, w)).astype(np.uint16)
    d.flat[::5] = 0
    d.flat[1::5] = 65535
    ref = scalar_source(d, scale, 0.1, 3.0)
    assert np.array_equal(tr.source_level0(d, scale, 0.1, 3.0), ref)
    assert (ref > 0).any()


@pytest.mark.parametrize("h,w", SHAPES_CPU)
@pytest.mark.parametrize("trunc", [0.07, 0.0625, 0.01])
def test_downsample_matches_scalar_loop(h, w, trunc):
    for d in (tr.source_level0(_planted_frame(h, w, h + w), 1.0, 0.0, 3.5), _pairs_frame(h, w, h * w)):
        assert np.array_equal(tr.downsample(d, trunc), scalar_downsample(d, trunc))


def test_downsample_trunc_edge_and_subnormal_blocks():
    nxt = np.nextafter(_f32(1.0625), _f32(np.inf))
    d = np.array([[1.0, 1.0625, 1.0, nxt, SUB, SUB], [1.0, 1.0625, 1.0, nxt, SUB, np.nextafter(_f32(0), _f32(1))]], _f32)
    for out in (tr.downsample(d, 0.0625), scalar_downsample(d, 0.0625)):
        assert out[0, 0] == _f32(1.03125) and out[0, 1] == 0.0 and 0.0 < out[0, 2] < 1e-39


@pytest.mark.parametrize("crop", [(0, 0, 479, 641), (1, 3, 478, 637), (0, 0, 1, 641), (0, 0, 479, 1), (200, 300, 7, 5)])
def test_pyramid_of_a_closed_form_frame_matches_scalar_loops(crop):
    """641x479 closed-form frames (and crops) with planted values, five levels, every level against the loops."""
    full = _closed_form_frame(641, 479)
    full = np.where(np.random.default_rng(1).random(full.shape) < 0.02, _planted_frame(479, 641, 2), full).astype(_f32)
    y, x, h, w = crop
    d = full[y:y + h, x:x + w]
    lv = tr.pyramid(d, 5, depth_min=0.1, depth_max=3.0, trunc=0.07)
    ref = scalar_source(d)
    assert np.array_equal(lv[0], ref)
    for level in range(1, 5):
        ref = scalar_downsample(ref, 0.07)
        assert np.array_equal(lv[level], ref), level


# -- the step checker the GPU tests use, on the reference's own call ---------------------------------------------------------------

class _Out:
    """The reference's track() in the shape of an OdometryResult with a trace."""

    def __init__(self, r):
        self.transformation, self.fitness, self.inlier_rmse = r["T_cw"], r["fitness"], r["inlier_rmse"]
        self.information, self.success, self.iterations, self.degenerate = r["information"], r["success"], r["iterations"], r["degenerate"]
        last = r["trace"][-1]
        self.inliers, self.valid = last["inliers"], last["valid"]
        self.trace = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in row.items()} for row in r["trace"]]


def test_check_call_accepts_the_reference_and_rejects_one_pixel():
    """check_call passes the reference's own call; one pixel's worth of change to H, a count off by one or a wrong status fails it."""
    import copy

    w2, h2 = W // 4, H // 4
    K2 = tr.level_intrinsics(K, 2)
    depth = render(T_TRUE, K2, h2, w2)[0]
    T0 = perturbed(T_TRUE, (1, 0, 1), (0, 1, 0), 1.0, 0.02)
    its = (6, 3)
    r = tr.track(depth, K2, T0, model_of(T0), iterations=its)
    out = _Out(r)
    rep = tr.check_call(out, depth, K2, T0, model_of(T0), its)
    assert rep["rows"] == len(r["trace"]) and rep["xi_rel"] == 0.0 and not rep["near_pivot"]
    row = out.trace[-1]
    n = row["inliers"]

    def broken(edit):
        o = copy.deepcopy(out)
        edit(o)
        with pytest.raises(AssertionError):
            tr.check_call(o, depth, K2, T0, model_of(T0), its)

    def one_pixel(o):
        o.trace[-1]["H"] = o.trace[-1]["H"] * (1.0 + 1.0 / n)

    broken(one_pixel)
    broken(lambda o: o.trace[0].update(inliers=o.trace[0]["inliers"] + 1))
    broken(lambda o: o.trace[1].update(valid=o.trace[1]["valid"] - 1))
    broken(lambda o: o.trace[-1].update(sq_error=o.trace[-1]["sq_error"] * (1.0 + 1.0 / n)))
    broken(lambda o: o.trace[0].update(status=1))
    broken(lambda o: setattr(o, "degenerate", o.degenerate ^ 1))
    broken(lambda o: setattr(o, "iterations", (o.iterations[0] + 1, o.iterations[1])))
    broken(lambda o: setattr(o, "inlier_rmse", np.nextafter(o.inlier_rmse, 1.0)))
