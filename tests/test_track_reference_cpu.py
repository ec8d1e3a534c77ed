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
    valid, pc, q, n = tr.associate(src, model, K, A, R0, 0.07)
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
