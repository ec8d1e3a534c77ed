"""CPU: the numpy restatement of hv_tsdf_track_color (tests/track_color_reference.py) on the analytic scene of
tests/test_track_reference_cpu.py, coloured by a smooth function of the world point.  The photometric term must remove the
single-plane degeneracy, must not hurt where geometry suffices, J_I must be the derivative of r_I, weight 0 must be the depth-only
linearisation, and the intensity pyramid / gradient rules must hold pixel by pixel."""
import copy

import numpy as np
import pytest

from tests import track_color_reference as tc
from tests import track_reference as tr
from tests.test_track_reference_cpu import DIRECTIONS, PLANES, SHAPES_CPU, T_TRUE, H, K, W, perturbed, render

_f32 = np.float32
WEIGHT, DELTA_I = 0.01, 0.1
STARTS = [(d, deg, m) for d in range(len(DIRECTIONS)) for deg, m in ((1.0, 0.02), (3.0, 0.05))]


def texture(p):
    """Smooth colour of world points p [...,3] -> [...,3] in [0, 1]."""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    r = 0.5 + 0.25 * np.sin(9.0 * x + 2.0 * y) + 0.2 * np.sin(5.0 * y - 3.0 * z + 1.0)
    g = 0.5 + 0.25 * np.sin(7.0 * y + 3.0 * z + 0.5) + 0.2 * np.sin(11.0 * x + 0.3)
    b = 0.5 + 0.25 * np.sin(6.0 * x - 8.0 * y + 2.0) + 0.2 * np.sin(4.0 * z + 13.0 * x)
    return np.clip(np.stack([r, g, b], -1), 0.0, 1.0)


def render_rgb(T_cw, Kl, h, w, **kw):
    """render() plus the texture at the hit points: (depth, normal, mask, colour float32 in [0, 1])."""
    depth, nrm, mask = render(T_cw, Kl, h, w, **kw)
    fx, fy, cx, cy = Kl
    T_wc = np.linalg.inv(T_cw)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    pc = depth.astype(np.float64)[..., None] * np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    pw = pc @ T_wc[:3, :3].T + T_wc[:3, 3]
    return depth, nrm, mask, np.where(mask[..., None], texture(pw), 0.0).astype(_f32)


def model_of(T_init, **kw):
    return lambda level, Kl, h, w: render_rgb(T_init, Kl, h, w, **kw)


def frame(**kw):
    depth, _, _, col = render_rgb(T_TRUE, K, H, W, **kw)
    return depth, np.rint(col.astype(np.float64) * 255.0).astype(np.uint8)


@pytest.fixture(scope="module")
def plane_frame():
    return frame(planes=PLANES[:1], sphere=False)


@pytest.fixture(scope="module")
def scene_frame():
    return frame()


@pytest.mark.parametrize("direction,deg,metres", STARTS)
def test_single_textured_plane_is_no_longer_degenerate(plane_frame, direction, deg, metres):
    """One exact plane: depth only is degenerate and returns the start; the hybrid call recovers the pose."""
    depth, rgb = plane_frame
    kw = dict(planes=PLANES[:1], sphere=False)
    T0 = perturbed(T_TRUE, *DIRECTIONS[direction], deg, metres)
    plain = tr.track(depth, K, T0, lambda level, Kl, h, w: render(T0, Kl, h, w, **kw))
    assert not plain["success"] and plain["degenerate"] & 1
    out = tc.track(depth, rgb, K, T0, model_of(T0, **kw), lam=WEIGHT, idelta=DELTA_I)
    dt, dr = tr.pose_error(out["T_cw"], T_TRUE)
    print("plane, start %d %.0f deg: %.3g m, %.3g deg, iterations %s" % (direction, deg, dt, dr, out["iterations"]))
    assert out["success"] and out["degenerate"] == 0, out["iterations"]
    assert dt <= 1e-5 and dr <= 5e-4, (dt, dr, out["iterations"])
    assert out["photometric_inliers"] > 0.5 * out["inliers"] and out["intensity_rmse"] < 0.01


@pytest.mark.parametrize("direction,deg,metres", STARTS)
def test_full_scene_is_not_hurt(scene_frame, direction, deg, metres):
    depth, rgb = scene_frame
    T0 = perturbed(T_TRUE, *DIRECTIONS[direction], deg, metres)
    out = tc.track(depth, rgb, K, T0, model_of(T0), lam=WEIGHT, idelta=DELTA_I)
    dt, dr = tr.pose_error(out["T_cw"], T_TRUE)
    print("scene, start %d %.0f deg: %.3g m, %.3g deg" % (direction, deg, dt, dr))
    assert out["success"] and out["degenerate"] == 0
    assert dt <= 1e-5 and dr <= 1e-4, (dt, dr, out["iterations"])


def _fixed_association(scene_frame):
    depth, rgb = scene_frame
    T0 = perturbed(T_TRUE, (1, 2, 0), (0, 1, -1), 2.0, 0.03)
    src, isrc = tr.source_level0(depth), tc.intensity_level0(rgb)
    model = render_rgb(T0, K, H, W)
    A = tr.exp_twist(np.array([0.004, -0.003, 0.002, 0.005, 0.004, -0.006]))
    return src, isrc, model, T0[:3, :3], A


def test_photometric_jacobian_matches_finite_differences(scene_frame):
    """With the association (the model pixel and its record) held fixed, J_I is the derivative of r_I along exp(xi) A, where
    x' - u' moves with the projection.  The step keeps every x' inside its pixel (pixels within 1e-3 of a boundary are left out)."""
    src, isrc, model, R0, A = _fixed_association(scene_frame)
    I, gx, gy, ok = tc.model_record(model[3], model[0], model[2], 0.07)
    valid, a = tr.associate(src, model, K, A, R0, 0.07)
    pk = ok[a["vi"], a["ui"]] & (np.abs(a["dx"]) < 0.499) & (np.abs(a["dy"]) < 0.499)
    assert pk.sum() > 40000
    pc, us, vs = a["pc"][pk], a["ui"][pk], a["vi"][pk]
    Im, Gx, Gy, Is = I[vs, us], gx[vs, us], gy[vs, us], isrc[a["v"][pk], a["u"][pk]]

    def r_of(A_):
        # r_I with (u', v') fixed: x' - u' taken against the fixed pixel
        fx, fy, cx, cy = K
        p = np.stack(tr.transform(A_, pc[:, 0], pc[:, 1], pc[:, 2]), 1)
        dx, dy = fx * p[:, 0] / p[:, 2] + cx - us, fy * p[:, 1] / p[:, 2] + cy - vs
        return ((Im.astype(np.float64) + Gx.astype(np.float64) * dx) + Gy.astype(np.float64) * dy) - Is.astype(np.float64)

    r0, J = tc.photometric(A, pc, K, Im, Gx, Gy, Is)
    assert np.abs(r0 - r_of(A)).max() < 1e-12
    eps = 1e-6
    Jfd = np.zeros_like(J)
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = eps
        Jfd[:, k] = (r_of(tr.exp_twist(xi) @ A) - r_of(tr.exp_twist(-xi) @ A)) / (2 * eps)
    assert np.abs(Jfd - J).max() < 1e-7 * max(1.0, np.abs(J).max()), np.abs(Jfd - J).max()
    assert np.abs(J).max() > 1.0  # (the texture has gradients: the check is not vacuous)


def test_weight_zero_is_the_depth_only_linearisation(scene_frame):
    src, isrc, model, R0, A = _fixed_association(scene_frame)
    ref = tr.linearise(src, model[:3], K, A, R0, 0.07, 0.05)
    lin = tc.linearise(src, isrc, model, K, A, R0, 0.07, 0.05, 0.0, DELTA_I)
    assert lin["inliers"] == ref["inliers"] and lin["valid"] == ref["valid"]
    assert 0 < lin["photometric_inliers"] <= lin["inliers"] and lin["sq_intensity_error"] > 0.0
    bar = 2.0 * (ref["inliers"] + 2) * tr.EPS
    assert (np.abs(lin["H"] - ref["H"]) <= bar * ref["H_abs"]).all() and (np.abs(lin["g"] - ref["g"]) <= bar * ref["g_abs"]).all()
    assert lin["sq_error"] == ref["sq_error"]
    full = tc.linearise(src, isrc, model, K, A, R0, 0.07, 0.05, WEIGHT, DELTA_I)
    assert np.abs(full["H"] - ref["H"]).max() > 1e3 * bar * ref["H_abs"].max()  # and a positive weight does change H


# -- intensity pyramid and gradient rules, pixel by pixel -----------------------------------------------------------------------------

def scalar_intensity(rgb, bgr=False):
    h, w = rgb.shape[:2]
    out = np.zeros((h, w), _f32)
    for v in range(h):
        for u in range(w):
            c = [_f32(x) for x in rgb[v, u]]
            r, g, b = (c[2], c[1], c[0]) if bgr else c
            out[v, u] = _f32(_f32(_f32(_f32(_f32(0.299) * r) + _f32(_f32(0.587) * g)) + _f32(_f32(0.114) * b)) / _f32(255))
    return out


def scalar_intensity_down(i):
    h, w = i.shape[0] // 2, i.shape[1] // 2
    out = np.zeros((h, w), _f32)
    for v in range(h):
        for u in range(w):
            s = _f32(_f32(_f32(i[2 * v, 2 * u] + i[2 * v, 2 * u + 1]) + i[2 * v + 1, 2 * u]) + i[2 * v + 1, 2 * u + 1])
            out[v, u] = _f32(s * _f32(0.25))
    return out


@pytest.mark.parametrize("h,w", SHAPES_CPU)
def test_intensity_pyramid_matches_scalar_loops(h, w):
    rgb = np.random.default_rng(h * 31 + w).integers(0, 256, (h, w, 3)).astype(np.uint8)
    rgb.flat[::7] = 255
    rgb.flat[3::11] = 0
    for bgr in (False, True):
        lv = tc.intensity_pyramid(rgb, 3 if min(h, w) >= 4 else 1, bgr)
        ref = scalar_intensity(rgb, bgr)
        assert np.array_equal(lv[0], ref)
        for level in lv[1:]:
            ref = scalar_intensity_down(ref)
            assert np.array_equal(level, ref) and level.shape == ref.shape
    assert np.array_equal(tc.intensity_level0(rgb, True), tc.intensity_level0(rgb[..., ::-1], False))
    if min(h, w) >= 2:
        assert tc.intensity_down(tc.intensity_level0(rgb)).shape == (h // 2, w // 2)


def test_gradient_validity_on_a_hand_made_map():
    """5x5: borders never; a mask hole kills itself and its four neighbours; a depth step of more than trunc kills both sides."""
    col = np.zeros((5, 5, 3), _f32)
    col[..., 0] = np.arange(5, dtype=_f32)[None, :] * _f32(0.1)
    col[..., 1] = np.arange(5, dtype=_f32)[:, None] * _f32(0.05)
    depth = np.ones((5, 5), _f32)
    mask = np.ones((5, 5), bool)
    I, gx, gy, ok = tc.model_record(col, depth, mask, 0.07)
    inner = np.zeros((5, 5), bool)
    inner[1:4, 1:4] = True
    assert np.array_equal(ok, inner)
    assert I[2, 3] == _f32(_f32(_f32(0.299) * col[2, 3, 0]) + _f32(_f32(0.587) * col[2, 3, 1])) + _f32(_f32(0.114) * col[2, 3, 2])
    assert gx[2, 2] == _f32(0.5) * _f32(I[2, 3] - I[2, 1]) and gy[2, 2] == _f32(0.5) * _f32(I[3, 2] - I[1, 2])
    assert gx[2, 2] > 0 and gy[2, 2] > 0 and not gx[~ok].any() and not gy[~ok].any()
    # a hole at (row 2, col 2)
    hole = mask.copy()
    hole[2, 2] = False
    ok2 = tc.model_record(col, depth, hole, 0.07)[3]
    expect = inner.copy()
    for v, u in ((2, 2), (1, 2), (3, 2), (2, 1), (2, 3)):
        expect[v, u] = False
    assert np.array_equal(ok2, expect)
    # a hole on the border kills the inner pixel next to it only
    edge = mask.copy()
    edge[0, 1] = False
    expect = inner.copy()
    expect[1, 1] = False
    assert np.array_equal(tc.model_record(col, depth, edge, 0.07)[3], expect)
    # a depth edge between columns 2 and 3: 0.0701 apart kills columns 2 and 3, exactly trunc apart keeps them
    step = depth.copy()
    step[:, 3:] = _f32(1.0701)
    expect = inner.copy()
    expect[:, 2:4] = False
    assert np.array_equal(tc.model_record(col, step, mask, 0.07)[3], expect)
    step[:, 3:] = _f32(1.0625)
    assert np.array_equal(tc.model_record(col, step, mask, 0.0625)[3], inner)
    step[:, 3:] = np.nextafter(_f32(1.0625), _f32(2))
    assert np.array_equal(tc.model_record(col, step, mask, 0.0625)[3], expect)
    # fewer than 3 pixels either way: no gradient anywhere
    for shape in ((2, 5), (5, 2), (1, 1)):
        assert not tc.model_record(np.ones(shape + (3,), _f32), np.ones(shape, _f32), np.ones(shape, bool), 0.07)[3].any()


# -- the step checker the GPU test uses, on the restatement's own call ----------------------------------------------------------------

def test_check_call_accepts_the_reference_and_rejects_one_pixel():
    w2, h2 = W // 4, H // 4
    K2 = tr.level_intrinsics(K, 2)
    depth, _, _, col = render_rgb(T_TRUE, K2, h2, w2)
    rgb = np.rint(col.astype(np.float64) * 255.0).astype(np.uint8)
    T0 = perturbed(T_TRUE, (1, 0, 1), (0, 1, 0), 1.0, 0.02)
    its = (6, 3)
    kw = dict(lam=WEIGHT, idelta=DELTA_I)
    out = tc.Result(tc.track(depth, rgb, K2, T0, model_of(T0), iterations=its, **kw))
    rep = tc.check_call(out, depth, rgb, K2, T0, model_of(T0), its, **kw)
    assert rep["rows"] == len(out.trace) and rep["xi_rel"] == 0.0 and not rep["near_pivot"]
    row = out.trace[-1]
    n, ni = row["inliers"], row["photometric_inliers"]
    assert ni > 1000

    def broken(edit):
        o = copy.deepcopy(out)
        edit(o)
        with pytest.raises(AssertionError):
            tc.check_call(o, depth, rgb, K2, T0, model_of(T0), its, **kw)

    # one photometric pixel's worth of H and g: the photometric part of the sums times 1 / n_I
    geo = tr.linearise(tr.pyramid(depth, 2)[0], model_of(T0)(0, K2, h2, w2)[:3], K2, row["A"], T0[:3, :3], 0.07, 0.05)

    def one_pixel_H(o):
        o.trace[-1]["H"] = o.trace[-1]["H"] + (o.trace[-1]["H"] - geo["H"]) / ni

    def one_pixel_g(o):
        o.trace[-1]["g"] = o.trace[-1]["g"] + (o.trace[-1]["g"] - geo["g"]) / ni

    broken(one_pixel_H)
    broken(one_pixel_g)
    broken(lambda o: o.trace[-1].update(sq_intensity_error=o.trace[-1]["sq_intensity_error"] * (1.0 + 1.0 / ni)))
    broken(lambda o: o.trace[0].update(photometric_inliers=o.trace[0]["photometric_inliers"] + 1))
    broken(lambda o: o.trace[0].update(inliers=o.trace[0]["inliers"] + 1))
    broken(lambda o: o.trace[-1].update(sq_error=o.trace[-1]["sq_error"] * (1.0 + 1.0 / n)))
    broken(lambda o: setattr(o, "photometric_inliers", o.photometric_inliers - 1))
    broken(lambda o: setattr(o, "intensity_rmse", np.nextafter(o.intensity_rmse, 1.0)))
    broken(lambda o: setattr(o, "inlier_rmse", np.nextafter(o.inlier_rmse, 1.0)))
    broken(lambda o: o.trace[0].update(status=1))
