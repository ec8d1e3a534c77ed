"""A numpy restatement of hv_tsdf_track_color (the hybrid contract in include/hipvol.h) - test infrastructure, no GPU.

Everything shared with the depth-only contract comes from tests/track_reference.py.  The model is whatever the caller hands in per
pyramid level: (depth, world normal, mask, colour [h,w,3] float32 in [0, 1]) at the initial pose.  Source intensity, model
intensity and gradients are float32 in the kernels' operation order, the photometric term float64 in theirs, so per pixel both sides
agree bit for bit and the sums differ only by their summation order.
"""
import numpy as np

from tests import track_reference as tr

COLOR_TRACE_STRIDE = 58

_f32 = np.float32
EPS = tr.EPS


def intensity_level0(rgb, bgr=False):
    """uint8 [h,w,3] -> float32 ((0.299f R + 0.587f G) + 0.114f B) / 255f."""
    c = np.asarray(rgb).astype(_f32)
    r, g, b = (c[..., 2], c[..., 1], c[..., 0]) if bgr else (c[..., 0], c[..., 1], c[..., 2])
    return (((_f32(0.299) * r + _f32(0.587) * g) + _f32(0.114) * b) / _f32(255)).astype(_f32)


def intensity_down(i):
    """level l -> l + 1: (((c0 + c1) + c2) + c3) * 0.25f over the children (2u,2v), (2u+1,2v), (2u,2v+1), (2u+1,2v+1)."""
    h, w = i.shape[0] // 2, i.shape[1] // 2
    s = ((i[0:2 * h:2, 0:2 * w:2] + i[0:2 * h:2, 1:2 * w:2]) + i[1:2 * h:2, 0:2 * w:2]) + i[1:2 * h:2, 1:2 * w:2]
    return (s * _f32(0.25)).astype(_f32)


def intensity_pyramid(rgb, n_levels, bgr=False):
    levels = [intensity_level0(rgb, bgr)]
    for _ in range(1, n_levels):
        levels.append(intensity_down(levels[-1]))
    return levels


def model_record(color, mdepth, mmask, trunc):
    """-> (I_m, g_x, g_y float32 [h,w], has-gradient bool [h,w]).  A pixel has a gradient iff it is off the border, the mask is set
    at it and its four neighbours and |z(neighbour) - z| <= trunc (float64 difference of the float32 depths); g = 0 elsewhere."""
    c = np.asarray(color, _f32)
    I = ((_f32(0.299) * c[..., 0] + _f32(0.587) * c[..., 1]) + _f32(0.114) * c[..., 2]).astype(_f32)
    h, w = I.shape
    gx, gy, ok = np.zeros((h, w), _f32), np.zeros((h, w), _f32), np.zeros((h, w), bool)
    if h < 3 or w < 3:
        return I, gx, gy, ok
    z = np.asarray(mdepth).astype(np.float64)
    m = np.asarray(mmask, bool)
    ctr = (slice(1, -1), slice(1, -1))
    nb = [(slice(1, -1), slice(2, None)), (slice(1, -1), slice(0, -2)), (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1))]
    good = m[ctr].copy()
    for s in nb:
        good &= m[s] & (np.abs(z[s] - z[ctr]) <= trunc)
    ok[ctr] = good
    gx[ctr] = np.where(good, _f32(0.5) * (I[nb[0]] - I[nb[1]]), _f32(0))
    gy[ctr] = np.where(good, _f32(0.5) * (I[nb[2]] - I[nb[3]]), _f32(0))
    return I, gx, gy, ok


def associate(src, model, K, A, R0, trunc):
    """tr.associate, also returning per inlier the source pixel (u, v), the model pixel (u', v') and the projection's offsets
    (x' - u', y' - v').  -> (valid, dict of arrays)."""
    mdepth, mnormal, mmask = model[:3]
    h, w = src.shape
    fx, fy, cx, cy = (float(k) for k in K)
    v, u = np.nonzero(src > 0)
    valid = len(u)
    d = src[v, u].astype(np.float64)
    pc = np.stack([d * ((u - cx) / fx), d * ((v - cy) / fy), d], axis=1)
    p = np.stack(tr.transform(A, pc[:, 0], pc[:, 1], pc[:, 2]), axis=1)
    keep = p[:, 2] > 0
    pc, p, u, v = pc[keep], p[keep], u[keep], v[keep]
    with np.errstate(over="ignore", invalid="ignore"):
        xf, yf = fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy
        uf, vf = np.floor(xf + 0.5), np.floor(yf + 0.5)
        keep = (uf >= 0) & (uf < w) & (vf >= 0) & (vf < h)
    pc, p, u, v, xf, yf, uf, vf = (a[keep] for a in (pc, p, u, v, xf, yf, uf, vf))
    ui, vi = uf.astype(np.int64), vf.astype(np.int64)
    keep = np.asarray(mmask, bool)[vi, ui]
    pc, p, u, v, xf, yf, uf, vf, ui, vi = (a[keep] for a in (pc, p, u, v, xf, yf, uf, vf, ui, vi))
    z = np.asarray(mdepth)[vi, ui].astype(np.float64)
    q = np.stack([z * ((uf - cx) / fx), z * ((vf - cy) / fy), z], axis=1)
    nw = np.asarray(mnormal)[vi, ui].astype(np.float64)
    n = np.stack([R0[r, 0] * nw[:, 0] + R0[r, 1] * nw[:, 1] + R0[r, 2] * nw[:, 2] for r in range(3)], axis=1)
    e = p - q
    keep = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]) <= trunc
    return valid, {"pc": pc[keep], "q": q[keep], "n": n[keep], "u": u[keep], "v": v[keep], "ui": ui[keep], "vi": vi[keep],
                   "dx": (xf - uf)[keep], "dy": (yf - vf)[keep]}


def photometric(A, pc, K, Im, gx, gy, Is):
    """r_I and J_I of fixed associations: pc [N,3] source camera points; Im, gx, gy [N] the associated model records; Is [N] the
    source intensities.  The offsets x' - u', y' - v' follow from the projection of A pc and the model pixel round(x'), round(y')."""
    fx, fy, cx, cy = (float(k) for k in K)
    p = np.stack(tr.transform(A, pc[:, 0], pc[:, 1], pc[:, 2]), axis=1)
    xf, yf = fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy
    return _photometric(p, xf - np.floor(xf + 0.5), yf - np.floor(yf + 0.5), fx, fy, Im, gx, gy, Is)


def _photometric(p, dx, dy, fx, fy, Im, gx, gy, Is):
    Im, gx, gy, Is = (np.asarray(a).astype(np.float64) for a in (Im, gx, gy, Is))
    r = ((Im + gx * dx) + gy * dy) - Is
    a = gx * fx / p[:, 2]
    b = gy * fy / p[:, 2]
    c = -(a * p[:, 0] + b * p[:, 1]) / p[:, 2]
    J = np.stack([p[:, 1] * c - p[:, 2] * b, p[:, 2] * a - p[:, 0] * c, p[:, 0] * b - p[:, 1] * a, a, b, c], axis=1)
    return r, J


def linearise(src, isrc, model, K, A, R0, trunc, delta, lam, idelta, record=None):
    """-> dict(H, g, sq_error, inliers, valid, H_abs, g_abs as tr.linearise, for the combined system; photometric_inliers,
    sq_intensity_error).  model = (depth, world normal, mask, colour); record = model_record(...) of it if already at hand."""
    if record is None:
        record = model_record(model[3], model[0], model[2], trunc)
    I, gx, gy, ok = record
    valid, a = associate(src, model, K, A, R0, trunc)
    r, J = tr.residuals(A, a["pc"], a["q"], a["n"])
    w = tr.huber(r, delta)
    pk = ok[a["vi"], a["ui"]]
    p = np.stack(tr.transform(A, a["pc"][pk, 0], a["pc"][pk, 1], a["pc"][pk, 2]), axis=1)
    us, vs = a["ui"][pk], a["vi"][pk]
    rI, JI = _photometric(p, a["dx"][pk], a["dy"][pk], float(K[0]), float(K[1]), I[vs, us], gx[vs, us], gy[vs, us],
                          isrc[a["v"][pk], a["u"][pk]])
    wI = lam * tr.huber(rI, idelta)
    H, H_abs, g, g_abs = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros(6), np.zeros(6)
    for i in range(6):
        wa, wb = w * J[:, i], wI * JI[:, i]
        for j in range(i, 6):
            t, s = wa * J[:, j], wb * JI[:, j]
            H[i, j] = H[j, i] = t.sum() + s.sum()
            H_abs[i, j] = H_abs[j, i] = np.abs(t).sum() + np.abs(s).sum()
        t, s = wa * r, wb * rI
        g[i], g_abs[i] = t.sum() + s.sum(), np.abs(t).sum() + np.abs(s).sum()
    return {"H": H, "g": g, "sq_error": float((r * r).sum()), "inliers": len(r), "valid": valid, "H_abs": H_abs, "g_abs": g_abs,
            "photometric_inliers": len(rI), "sq_intensity_error": float((rI * rI).sum())}


def track(depth, rgb, K, T_init, model, iterations=(10, 5, 4), depth_scale=1.0, depth_min=0.1, depth_max=3.0, trunc=0.07, delta=0.05,
          lam=0.01, idelta=0.1, bgr=False):
    """The whole call.  model(level, K_level, h, w) -> (depth, world normal, mask, colour) of the map cast at T_init.
    -> tr.track's dict plus photometric_inliers and intensity_rmse."""
    nl = len(iterations)
    srcs = tr.pyramid(depth, nl, depth_scale, depth_min, depth_max, trunc)
    ints = intensity_pyramid(rgb, nl, bgr)
    T_init = np.asarray(T_init, np.float64)
    R0 = T_init[:3, :3]
    A = np.eye(4)
    trace, iters, degenerate, last = [], [0] * nl, 0, None
    for level in range(nl - 1, -1, -1):
        if iterations[level] == 0:
            continue
        Kl = tr.level_intrinsics(K, level)
        h, w = srcs[level].shape
        maps = model(level, Kl, h, w)
        rec = model_record(maps[3], maps[0], maps[2], trunc)
        for it in range(iterations[level]):
            lin = linearise(srcs[level], ints[level], maps, Kl, A, R0, trunc, delta, lam, idelta, rec)
            xi, deg = tr.solve(lin["H"], lin["g"], lin["inliers"])
            row = dict(lin, level=level, iteration=it, A=A.copy(), xi=xi)
            iters[level] += 1
            if level == 0:
                last = lin
            if deg:
                row["status"] = 2
                trace.append(row)
                degenerate |= 1 << level
                break
            A = tr.exp_twist(xi) @ A
            row["status"] = 1 if tr.converged(xi) else 0
            trace.append(row)
            if row["status"] == 1:
                break
    inl, val, pin = last["inliers"], last["valid"], last["photometric_inliers"]
    return {"T_cw": tr.rigid_inverse(A) @ T_init, "fitness": inl / val if val else 0.0,
            "inlier_rmse": float(np.sqrt(last["sq_error"] / inl)) if inl else 0.0, "information": last["H"],
            "success": not (degenerate & 1) and inl >= tr.MIN_INLIERS, "iterations": tuple(iters), "degenerate": degenerate,
            "inliers": inl, "valid": val, "photometric_inliers": pin,
            "intensity_rmse": float(np.sqrt(last["sq_intensity_error"] / pin)) if pin else 0.0, "trace": trace}


class Result:
    """track()'s dict in the shape of an OdometryResult, so that check_call can be held against the restatement's own call."""

    def __init__(self, out):
        self.transformation, self.information = out["T_cw"], out["information"]
        self.fitness, self.inlier_rmse, self.success = out["fitness"], out["inlier_rmse"], out["success"]
        self.iterations, self.degenerate, self.inliers, self.valid = out["iterations"], out["degenerate"], out["inliers"], out["valid"]
        self.photometric_inliers, self.intensity_rmse = out["photometric_inliers"], out["intensity_rmse"]
        self.trace = [dict(r) for r in out["trace"]]


def check_call(out, depth, rgb, K, T_init, model, iterations, depth_scale=1.0, depth_min=0.1, depth_max=3.0, trunc=0.07, delta=0.05,
               lam=0.01, idelta=0.1, bgr=False):
    """Hold one traced hv_tsdf_track_color result to this restatement, step by step, with tr.check_call's rules:
      - valid, inliers and photometric_inliers are equal;
      - H, g of the combined system: |gpu - ref| <= 2 (n + 2) 2^-53 S element by element, n = inliers + photometric inliers (the
        number of terms in each sum) and S the sum of the terms' absolute values; the squared geometric error with n = inliers, the
        squared intensity error with n = photometric inliers, each against its own sum;
      - solve, degenerate decision, status, next A, schedule and outputs as tr.check_call; intensity_rmse and
        photometric_inliers from the last row.
    -> dict(rows, near_pivot, xi_rel)."""
    nl = len(iterations)
    T_init = np.asarray(T_init, np.float64)
    R0 = T_init[:3, :3]
    srcs = tr.pyramid(depth, nl, depth_scale, depth_min, depth_max, trunc)
    ints = intensity_pyramid(rgb, nl, bgr)
    rows = out.trace
    assert rows is not None and len(rows) == sum(out.iterations), (len(rows), out.iterations)
    assert len(out.iterations) == nl and out.degenerate >> nl == 0, (out.iterations, out.degenerate)

    # schedule
    k = 0
    for level in range(nl - 1, -1, -1):
        if iterations[level] == 0:
            assert out.iterations[level] == 0 and not out.degenerate >> level & 1, level
            continue
        start = k
        while k < len(rows) and rows[k]["level"] == level:
            k += 1
        grp = rows[start:k]
        assert 1 <= len(grp) <= iterations[level], (level, len(grp), iterations)
        assert [r["iteration"] for r in grp] == list(range(len(grp))), level
        assert all(r["status"] == 0 for r in grp[:-1]), (level, [r["status"] for r in grp])
        assert grp[-1]["status"] in (1, 2) or len(grp) == iterations[level], (level, grp[-1]["status"], len(grp))
        assert out.iterations[level] == len(grp), (level, out.iterations)
        assert bool(out.degenerate >> level & 1) == (grp[-1]["status"] == 2), (level, out.degenerate)
    assert k == len(rows), "rows out of the coarse-to-fine order"

    # every step
    maps, near, xi_rel = {}, [], 0.0
    A_next = np.eye(4)
    for k, row in enumerate(rows):
        level = row["level"]
        what = (k, level, row["iteration"])
        if k == 0:
            assert np.array_equal(row["A"], np.eye(4)), what
        else:
            assert np.abs(row["A"] - A_next).max() <= tr.A_REL * max(1.0, np.abs(A_next).max()), (what, row["A"], A_next)
        if level not in maps:
            Kl = tr.level_intrinsics(K, level)
            h, w = srcs[level].shape
            m = model(level, Kl, h, w)
            maps[level] = (Kl, m, model_record(m[3], m[0], m[2], trunc))
        Kl, m, rec = maps[level]
        ref = linearise(srcs[level], ints[level], m, Kl, row["A"], R0, trunc, delta, lam, idelta, rec)
        assert row["valid"] == ref["valid"], (what, "valid", row["valid"], ref["valid"])
        assert row["inliers"] == ref["inliers"], (what, "inliers", row["inliers"], ref["inliers"])
        assert row["photometric_inliers"] == ref["photometric_inliers"], (what, "photometric inliers", row["photometric_inliers"],
                                                                          ref["photometric_inliers"])
        bar = 2.0 * (ref["inliers"] + ref["photometric_inliers"] + 2) * EPS
        dH = np.abs(row["H"] - ref["H"])
        assert (dH <= bar * ref["H_abs"]).all(), (what, "H", float((dH / np.maximum(ref["H_abs"], 1e-300)).max()), bar)
        dg = np.abs(row["g"] - ref["g"])
        assert (dg <= bar * ref["g_abs"]).all(), (what, "g", float((dg / np.maximum(ref["g_abs"], 1e-300)).max()), bar)
        bar_e = 2.0 * (ref["inliers"] + 2) * EPS
        assert abs(row["sq_error"] - ref["sq_error"]) <= bar_e * ref["sq_error"], (what, "e", row["sq_error"], ref["sq_error"])
        bar_i = 2.0 * (ref["photometric_inliers"] + 2) * EPS
        assert abs(row["sq_intensity_error"] - ref["sq_intensity_error"]) <= bar_i * ref["sq_intensity_error"], (
            what, "e_I", row["sq_intensity_error"], ref["sq_intensity_error"])

        xi_ref, deg_ref = tr.solve(row["H"], row["g"], row["inliers"])
        if row["inliers"] >= tr.MIN_INLIERS and tr.pivot_near_threshold(row["H"]):
            near.append(what)
        else:
            assert (row["status"] == 2) == deg_ref, (what, "degenerate decision", row["status"], tr.pivots(row["H"]))
        if row["status"] == 2:
            assert not row["xi"].any(), what
            A_next = row["A"]
        else:
            if not deg_ref:
                scale = np.abs(xi_ref).max()
                rel = float(np.abs(row["xi"] - xi_ref).max() / scale) if scale > 0 else float(np.abs(row["xi"]).max())
                xi_rel = max(xi_rel, rel)
                assert rel <= tr.XI_REL, (what, "xi", row["xi"], xi_ref)
            assert (row["status"] == 1) == tr.converged(row["xi"]), (what, row["status"], row["xi"])
            A_next = tr.exp_twist(row["xi"]) @ row["A"]

    # outputs
    last = rows[-1]
    assert last["level"] == 0
    inl, val, pin = last["inliers"], last["valid"], last["photometric_inliers"]
    assert out.success == (last["status"] != 2 and inl >= tr.MIN_INLIERS), (out.success, last["status"], inl)
    assert np.array_equal(out.information, last["H"])
    assert out.inliers == inl and out.valid == val
    assert out.fitness == (inl / val if val else 0.0), (out.fitness, inl, val)
    assert out.inlier_rmse == (float(np.sqrt(last["sq_error"] / inl)) if inl else 0.0), (out.inlier_rmse, last["sq_error"], inl)
    assert out.photometric_inliers == pin, (out.photometric_inliers, pin)
    assert out.intensity_rmse == (float(np.sqrt(last["sq_intensity_error"] / pin)) if pin else 0.0), (
        out.intensity_rmse, last["sq_intensity_error"], pin)
    T_exp = tr.rigid_inverse(A_next) @ T_init
    assert np.abs(out.transformation - T_exp).max() <= 1e-12 * (1.0 + np.abs(T_init).max()), (out.transformation, T_exp)
    return {"rows": len(rows), "near_pivot": near, "xi_rel": xi_rel}
