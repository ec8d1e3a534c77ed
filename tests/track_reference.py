"""A numpy restatement of hv_tsdf_track (the contract in include/hipvol.h) - test infrastructure, no GPU - and the flow of
hv_tsdf_track_color: association, linearisation, the call's loop and the step-by-step checker take an optional photometric term,
which tests/track_color_reference.py supplies.

The model is whatever the caller hands in per pyramid level (depth, world normal and hit mask at the initial pose: the GPU's own
ray_cast maps in the GPU tests, an analytic scene in the CPU tests).  Everything else - source pyramid, association, linearisation,
Cholesky solve, update, stopping and outputs - follows the kernels operation by operation (float32 pyramid, float64 geometry in the
same order), so per pixel the two agree bit for bit and the sums differ only by their summation order.
"""
import numpy as np

# the named constants of include/hipvol.h
MAX_LEVELS = 8
MIN_INLIERS = 6
PIVOT_REL = 1e-10
CONVERGED = 1e-6
TRACE_STRIDE = 56

_f32 = np.float32


def source_level0(depth, depth_scale=1.0, depth_min=0.1, depth_max=3.0):
    """depth / depth_scale in float32; 0 where not finite or outside (depth_min, depth_max] (compared in float64)."""
    d = np.asarray(depth)
    d = d.astype(_f32) / _f32(depth_scale)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d) & (d.astype(np.float64) > depth_min) & (d.astype(np.float64) <= depth_max)
    return np.where(ok, d, _f32(0)).astype(_f32)


def downsample(d, trunc):
    """level l -> l + 1: float32 mean of the valid 2x2 children in the order (2u,2v), (2u+1,2v), (2u,2v+1), (2u+1,2v+1); valid iff
    max - min of the valid children <= trunc."""
    h, w = d.shape[0] // 2, d.shape[1] // 2
    kids = (d[0:2 * h:2, 0:2 * w:2], d[0:2 * h:2, 1:2 * w:2], d[1:2 * h:2, 0:2 * w:2], d[1:2 * h:2, 1:2 * w:2])
    s = np.zeros((h, w), _f32)
    n = np.zeros((h, w), np.int32)
    mx = np.full((h, w), -np.inf, _f32)
    mn = np.full((h, w), np.inf, _f32)
    for c in kids:
        v = c > 0
        s = np.where(v, s + c, s).astype(_f32)
        mx = np.where(v, np.maximum(mx, c), mx)
        mn = np.where(v, np.minimum(mn, c), mn)
        n += v
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (n > 0) & ((mx - mn).astype(np.float64) <= trunc)
        out = np.where(ok, s / n.astype(_f32), _f32(0))
    return out.astype(_f32)


def pyramid(depth, n_levels, depth_scale=1.0, depth_min=0.1, depth_max=3.0, trunc=0.07):
    levels = [source_level0(depth, depth_scale, depth_min, depth_max)]
    for _ in range(1, n_levels):
        levels.append(downsample(levels[-1], trunc))
    return levels


def level_intrinsics(K, level):
    s = float(1 << level)
    fx, fy, cx, cy = (float(k) for k in K)
    return np.array([fx / s, fy / s, (cx + 0.5) / s - 0.5, (cy + 0.5) / s - 0.5])


def associate(src, model, K, A, R0, trunc):
    """-> (valid count, dict of inlier arrays: pc [N,3] source camera points, q [N,3] model vertices, n [N,3] model normals, all
    anchor / source camera frame, float64; and what a photometric term needs: the source pixel (u, v), the model pixel (ui, vi) and
    the projection's offsets from it (dx, dy) = (x' - u', y' - v')).  model = (depth [h,w], world normal [h,w,3], mask [h,w], ...)."""
    mdepth, mnormal, mmask = model[:3]
    h, w = src.shape
    fx, fy, cx, cy = (float(k) for k in K)
    v, u = np.nonzero(src > 0)
    valid = len(u)
    d = src[v, u].astype(np.float64)
    pc = np.stack([d * ((u - cx) / fx), d * ((v - cy) / fy), d], axis=1)
    p = np.stack(transform(A, pc[:, 0], pc[:, 1], pc[:, 2]), axis=1)
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


def transform(A, x, y, z):
    return [A[r, 0] * x + A[r, 1] * y + A[r, 2] * z + A[r, 3] for r in range(3)]


def residuals(A, pc, q, n):
    """r = n . (A pc - q) and J = [p x n, n] of fixed associations."""
    p = np.stack(transform(A, pc[:, 0], pc[:, 1], pc[:, 2]), axis=1)
    e = p - q
    r = n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1] + n[:, 2] * e[:, 2]
    J = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0],
                  n[:, 0], n[:, 1], n[:, 2]], axis=1)
    return r, J


def huber(r, delta):
    a = np.abs(r)
    with np.errstate(divide="ignore"):
        return np.where(a <= delta, 1.0, delta / a)


def _sums(w, J, r):
    """One term's sums and the sums of their absolute values, each [6,7] upper triangular: [a,b] = sum (w J_a) J_b for a <= b < 6,
    [a,6] = sum (w J_a) r - every element the kernel's float64 product."""
    S, S_abs = np.zeros((6, 7)), np.zeros((6, 7))
    for a in range(6):
        wa = w * J[:, a]
        for b in range(a, 7):
            t = wa * (J[:, b] if b < 6 else r)
            S[a, b], S_abs[a, b] = t.sum(), np.abs(t).sum()
    return S, S_abs


def linearise(src, model, K, A, R0, trunc, delta, photometric=None):
    """-> dict(H 6x6, g 6, sq_error, inliers, valid, H_abs, g_abs).  H_abs and g_abs are the sums of the terms' absolute values
    (sq_error is its own), the scale of a summation error bound.  photometric(A, inliers of associate) -> (r_I, J_I, w_I) of the
    inliers that have a photometric term: H, g and their _abs are then those of the combined system, each the geometric sum plus
    the photometric sum, and the dict also holds photometric_inliers and sq_intensity_error."""
    valid, a = associate(src, model, K, A, R0, trunc)
    r, J = residuals(A, a["pc"], a["q"], a["n"])
    S, S_abs = _sums(huber(r, delta), J, r)
    lin = {"sq_error": float((r * r).sum()), "inliers": len(r), "valid": valid}
    if photometric is not None:
        rI, JI, wI = photometric(A, a)
        SI, SI_abs = _sums(wI, JI, rI)
        S, S_abs = S + SI, S_abs + SI_abs
        lin.update(photometric_inliers=len(rI), sq_intensity_error=float((rI * rI).sum()))
    low = np.tril_indices(6, -1)
    for name, M in (("", S), ("_abs", S_abs)):
        H = M[:, :6].copy()
        H[low] = H.T[low]
        lin.update({"H" + name: H, "g" + name: M[:, 6].copy()})
    return lin


def pivots(H):
    """-> the Cholesky pivots d_j of H as the kernel computes them, up to and including the first that is not positive."""
    L = np.zeros((6, 6))
    out = []
    for j in range(6):
        d = H[j, j]
        for q in range(j):
            d -= L[j, q] * L[j, q]
        out.append(float(d))
        if not d > 0.0:
            break
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            e = H[i, j]
            for q in range(j):
                e -= L[i, q] * L[j, q]
            L[i, j] = e / L[j, j]
    return out


def solve(H, g, inliers):
    """Cholesky as the kernel does it -> (xi, degenerate)."""
    if inliers < MIN_INLIERS:
        return np.zeros(6), True
    tr = float(np.trace(H))
    L = np.zeros((6, 6))
    for j in range(6):
        d = H[j, j]
        for q in range(j):
            d -= L[j, q] * L[j, q]
        if not d > PIVOT_REL * tr:
            return np.zeros(6), True
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            e = H[i, j]
            for q in range(j):
                e -= L[i, q] * L[j, q]
            L[i, j] = e / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        e = -g[i]
        for q in range(i):
            e -= L[i, q] * y[q]
        y[i] = e / L[i, i]
    xi = np.zeros(6)
    for i in range(5, -1, -1):
        e = y[i]
        for q in range(i + 1, 6):
            e -= L[q, i] * xi[q]
        xi[i] = e / L[i, i]
    return xi, False


def exp_twist(xi):
    """[Rodrigues(omega), t] as a 4x4."""
    w = np.asarray(xi[:3], np.float64)
    th = float(np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]))
    sa = 1.0 if th < 1e-8 else np.sin(th) / th
    sb = 0.5 if th < 1e-8 else (1.0 - np.cos(th)) / (th * th)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + sa * K + sb * (K @ K)
    E[:3, 3] = xi[3:]
    return E


def converged(xi):
    """|omega| + |t| < CONVERGED, both norms as the kernel forms them."""
    x = [float(v) for v in xi]
    return float(np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) + np.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5])) < CONVERGED


def track(depth, K, T_init, model, iterations=(10, 5, 4), depth_scale=1.0, depth_min=0.1, depth_max=3.0, trunc=0.07, delta=0.05,
          photometric=None):
    """The whole call.  model(level, K_level, h, w) -> (depth, world normal, mask, ...) of the map cast at T_init.  A hybrid call
    gives photometric(level, K_level, maps) -> the level's term for linearise.
    -> dict(T_cw, fitness, inlier_rmse, information, success, iterations, degenerate, inliers, valid, trace) and, hybrid,
    photometric_inliers and intensity_rmse."""
    nl = len(iterations)
    srcs = pyramid(depth, nl, depth_scale, depth_min, depth_max, trunc)
    T_init = np.asarray(T_init, np.float64)
    R0 = T_init[:3, :3]
    A = np.eye(4)
    trace, iters, degenerate, last = [], [0] * nl, 0, None
    for level in range(nl - 1, -1, -1):
        if iterations[level] == 0:
            continue
        Kl = level_intrinsics(K, level)
        h, w = srcs[level].shape
        maps = model(level, Kl, h, w)
        term = photometric(level, Kl, maps) if photometric else None
        for it in range(iterations[level]):
            lin = linearise(srcs[level], maps, Kl, A, R0, trunc, delta, term)
            xi, deg = solve(lin["H"], lin["g"], lin["inliers"])
            row = dict(lin, level=level, iteration=it, A=A.copy(), xi=xi)
            iters[level] += 1
            if level == 0:
                last = lin
            if deg:
                row["status"] = 2
                trace.append(row)
                degenerate |= 1 << level
                break
            A = exp_twist(xi) @ A
            row["status"] = 1 if converged(xi) else 0
            trace.append(row)
            if row["status"] == 1:
                break
    inl, val = last["inliers"], last["valid"]
    out = {"T_cw": rigid_inverse(A) @ T_init, "fitness": inl / val if val else 0.0,
           "inlier_rmse": float(np.sqrt(last["sq_error"] / inl)) if inl else 0.0, "information": last["H"],
           "success": not (degenerate & 1) and inl >= MIN_INLIERS, "iterations": tuple(iters), "degenerate": degenerate,
           "inliers": inl, "valid": val, "trace": trace}
    if photometric:
        pin = last["photometric_inliers"]
        out.update(photometric_inliers=pin, intensity_rmse=float(np.sqrt(last["sq_intensity_error"] / pin)) if pin else 0.0)
    return out


EPS = 2.0 ** -53  # unit roundoff of float64
XI_REL = 1e-12     # the solve of the same H, g: the same correctly rounded operations in the same order on both sides
A_REL = 1e-13      # exp(xi) A: sin / cos of two libms and the order of a 4-term product


def rigid_inverse(A):
    Ai = np.eye(4)
    Ai[:3, :3] = A[:3, :3].T
    Ai[:3, 3] = -A[:3, :3].T @ A[:3, 3]
    return Ai


def pivot_near_threshold(H):
    """True when a Cholesky pivot that decides the degenerate flag lies within rounding of PIVOT_REL * trace(H)."""
    thr = PIVOT_REL * float(np.trace(H))
    tol = 64.0 * EPS * float(np.abs(np.diag(H)).sum())
    for d in pivots(H):
        if abs(d - thr) <= tol:
            return True
        if not d > thr:
            return False
    return False


def check_call(out, depth, K, T_init, model, iterations, depth_scale=1.0, depth_min=0.1, depth_max=3.0, trunc=0.07, delta=0.05,
               photometric=None):
    """Hold one traced hv_tsdf_track or (photometric given, as for track) hv_tsdf_track_color result (an OdometryResult with trace)
    to this restatement, step by step.

    model(level, K_level, h, w) -> (depth, world normal, mask, ...) of the map cast at T_init with the call's depth_min, depth_max
    and weight_threshold (in the GPU tests: the public ray_cast, i.e. the same kernel the call uses).  Every traced row is
    linearised here at the row's own state A.  Per pixel both sides do the same IEEE operations, so:
      - valid, inliers and (hybrid) photometric_inliers are equal;
      - H, g and the squared error differ only by the order of their float64 sums: |gpu - ref| <= 2 (n + 2) 2^-53 S element by
        element, n the number of terms in the sum and S the sum of the terms' absolute values (each order errs by at most
        ~n 2^-53 S; one pixel contributes ~S / n, so one lost, doubled or mis-weighted pixel fails it).  n is the inliers for the
        squared error and for a depth-only H and g, inliers + photometric inliers for the H and g of a hybrid call's combined
        system, and the photometric inliers for the squared intensity error;
      - the row's H, g solved here give its xi and its degenerate decision (a pivot within rounding of the threshold is
        reported in the result instead), status 1 iff converged(xi), and the next row's A is exp(xi) A, or A after status 2.
    Then the schedule (coarse to fine, levels with 0 iterations absent, iterations from 0, a level ends at its first non-zero
    status or its cap) and the outputs (iterations, degenerate bits, success, information, fitness, inlier_rmse, T_cw; hybrid:
    photometric_inliers and intensity_rmse from the last row).
    -> dict(rows, near_pivot [(row, level, iteration)], xi_rel: the largest relative xi difference)."""
    nl = len(iterations)
    T_init = np.asarray(T_init, np.float64)
    R0 = T_init[:3, :3]
    srcs = pyramid(depth, nl, depth_scale, depth_min, depth_max, trunc)
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
            assert np.abs(row["A"] - A_next).max() <= A_REL * max(1.0, np.abs(A_next).max()), (what, row["A"], A_next)
        if level not in maps:
            Kl = level_intrinsics(K, level)
            h, w = srcs[level].shape
            m = model(level, Kl, h, w)
            maps[level] = (Kl, m, photometric(level, Kl, m) if photometric else None)
        Kl, m, term = maps[level]
        ref = linearise(srcs[level], m, Kl, row["A"], R0, trunc, delta, term)
        assert row["valid"] == ref["valid"], (what, "valid", row["valid"], ref["valid"])
        assert row["inliers"] == ref["inliers"], (what, "inliers", row["inliers"], ref["inliers"])
        pin = 0
        if photometric:
            pin = ref["photometric_inliers"]
            assert row["photometric_inliers"] == pin, (what, "photometric inliers", row["photometric_inliers"], pin)
            bar_i = 2.0 * (pin + 2) * EPS
            assert abs(row["sq_intensity_error"] - ref["sq_intensity_error"]) <= bar_i * ref["sq_intensity_error"], (
                what, "e_I", row["sq_intensity_error"], ref["sq_intensity_error"])
        bar = 2.0 * (ref["inliers"] + pin + 2) * EPS
        dH = np.abs(row["H"] - ref["H"])
        assert (dH <= bar * ref["H_abs"]).all(), (what, "H", float((dH / np.maximum(ref["H_abs"], 1e-300)).max()), bar)
        dg = np.abs(row["g"] - ref["g"])
        assert (dg <= bar * ref["g_abs"]).all(), (what, "g", float((dg / np.maximum(ref["g_abs"], 1e-300)).max()), bar)
        bar_e = 2.0 * (ref["inliers"] + 2) * EPS
        assert abs(row["sq_error"] - ref["sq_error"]) <= bar_e * ref["sq_error"], (what, "e", row["sq_error"], ref["sq_error"])

        xi_ref, deg_ref = solve(row["H"], row["g"], row["inliers"])
        if row["inliers"] >= MIN_INLIERS and pivot_near_threshold(row["H"]):
            near.append(what)
        else:
            assert (row["status"] == 2) == deg_ref, (what, "degenerate decision", row["status"], pivots(row["H"]))
        if row["status"] == 2:
            assert not row["xi"].any(), what
            A_next = row["A"]
        else:
            if not deg_ref:
                scale = np.abs(xi_ref).max()
                rel = float(np.abs(row["xi"] - xi_ref).max() / scale) if scale > 0 else float(np.abs(row["xi"]).max())
                xi_rel = max(xi_rel, rel)
                assert rel <= XI_REL, (what, "xi", row["xi"], xi_ref)
            assert (row["status"] == 1) == converged(row["xi"]), (what, row["status"], row["xi"])
            A_next = exp_twist(row["xi"]) @ row["A"]

    # outputs
    last = rows[-1]
    assert last["level"] == 0
    inl, val = last["inliers"], last["valid"]
    assert out.success == (last["status"] != 2 and inl >= MIN_INLIERS), (out.success, last["status"], inl)
    assert np.array_equal(out.information, last["H"])
    assert out.inliers == inl and out.valid == val
    assert out.fitness == (inl / val if val else 0.0), (out.fitness, inl, val)
    assert out.inlier_rmse == (float(np.sqrt(last["sq_error"] / inl)) if inl else 0.0), (out.inlier_rmse, last["sq_error"], inl)
    if photometric:
        pin = last["photometric_inliers"]
        assert out.photometric_inliers == pin, (out.photometric_inliers, pin)
        assert out.intensity_rmse == (float(np.sqrt(last["sq_intensity_error"] / pin)) if pin else 0.0), (
            out.intensity_rmse, last["sq_intensity_error"], pin)
    T_exp = rigid_inverse(A_next) @ T_init
    assert np.abs(out.transformation - T_exp).max() <= 1e-12 * (1.0 + np.abs(T_init).max()), (out.transformation, T_exp)
    return {"rows": len(rows), "near_pivot": near, "xi_rel": xi_rel}


def pose_error(T_a, T_b):
    """-> (distance between the camera centres in m, rotation angle in deg) of two T_cw."""
    D = np.asarray(T_a, np.float64) @ np.linalg.inv(np.asarray(T_b, np.float64))
    c = np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(D[:3, 3])), float(np.degrees(np.arccos(c)))
