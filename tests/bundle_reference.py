"""The numpy restatement of hv_bundle_adjust's contract (include/hipvol.h, rules B1-B8): the same projection, Huber weight, depth rule,
updates, Levenberg-Marquardt rule and stopping rules as the pose graph's restatement, the Schur-complement PCG over the free cameras
(sums in numpy's order, not the device's), and a dense numpy.linalg.solve of the FULL damped system over cameras and points as a
second, independent inner solver.  The Jacobians are written out per observation (J_camera = J W, J_point = J R) and the blocks are
products of them: the library keeps A = w s J^T J and q instead.  Everything per observation is vectorised and takes a dtype, so that
the same text evaluates in numpy.longdouble for the measured tolerance."""
import numpy as np

from tests.pose_graph_reference import DECREASE, GRADIENT, RESIDUAL, STEP, exp, hat  # noqa: F401  (B5 and B6: the pose graph's own)

DEFAULTS = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, bf=1.0, huber_delta2_mono=5.991, huber_delta2_stereo=7.815, min_depth=1e-6,
                lambda_scale=1e-5, gradient_tolerance=1e-6, step_tolerance=1e-6, decrease_tolerance=1e-6, residual_tolerance=1e-6,
                cg_tolerance=1e-8, max_iterations=100, cg_max_iterations=100, huber=True, fixed_points=False)


def linearise(cams, pts, idx, meas, active, P, dtype=np.float64):
    """One evaluation at (cams [N,4,4], pts [M,3]) of the observations idx [O,2], meas [O,4], active [O] bool.  -> dict q [O,3], r [O,3],
    chi2, w, rho [O], on [O] (active and in front), low [O] (active with q_z <= min_depth), Jc [O,3,6], Jp [O,3,3], ws [O], F."""
    cams, pts, meas = np.asarray(cams, dtype).reshape(-1, 4, 4), np.asarray(pts, dtype).reshape(-1, 3), np.asarray(meas, dtype).reshape(-1, 4)
    idx = np.asarray(idx).reshape(-1, 2)
    active = np.asarray(active, bool)
    f, P = dtype, {**DEFAULTS, **P}
    fx, fy, cx, cy, bf = (f(P[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    T = cams[idx[:, 0]]
    R = T[:, :3, :3]
    q = (R @ pts[idx[:, 1]][..., None])[..., 0] + T[:, :3, 3]
    low = active & ~(q[:, 2] > f(P["min_depth"]))
    on = active & ~low
    q = np.where(on[:, None], q, f(0))
    z = np.where(on, q[:, 2], f(1))
    iz = 1 / z
    xz, yz = q[:, 0] * iz, q[:, 1] * iz
    stereo = np.isfinite(np.asarray(meas[:, 2], np.float64))
    ur = np.where(stereo, meas[:, 2], f(0))
    pu = fx * xz + cx
    r = np.stack([meas[:, 0] - pu, meas[:, 1] - (fy * yz + cy), np.where(stereo, ur - (pu - bf * iz), f(0))], -1)
    r = np.where(on[:, None], r, f(0))
    s = meas[:, 3]
    chi2 = np.where(on, s * (r * r).sum(-1), f(0))
    d2 = np.where(stereo, f(P["huber_delta2_stereo"]), f(P["huber_delta2_mono"]))
    out = bool(P["huber"]) & (chi2 > d2)
    sq = np.sqrt(np.where(out, chi2, f(1)))
    w = np.where(on, np.where(out, np.sqrt(d2) / sq, f(1)), f(0))
    rho = np.where(out, 2 * np.sqrt(d2) * sq - d2, chi2)
    zero = np.zeros_like(iz)
    J = np.stack([np.stack([-fx * iz, zero, fx * xz * iz], -1), np.stack([zero, -fy * iz, fy * yz * iz], -1),
                  np.where(stereo[:, None], np.stack([-fx * iz, zero, (fx * xz - bf * iz) * iz], -1), f(0))], -2)
    J = np.where(on[:, None, None], J, f(0))
    W = np.concatenate([-hat(q), np.broadcast_to(np.eye(3, dtype=dtype), (len(q), 3, 3))], -1)
    return dict(q=q, r=r, chi2=chi2, w=w, rho=rho, on=on, low=low, J=J, Jc=J @ W, Jp=J @ R, ws=w * s, F=rho[on].sum() if on.any() else f(0))


def blocks(lin, idx, N, M):
    """-> B [N,6,6], bc [N,6], C [M,3,3], bp [M,3], E [O,6,3] in the order of the observation index."""
    Jc, Jp, ws, r = lin["Jc"], lin["Jp"], lin["ws"][:, None, None], lin["r"]
    dt = Jc.dtype
    JcT, JpT = np.swapaxes(Jc, -1, -2), np.swapaxes(Jp, -1, -2)
    B, bc, C, bp = np.zeros((N, 6, 6), dt), np.zeros((N, 6), dt), np.zeros((M, 3, 3), dt), np.zeros((M, 3), dt)
    np.add.at(B, idx[:, 0], ws * (JcT @ Jc))
    np.add.at(C, idx[:, 1], ws * (JpT @ Jp))
    np.add.at(bc, idx[:, 0], (ws * JcT @ r[..., None])[..., 0])
    np.add.at(bp, idx[:, 1], (ws * JpT @ r[..., None])[..., 0])
    return dict(B=B, bc=bc, C=C, bp=bp, E=ws * (JcT @ Jp))


def objective(cams, pts, idx, meas, on, P):
    """F at a trial state for the observations `on`: not-a-number when one of them has q_z <= min_depth (B4)."""
    lin = linearise(cams, pts, idx, meas, on, P)
    return (np.nan if lin["low"].any() else float(lin["F"])), lin


def solve_schur(blk, idx, lam, cam_fixed, points_free, cg_tolerance, cg_max_iterations):
    """-> (dc [N,6], dp [M,3], iterations, residual): PCG from 0 on the reduced camera system, then the back-substitution (B7)."""
    B, bc, C, bp, E = blk["B"], blk["bc"], blk["C"], blk["bp"], blk["E"]
    N, M = len(B), len(C)
    ci, pi = idx[:, 0], idx[:, 1]
    if points_free:
        Ci = np.linalg.inv(C + lam * np.eye(3))
    else:
        Ci, E, bp = np.zeros_like(C), np.zeros_like(E), np.zeros_like(bp)
    ET = np.swapaxes(E, -1, -2)
    wp = (Ci @ bp[..., None])[..., 0]

    def to_points(x):  # (C + lam)^-1 E^T x
        t = np.zeros((M, 3))
        np.add.at(t, pi, (ET @ x[ci][..., None])[..., 0])
        return (Ci @ t[..., None])[..., 0]

    def to_cams(y):  # E y
        a = np.zeros((N, 6))
        np.add.at(a, ci, (E @ y[pi][..., None])[..., 0])
        return a

    def product(x):
        q = (B @ x[..., None])[..., 0] + lam * x - to_cams(to_points(x))
        q[cam_fixed] = 0
        return q

    Sd = B + lam * np.eye(6)
    np.subtract.at(Sd, ci, E @ Ci[pi] @ ET)
    Sd[cam_fixed] = np.eye(6)
    Lc = np.linalg.cholesky(Sd)

    def precond(r):
        y = np.linalg.solve(Lc, r[..., None])
        z = np.linalg.solve(np.swapaxes(Lc, -1, -2), y)[..., 0]
        z[cam_fixed] = 0
        return z

    r = -(bc - to_cams(wp))
    r[cam_fixed] = 0
    x = np.zeros((N, 6))
    z = precond(r)
    rz = (r * z).sum()
    rz0, p, its, res = rz, None, 0, 0.0
    for j in range(cg_max_iterations):
        res = np.sqrt(rz / rz0) if rz0 > 0 else 0.0
        if not rz > cg_tolerance ** 2 * rz0:
            break
        p = z.copy() if j == 0 else z + (rz / rz_prev) * p
        its = j + 1
        q = product(p)
        pq = (p * q).sum()
        alpha = rz / pq if pq > 0 else 0.0
        x += alpha * p
        r -= alpha * q
        z = precond(r)
        rz_prev, rz = rz, (r * z).sum()
    return x, -(wp + to_points(x)), its, res


def dense_system(blk, idx):
    """The full H over (cameras, points), [6 N + 3 M] square."""
    N, M = len(blk["B"]), len(blk["C"])
    H = np.zeros((6 * N + 3 * M, 6 * N + 3 * M))
    for i in range(N):
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = blk["B"][i]
    for j in range(M):
        H[6 * N + 3 * j:6 * N + 3 * j + 3, 6 * N + 3 * j:6 * N + 3 * j + 3] = blk["C"][j]
    for (c, j), E in zip(idx, blk["E"]):
        H[6 * c:6 * c + 6, 6 * N + 3 * j:6 * N + 3 * j + 3] += E
        H[6 * N + 3 * j:6 * N + 3 * j + 3, 6 * c:6 * c + 6] += E.T
    return H


def solve_dense(blk, idx, lam, cam_fixed, points_free, cg_tolerance=None, cg_max_iterations=None):
    N, M = len(blk["B"]), len(blk["C"])
    H = dense_system(blk, idx) + lam * np.eye(6 * N + 3 * M)
    b = np.concatenate([blk["bc"].reshape(-1), blk["bp"].reshape(-1)])
    free = np.concatenate([np.repeat(~np.asarray(cam_fixed, bool), 6), np.full(3 * M, bool(points_free))])
    d = np.zeros(len(b))
    if free.any():
        d[free] = np.linalg.solve(H[np.ix_(free, free)], -b[free])
    return d[:6 * N].reshape(N, 6), d[6 * N:].reshape(M, 3), 0, 0.0


def step(cams, pts, idx, meas, on, cam_fixed, lam, nu, first, params, solver=solve_schur):
    """One outer iteration from (cams, pts) with the damping state (lam, nu) and the observations `on` (at the first iteration the
    caller's active flags: those behind are switched off here): -> (cams, pts, on, lam, nu, row)."""
    P = {**DEFAULTS, **params}
    N, M = len(cams), len(pts)
    pf = not P["fixed_points"]
    lin = linearise(cams, pts, idx, meas, on, P)
    behind = lin["low"] if first else np.zeros(len(idx), bool)
    on = lin["on"]
    blk = blocks(lin, idx, N, M)
    blk["bc"][cam_fixed] = 0
    if not pf:
        blk["bp"][:] = 0
    if first:
        diag = [blk["B"][~cam_fixed][:, range(6), range(6)].reshape(-1)]
        if pf:
            diag.append(blk["C"][:, range(3), range(3)].reshape(-1))
        diag = np.concatenate(diag)
        lam = P["lambda_scale"] * max(0.0, diag.max()) if len(diag) else 0.0
    dc, dp, cg_its, cg_res = solver(blk, idx, lam, cam_fixed, pf, P["cg_tolerance"], P["cg_max_iterations"])
    tc, tp = exp(dc) @ cams, pts + dp
    F = float(lin["F"])
    Fn, _ = objective(tc, tp, idx, meas, on, P)
    pred = (dc * (lam * dc - blk["bc"])).sum() + (dp * (lam * dp - blk["bp"])).sum()
    rho = (F - Fn) / pred if (pred > 0 and Fn == Fn) else 0.0
    grad = max(np.abs(blk["bc"]).max(), np.abs(blk["bp"]).max())
    stepn = np.sqrt((dc * dc).sum() + (dp * dp).sum())
    conv, accepted, lam_new, nu_new = 0, False, lam, nu
    if F <= P["residual_tolerance"]:
        conv = RESIDUAL
    elif grad <= P["gradient_tolerance"]:
        conv = GRADIENT
    else:
        accepted = rho > 0
        if accepted:
            lam_new, nu_new = lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 2.0
        else:
            lam_new, nu_new = lam * nu, 2.0 * nu
        if stepn <= P["step_tolerance"]:
            conv = STEP
        elif accepted and (F - Fn) <= P["decrease_tolerance"] * F:
            conv = DECREASE
    row = dict(lam=lam, F=F, F_trial=Fn, rho=rho, accepted=bool(accepted), cg_iterations=cg_its, cg_residual=cg_res, step=stepn, gradient=grad,
               lam_new=lam_new, converged=conv, lin=lin, blk=blk, behind=behind, on=on, dc=dc, dp=dp, pred=pred)
    return (tc if accepted else cams), (tp if accepted else pts), on, lam_new, nu_new, row


def optimize(cams, pts, idx, meas, active=None, cam_fixed=None, solver=solve_schur, **params):
    """The whole call: -> dict cameras, points, chi2 [O], behind [O], inlier [O], chi2_initial, chi2_final, lam, iterations,
    cg_iterations_total, converged, success, trace (the rows of step(), each with the state it started from)."""
    P = {**DEFAULTS, **params}
    cams, pts = np.array(cams, np.float64).reshape(-1, 4, 4), np.array(pts, np.float64).reshape(-1, 3)
    idx, meas = np.asarray(idx, np.int64).reshape(-1, 2), np.asarray(meas, np.float64).reshape(-1, 4)
    O = len(idx)
    on = np.ones(O, bool) if active is None else np.asarray(active, bool).copy()
    cam_fixed = np.zeros(len(cams), bool) if cam_fixed is None else np.asarray(cam_fixed, bool)
    behind = np.zeros(O, bool)
    if not on.any():
        return dict(cameras=cams, points=pts, chi2=np.zeros(O), behind=behind, inlier=np.zeros(O, bool), chi2_initial=0.0, chi2_final=0.0, lam=0.0,
                    iterations=0, cg_iterations_total=0, converged=RESIDUAL, success=True, trace=[])
    lam, nu, trace, conv = 0.0, 2.0, [], 0
    for it in range(P["max_iterations"]):
        c0, p0 = cams, pts
        cams, pts, on, lam, nu, row = step(cams, pts, idx, meas, on, cam_fixed, lam, nu, it == 0, P, solver)
        row["cameras"], row["points"] = c0, p0
        if it == 0:
            behind = row["behind"]
        trace.append(row)
        conv = row["converged"]
        if conv:
            break
    Ff, lin = objective(cams, pts, idx, meas, on, P)
    stereo = np.isfinite(meas[:, 2])
    gate = np.where(stereo, P["huber_delta2_stereo"], P["huber_delta2_mono"])
    last = trace[-1]
    return dict(cameras=cams, points=pts, chi2=lin["chi2"], behind=behind, inlier=on & (lin["chi2"] <= gate), chi2_initial=trace[0]["F"],
                chi2_final=last["F_trial"] if last["accepted"] else last["F"], lam=lam, iterations=len(trace),
                cg_iterations_total=sum(r["cg_iterations"] for r in trace), converged=conv, success=conv != 0 and np.isfinite(Ff), trace=trace)


def scales(lin_ld, blk_ld, cams, pts, idx, meas, P):
    """What a deviation of each quantity is measured against: the magnitude its own rounding error is proportional to, from the
    longdouble evaluation.  r: the pixel magnitudes it is a difference of, max(|u|, |v|, |u_r|, |pi|) (+ the conditioning of the
    division, |q| / q_z); chi2: inv_sigma2 |r|_1 S_r; w: 1 + S_chi / chi2 where the kernel acts; a block: the sum over its
    observations of the magnitude of each term, |J_a| |J_b| ws (1 + S_w); a gradient: the sum of |J| ws S_r."""
    f = lambda a: np.asarray(a, np.float64)
    cams, pts, meas = f(cams).reshape(-1, 4, 4), f(pts).reshape(-1, 3), f(meas).reshape(-1, 4)
    idx = np.asarray(idx).reshape(-1, 2)
    N, M = len(cams), len(pts)
    q, on = f(lin_ld["q"]), lin_ld["on"]
    T = cams[idx[:, 0]]
    qa = (np.abs(T[:, :3, :3]) @ np.abs(pts[idx[:, 1]])[..., None])[..., 0] + np.abs(T[:, :3, 3])
    z = np.where(on, q[:, 2], 1.0)
    cond = 1 + qa.max(-1) / z
    pix = np.maximum(np.abs(np.nan_to_num(meas[:, :3], nan=0.0, posinf=0.0, neginf=0.0)).max(-1),
                     max(abs(P["cx"]), abs(P["cy"])) + max(P["fx"], P["fy"], P["bf"]) * cond)
    r = f(lin_ld["r"])
    S_r = np.maximum(np.abs(r).max(-1), pix * cond)
    S_chi = meas[:, 3] * np.abs(r).sum(-1) * S_r
    chi2 = f(lin_ld["chi2"])
    S_w = np.where(f(lin_ld["w"]) < 1, 1 + S_chi / np.where(chi2 > 0, chi2, 1.0), 1.0)
    ws = f(lin_ld["ws"])
    Jc, Jp = np.abs(f(lin_ld["Jc"])).max((-1, -2)) * cond, np.abs(f(lin_ld["Jp"])).max((-1, -2)) * cond
    S_B, S_C, S_bc, S_bp = np.zeros(N), np.zeros(M), np.zeros(N), np.zeros(M)
    np.add.at(S_B, idx[:, 0], Jc * Jc * ws * S_w)
    np.add.at(S_C, idx[:, 1], Jp * Jp * ws * S_w)
    np.add.at(S_bc, idx[:, 0], Jc * ws * S_w * S_r)
    np.add.at(S_bp, idx[:, 1], Jp * ws * S_w * S_r)
    return dict(r=S_r[:, None], chi2=S_chi, w=S_w, B=S_B[:, None, None], C=S_C[:, None, None], bc=S_bc[:, None], bp=S_bp[:, None])


def deviation(got, want_ld, S):
    """The largest |got - want| / scale over r, chi2, w, B, bc, C, bp, by name."""
    out = {}
    for k in ("r", "chi2", "w", "B", "bc", "C", "bp"):
        if k in got and got[k] is not None:
            sc = np.where(S[k] > 0, S[k], 1.0)
            out[k] = float(np.max(np.abs(np.asarray(got[k], np.longdouble) - want_ld[k]) / sc)) if np.size(got[k]) else 0.0
    return out
