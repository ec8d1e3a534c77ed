"""The numpy restatement of hv_pose_graph_optimize's contract (include/hipvol.h): the same Log, exp, Ad and Jl^-1, the same line
process, Levenberg-Marquardt rule and stopping rules, the same block-Jacobi PCG (sums in numpy's order, not the device's two-stage
order), and a dense numpy.linalg.solve of the damped system as a second, independent inner solver.  Everything per-edge is
vectorised over the edges and takes a dtype, so that the same text evaluates in numpy.longdouble for the measured tolerance."""
import numpy as np

SMALL = 1e-8
NEAR_PI_COS = -0.99
JINV_SERIES = 0.05
GRADIENT, STEP, DECREASE, RESIDUAL = 1, 2, 3, 4

DEFAULTS = dict(line_process_weight=1.0, edge_prune_threshold=0.25, lambda_scale=1e-5, gradient_tolerance=1e-6, step_tolerance=1e-6,
                decrease_tolerance=1e-6, residual_tolerance=1e-6, cg_tolerance=1e-8, max_iterations=100, cg_max_iterations=100, fixed=0)


def hat(w):
    """[..., 3] -> [..., 3, 3]"""
    z = np.zeros_like(w[..., 0])
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1), np.stack([w[..., 2], z, -w[..., 0]], -1),
                     np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def exp(xi):
    """[..., 6] (omega, t) -> [..., 4, 4]: Rodrigues rotation, plain translation part."""
    xi = np.asarray(xi)
    w, t = xi[..., :3], xi[..., 3:]
    th = np.sqrt((w * w).sum(-1))
    small = th < SMALL
    ths = np.where(small, 1, th)
    a = np.where(small, 1, np.sin(ths) / ths)[..., None, None]
    b = np.where(small, 0.5, (1 - np.cos(ths)) / (ths * ths))[..., None, None]
    K = hat(w)
    T = np.zeros(xi.shape[:-1] + (4, 4), xi.dtype)
    T[..., :3, :3] = np.eye(3, dtype=xi.dtype) + a * K + b * (K @ K)
    T[..., :3, 3] = t
    T[..., 3, 3] = 1
    return T


def log_rot(R):
    """[..., 3, 3] -> [..., 3], the three branches of the contract."""
    R = np.asarray(R)
    one = R.dtype.type(1)
    v = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1) / 2
    s = np.sqrt((v * v).sum(-1))
    c = (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1) / 2
    th = np.arctan2(s, c)
    small = s < SMALL
    w = v * np.where(small, one, th / np.where(small, one, s))[..., None]
    near = c < NEAR_PI_COS
    if np.any(near):
        I = np.eye(3, dtype=R.dtype)
        cn = np.where(near, c, 0)
        A = ((R + np.swapaxes(R, -1, -2)) / 2 - cn[..., None, None] * I) / (1 - cn)[..., None, None]
        d = np.stack([A[..., 0, 0], A[..., 1, 1], A[..., 2, 2]], -1)
        k = np.argmax(d, -1)
        row = np.take_along_axis(A, k[..., None, None], -2)[..., 0, :]
        dk = np.take_along_axis(d, k[..., None], -1)
        a = row / np.sqrt(np.where(near[..., None], dk, one))
        n = np.sqrt((a * a).sum(-1))
        sg = np.where((a * v).sum(-1) < 0, -one, one)
        w = np.where(near[..., None], a * (sg * th / np.where(near, n, one))[..., None], w)
    return w


def log(T):
    """[..., 4, 4] -> [..., 6] = (Log R, t): inverts exp."""
    T = np.asarray(T)
    return np.concatenate([log_rot(T[..., :3, :3]), T[..., :3, 3]], -1)


def inv(T):
    """The rigid inverse [R^T, -R^T t]."""
    T = np.asarray(T)
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:])[..., 0]
    out[..., 3, 3] = 1
    return out


def adjoint(A):
    """Ad of [Ra, ta] in the (omega, t) order: [[Ra, 0], [[ta]x Ra, Ra]]."""
    A = np.asarray(A)
    Ra, ta = A[..., :3, :3], A[..., :3, 3]
    out = np.zeros(A.shape[:-2] + (6, 6), A.dtype)
    out[..., :3, :3] = Ra
    out[..., 3:, :3] = hat(ta) @ Ra
    out[..., 3:, 3:] = Ra
    return out


def jl_inv(r):
    """Jl^-1(r) = [[Jw(omega), 0], [-[t]x, I]], closed form, the coefficient's series below JINV_SERIES."""
    r = np.asarray(r)
    w, t = r[..., :3], r[..., 3:]
    th2 = (w * w).sum(-1)
    th = np.sqrt(th2)
    ser = th < JINV_SERIES
    ths = np.where(ser, 1, th)
    c2 = np.where(ser, r.dtype.type(1) / 12 + th2 * (r.dtype.type(1) / 720 + th2 * (r.dtype.type(1) / 30240)),
                  1 / (ths * ths) - np.cos(ths / 2) / (2 * ths * np.sin(ths / 2)))
    K = hat(w)
    out = np.zeros(r.shape[:-1] + (6, 6), r.dtype)
    out[..., :3, :3] = np.eye(3, dtype=r.dtype) - K / 2 + c2[..., None, None] * (K @ K)
    out[..., 3:, :3] = -hat(t)
    out[..., 3:, 3:] = np.eye(3, dtype=r.dtype)
    return out


def residual(poses, nodes, Z):
    """r [E,6] = Log(inv(T_t) T_s inv(Z))"""
    return log(inv(poses[nodes[:, 1]]) @ poses[nodes[:, 0]] @ inv(Z))


def line_process(chi2, uncertain, mu):
    q = mu / (mu + chi2)
    return np.where(uncertain, q * q, chi2.dtype.type(1))


def linearise(poses, nodes, Z, info, uncertain, mu, dtype=np.float64):
    """-> dict r [E,6], chi2 [E], l [E], J [E,6,6] (= J_s; J_t = -J_s), M [E,6,6], g [E,6], F."""
    poses, Z, info = (np.asarray(a, dtype).reshape(-1, s, s) for a, s in ((poses, 4), (Z, 4), (info, 6)))
    nodes = np.asarray(nodes).reshape(-1, 2)
    unc = np.zeros(len(nodes), bool) if uncertain is None else np.asarray(uncertain).astype(bool)
    mu = dtype(mu)
    A = inv(poses[nodes[:, 1]])
    r = log(A @ poses[nodes[:, 0]] @ inv(Z))
    Or = (info @ r[..., None])[..., 0]
    chi2 = (r * Or).sum(-1)
    l = line_process(chi2, unc, mu)
    J = jl_inv(r) @ adjoint(A)
    Jt = np.swapaxes(J, -1, -2)
    M = l[:, None, None] * (Jt @ (info @ J))
    g = l[:, None] * (Jt @ Or[..., None])[..., 0]
    cost = np.where(unc, l * chi2 + mu * (np.sqrt(l) - 1) ** 2, chi2)
    return dict(r=r, chi2=chi2, l=l, J=J, M=M, g=g, F=cost.sum())


def objective(poses, nodes, Z, info, uncertain, mu):
    poses, Z, info = (np.asarray(a, np.float64).reshape(-1, s, s) for a, s in ((poses, 4), (Z, 4), (info, 6)))
    unc = np.zeros(len(nodes), bool) if uncertain is None else np.asarray(uncertain).astype(bool)
    r = residual(poses, np.asarray(nodes).reshape(-1, 2), Z)
    chi2 = (r * (info @ r[..., None])[..., 0]).sum(-1)
    l = line_process(chi2, unc, mu)
    return np.where(unc, l * chi2 + mu * (np.sqrt(l) - 1) ** 2, chi2).sum(), l


def gradient(lin, nodes, N, fixed=None):
    """b [N,6]: +g_e at the source, -g_e at the target, in the order of the edge index; 0 at the fixed node."""
    b = np.zeros((N, 6), lin["g"].dtype)
    np.add.at(b, nodes[:, 0], lin["g"])
    np.add.at(b, nodes[:, 1], -lin["g"])
    if fixed is not None:
        b[fixed] = 0
    return b


def diagonal_blocks(lin, nodes, N):
    D = np.zeros((N, 6, 6))
    np.add.at(D, nodes[:, 0], lin["M"])
    np.add.at(D, nodes[:, 1], lin["M"])
    return D


def product(lin, nodes, x, lam, fixed):
    """(H + lambda I) x without the matrix: u_e = M_e (x_s - x_t), +u_e to s, -u_e to t; the fixed node's row is 0."""
    u = (lin["M"] @ (x[nodes[:, 0]] - x[nodes[:, 1]])[..., None])[..., 0]
    q = lam * x
    np.add.at(q, nodes[:, 0], u)
    np.add.at(q, nodes[:, 1], -u)
    q[fixed] = 0
    return q


def solve_pcg(lin, nodes, b, D, lam, fixed, cg_tolerance, cg_max_iterations):
    """-> (d [N,6], iterations, residual): block-Jacobi PCG from 0 on (H + lambda I) d = -b over the free nodes."""
    N = len(b)
    P = D + lam * np.eye(6)
    P[fixed] = np.eye(6)
    Lc = np.linalg.cholesky(P)

    def precond(r):
        y = np.linalg.solve(Lc, r[..., None])
        z = np.linalg.solve(np.swapaxes(Lc, -1, -2), y)[..., 0]
        z[fixed] = 0
        return z

    x = np.zeros((N, 6))
    r = -b.copy()
    z = precond(r)
    rz = (r * z).sum()
    rz0, p, its, res = rz, None, 0, 0.0
    for j in range(cg_max_iterations):
        res = np.sqrt(rz / rz0) if rz0 > 0 else 0.0
        if not rz > cg_tolerance ** 2 * rz0:
            break
        p = z.copy() if j == 0 else z + (rz / rz_prev) * p
        its = j + 1
        q = product(lin, nodes, p, lam, fixed)
        pq = (p * q).sum()
        alpha = rz / pq if pq > 0 else 0.0
        x += alpha * p
        r -= alpha * q
        z = precond(r)
        rz_prev, rz = rz, (r * z).sum()
    return x, its, res


def dense_system(lin, nodes, N):
    H = np.zeros((N, 6, N, 6))
    for e, (s, t) in enumerate(nodes):
        M = lin["M"][e]
        H[s, :, s, :] += M
        H[t, :, t, :] += M
        H[s, :, t, :] -= M
        H[t, :, s, :] -= M
    return H.reshape(6 * N, 6 * N)


def solve_dense(lin, nodes, b, D, lam, fixed, cg_tolerance=None, cg_max_iterations=None):
    N = len(b)
    H = dense_system(lin, nodes, N) + lam * np.eye(6 * N)
    free = np.ones(6 * N, bool)
    free[6 * fixed:6 * fixed + 6] = False
    d = np.zeros(6 * N)
    d[free] = np.linalg.solve(H[np.ix_(free, free)], -b.reshape(-1)[free])
    return d.reshape(N, 6), 0, 0.0


def step(poses, nodes, Z, info, uncertain, lam, nu, first, params, solver=solve_pcg):
    """One outer iteration from `poses` [N,4,4] with the damping state (lam, nu): -> (new poses, new lam, new nu, row) where row holds
    what the call's trace row holds plus the linearisation."""
    P = {**DEFAULTS, **params}
    mu, fixed = P["line_process_weight"], P["fixed"]
    N = len(poses)
    lin = linearise(poses, nodes, Z, info, uncertain, mu)
    b = gradient(lin, nodes, N, fixed)
    D = diagonal_blocks(lin, nodes, N)
    if first:
        free = np.arange(N) != fixed
        lam = P["lambda_scale"] * max(0.0, D[free][:, range(6), range(6)].max()) if free.any() else 0.0
    d, cg_its, cg_res = solver(lin, nodes, b, D, lam, fixed, P["cg_tolerance"], P["cg_max_iterations"])
    trial = exp(d) @ poses
    F = lin["F"]
    Fn, _ = objective(trial, nodes, Z, info, uncertain, mu)
    pred = (d * (lam * d - b)).sum()
    rho = (F - Fn) / pred if (pred > 0 and Fn == Fn) else 0.0
    grad, stepn = np.abs(b).max(), np.sqrt((d * d).sum())
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
               lam_new=lam_new, converged=conv, lin=lin, b=b)
    return (trial if accepted else poses), lam_new, nu_new, row


def optimize(poses, nodes, Z, info, uncertain=None, solver=solve_pcg, **params):
    """The whole call: -> dict poses [N,4,4], l [E], kept [E], chi2_initial, chi2_final, lam, iterations, cg_iterations_total,
    converged, success, trace (the rows of step())."""
    P = {**DEFAULTS, **params}
    poses = np.array(poses, np.float64).reshape(-1, 4, 4)
    nodes = np.asarray(nodes, np.int64).reshape(-1, 2)
    Z = np.asarray(Z, np.float64).reshape(-1, 4, 4)
    info = np.asarray(info, np.float64).reshape(-1, 6, 6)
    if len(nodes) == 0:
        return dict(poses=poses, l=np.zeros(0), kept=np.zeros(0, bool), chi2_initial=0.0, chi2_final=0.0, lam=0.0, iterations=0,
                    cg_iterations_total=0, converged=GRADIENT, success=True, trace=[])
    lam, nu, trace, conv = 0.0, 2.0, [], 0
    for it in range(P["max_iterations"]):
        poses, lam, nu, row = step(poses, nodes, Z, info, uncertain, lam, nu, it == 0, P, solver)
        trace.append(row)
        conv = row["converged"]
        if conv:
            break
    Ff, l = objective(poses, nodes, Z, info, uncertain, P["line_process_weight"])
    last = trace[-1]
    return dict(poses=poses, l=l, kept=l >= P["edge_prune_threshold"], chi2_initial=trace[0]["F"],
                chi2_final=last["F_trial"] if last["accepted"] else last["F"], lam=lam, iterations=len(trace),
                cg_iterations_total=sum(r["cg_iterations"] for r in trace), converged=conv, success=conv != 0 and np.isfinite(Ff), trace=trace)


def scales(lin_ld, nodes, poses, Z, info, mu):
    """What a deviation of each per-edge quantity is measured against: the magnitude the quantity's own rounding error is
    proportional to, from the longdouble evaluation.  s_e = the largest entry of |inv(T_t)| |T_s| |inv(Z)| bounds the entries X is
    computed from; r: max(|r|, s_e); chi2: |Omega| |r|_1 S_r; l: 1 + 2 S_chi / (mu + chi2); M: |J|^2 |Omega| S_l; g: |J| |Omega| S_l S_r;
    the gradient of a node: the sum of S_g over its edges."""
    poses, Z, info = (np.asarray(a, np.float64).reshape(-1, s, s) for a, s in ((poses, 4), (Z, 4), (info, 6)))
    nodes = np.asarray(nodes).reshape(-1, 2)
    f = lambda a: np.asarray(a, np.float64)
    s_e = (np.abs(inv(poses[nodes[:, 1]])) @ np.abs(poses[nodes[:, 0]]) @ np.abs(inv(Z))).max((-1, -2))
    r = f(lin_ld["r"])
    S_r = np.maximum(np.abs(r).max(-1), s_e)
    Om = np.abs(info).max((-1, -2))
    S_chi = Om * np.abs(r).sum(-1) * S_r
    S_l = 1 + 2 * S_chi / (mu + f(lin_ld["chi2"]))
    Jm = np.abs(f(lin_ld["J"])).max((-1, -2))
    S_M = Jm * Jm * Om * S_l
    S_g = Jm * Om * S_l * S_r
    S_b = np.zeros(len(poses))
    np.add.at(S_b, nodes[:, 0], S_g)
    np.add.at(S_b, nodes[:, 1], S_g)
    return dict(r=S_r[:, None], chi2=S_chi, l=S_l, M=S_M[:, None, None], g=S_g[:, None], b=S_b[:, None])


def deviation(got, want_ld, S):
    """The largest |got - want| / scale over the per-edge quantities r, chi2, l, M, g and the gradient b, by name."""
    out = {}
    for k in ("r", "chi2", "l", "M", "g", "b"):
        if k in got and got[k] is not None:
            sc = np.where(S[k] > 0, S[k], 1.0)
            out[k] = float(np.max(np.abs(np.asarray(got[k], np.longdouble) - want_ld[k]) / sc))
    return out
