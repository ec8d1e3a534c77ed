"""numpy restatement of map-to-map registration (include/hipvol.h, hv_tsdf_register_volume) on dump() tuples - test
infrastructure, no GPU.

The arithmetic follows the contract operation by operation in float64 (every product and sum its own numpy call), so the decisions
(candidate, valid, inlier, Huber branch) are the library's wherever they do not sit on a boundary of the rules; a candidate that does
- some r_a within 1e-9 of 0 or 1, |rho| within 1e-9 of residual_trunc or huber_delta - is counted as FRAGILE.  The sums are numpy's
(pairwise), the library's are a wave butterfly: they agree to rounding of the additions, which linearise() bounds by returning
sum |term| beside every sum.  Candidates are visited in dump order, not in the library's pool order: the sums do not care.
"""
import collections

import numpy as np

from tests import raycast_reference as rr
from tests.merge_reference import FRAGILE_BAND, _lerp, check_rigid

R = 16
MIN_INLIERS, PIVOT_REL, CONVERGED, TRACE_STRIDE = 6, 1e-10, 1e-6, 54  # the named constants of include/hipvol.h
_LOCAL = np.stack(np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij"), -1).reshape(-1, 3)  # x * 256 + y * 16 + z

Params = collections.namedtuple("Params", "voxel_length sdf_trunc weight_threshold tsdf_band residual_trunc huber_delta")
Lin = collections.namedtuple("Lin", "H g e inliers candidates H_abs g_abs fragile")


def params(voxel_length, sdf_trunc, weight_threshold=3.0, tsdf_band=0.5, residual_trunc=None, huber_delta=None):
    """The defaults of ScalableTSDFVolume.register_volume."""
    return Params(float(voxel_length), float(sdf_trunc), float(weight_threshold), float(tsdf_band),
                  0.5 * float(sdf_trunc) if residual_trunc is None else float(residual_trunc),
                  0.25 * float(sdf_trunc) if huber_delta is None else float(huber_delta))


def check_arguments(T_init, prm, max_iterations):
    """The contract's argument checks -> None or the reason the call is refused."""
    why = check_rigid(T_init)
    if why is not None:
        return why
    if not 1 <= int(max_iterations) <= 10000:
        return "max_iterations"
    if not (np.isfinite(prm.weight_threshold) and prm.weight_threshold >= 0.0):
        return "weight_threshold"
    if not (prm.tsdf_band > 0.0 and prm.tsdf_band <= 1.0):
        return "tsdf_band"
    if not (np.isfinite(prm.residual_trunc) and prm.residual_trunc > 0.0 and np.isfinite(prm.huber_delta) and prm.huber_delta > 0.0):
        return "residual_trunc / huber_delta"
    return None


def candidates(src_dump, prm):
    """-> (global voxel indices [n,3] int64, tsdf_s [n] float32) of the source's candidates, in dump order."""
    keys, tsdf, weight, _ = (np.asarray(x) for x in src_dump)
    keys = keys.reshape(-1, 3).astype(np.int64)
    if len(keys) == 0:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.float32)
    tsdf, weight = tsdf.reshape(len(keys), -1), weight.reshape(len(keys), -1)
    is_c = (weight.astype(np.float64) > prm.weight_threshold) & (np.abs(tsdf.astype(np.float64)) <= prm.tsdf_band)
    u, v = np.nonzero(is_c)
    return keys[u] * R + _LOCAL[v], tsdf[u, v].astype(np.float32)


def anchor(src_dump, T_init, voxel_length):
    """-> (cs, c): the centre of the bounding box of the source's unit keys and where T_init puts it."""
    keys = np.asarray(src_dump[0], np.int64).reshape(-1, 3)
    T = np.asarray(T_init, np.float64)
    cs = ((keys.min(0) + keys.max(0) + 1).astype(np.float64) * 0.5) * (16.0 * np.float64(voxel_length))
    c = np.array([((T[a, 0] * cs[0] + T[a, 1] * cs[1]) + T[a, 2] * cs[2]) + T[a, 3] for a in range(3)])
    return cs, c


class Problem:
    """What stays fixed over the iterations of one call: the candidates, their q, the anchor, the destination's units."""

    def __init__(self, dst_dump, src_dump, T_init, prm):
        T = np.asarray(T_init, np.float64)
        self.prm = prm
        self.grid = rr._Grid(dst_dump) if len(np.asarray(dst_dump[0]).reshape(-1, 3)) else None  # None: the destination is empty
        self.gi, self.ts = candidates(src_dump, prm)
        if len(np.asarray(src_dump[0]).reshape(-1, 3)):
            self.cs, self.c = anchor(src_dump, T, prm.voxel_length)
        else:
            self.cs, self.c = np.zeros(3), np.zeros(3)
        vl = np.float64(prm.voxel_length)
        d = [(self.gi[:, a].astype(np.float64) + 0.5) * vl - self.cs[a] for a in range(3)]
        self.q = [(T[a, 0] * d[0] + T[a, 1] * d[1]) + T[a, 2] * d[2] for a in range(3)]


def linearise(dst_dump, src_dump, T_init, A, prm, problem=None):
    """One linearisation at the state A -> Lin(H [6,6], g [6], e, inliers, candidates, sum |terms| of H [6,6] and of g [6] (e is its
    own), fragile count)."""
    P = problem or Problem(dst_dump, src_dump, T_init, prm)
    A = np.asarray(A, np.float64)
    vl, trunc = np.float64(prm.voxel_length), np.float64(prm.sdf_trunc)
    n = len(P.ts)
    q = P.q
    y = [((A[a, 0] * q[0] + A[a, 1] * q[1]) + A[a, 2] * q[2]) + A[a, 3] for a in range(3)]
    g0, r = [], []
    ok = np.ones(n, bool)
    for a in range(3):
        p = P.c[a] + y[a]
        g = p / vl - 0.5
        with np.errstate(invalid="ignore"):
            ok &= np.abs(g) < 1.0e9
        f = np.floor(g)
        g0.append(np.where(ok, f, 0.0).astype(np.int64))
        r.append(g - f)
    fragile = np.zeros(n, bool)
    for a in range(3):
        fragile |= ok & ((np.abs(r[a]) < FRAGILE_BAND) | (np.abs(r[a] - 1.0) < FRAGILE_BAND))
    valid = ok.copy()
    f = []
    for _i, sx, sy, sz in rr._corners():
        if P.grid is None:
            valid[:] = False
            f.append(np.zeros(n))
            continue
        row, word = P.grid.locate(g0[0] + sx, g0[1] + sy, g0[2] + sz)
        rr_ = np.maximum(row, 0)
        valid &= (row >= 0) & (P.grid.weight[rr_, word].astype(np.float64) > prm.weight_threshold)
        f.append(P.grid.tsdf[rr_, word].astype(np.float64))
    u = [1 - r[a] for a in range(3)]
    c00, c01 = u[2] * f[0] + r[2] * f[4], u[2] * f[3] + r[2] * f[7]
    c10, c11 = u[2] * f[1] + r[2] * f[5], u[2] * f[2] + r[2] * f[6]
    b0, b1 = u[1] * c00 + r[1] * c01, u[1] * c10 + r[1] * c11
    phi = _lerp(r, f)  # (the merge contract's expression: u0 b0 + r0 b1)
    rho = trunc * (phi - P.ts.astype(np.float64))
    for bound in (prm.residual_trunc, prm.huber_delta):
        fragile |= valid & (np.abs(np.abs(rho) - bound) < FRAGILE_BAND)
    inl = valid & (np.abs(rho) <= prm.residual_trunc)
    e = [b1 - b0, u[0] * (c01 - c00) + r[0] * (c11 - c10),
         u[0] * (u[1] * (f[4] - f[0]) + r[1] * (f[7] - f[3])) + r[0] * (u[1] * (f[5] - f[1]) + r[1] * (f[6] - f[2]))]
    scale = trunc / vl
    grad = [scale * e[a] for a in range(3)]
    J = [y[1] * grad[2] - y[2] * grad[1], y[2] * grad[0] - y[0] * grad[2], y[0] * grad[1] - y[1] * grad[0], grad[0], grad[1], grad[2]]
    rho, J = rho[inl], [j[inl] for j in J]
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(np.abs(rho) <= prm.huber_delta, 1.0, prm.huber_delta / np.abs(rho))
    H, H_abs, g, g_abs = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros(6), np.zeros(6)
    for a in range(6):
        wa = w * J[a]
        for b in range(a, 6):
            t = wa * J[b]
            H[a, b] = H[b, a] = t.sum()
            H_abs[a, b] = H_abs[b, a] = np.abs(t).sum()
        t = wa * rho
        g[a], g_abs[a] = t.sum(), np.abs(t).sum()
    return Lin(H, g, float((rho * rho).sum()), int(inl.sum()), n, H_abs, g_abs, int(fragile.sum()))


def solve(H, g, inliers):
    """-> (xi [6], degenerate): Cholesky in the contract's order."""
    trH = 0.0
    for a in range(6):
        trH += H[a, a]
    degenerate = inliers < MIN_INLIERS
    Lm = np.zeros((6, 6))
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(6):
            d = H[j, j]
            for k in range(j):
                d -= Lm[j, k] * Lm[j, k]
            if not d > PIVOT_REL * trH:
                degenerate = True
            Lm[j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                s = H[i, j]
                for k in range(j):
                    s -= Lm[i, k] * Lm[j, k]
                Lm[i, j] = s / Lm[j, j]
        y, xi = np.zeros(6), np.zeros(6)
        for i in range(6):
            s = -g[i]
            for k in range(i):
                s -= Lm[i, k] * y[k]
            y[i] = s / Lm[i, i]
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s -= Lm[k, i] * xi[k]
            xi[i] = s / Lm[i, i]
    return (np.zeros(6), True) if degenerate else (xi, False)


def exp_se3(xi):
    """[Rodrigues(omega), t] -> [4,4]."""
    w = np.asarray(xi[:3], np.float64)
    th = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    sa = 1.0 if th < 1e-8 else np.sin(th) / th
    sb = 0.5 if th < 1e-8 else (1.0 - np.cos(th)) / (th * th)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + sa * K + sb * (K @ K)
    E[:3, 3] = xi[3:]
    return E


def compose(c, A, T_init):
    """Tr(c) A Tr(-c) T_init as the contract evaluates it."""
    M = np.eye(4)
    M[:3, :3] = A[:3, :3]
    M[:3, 3] = (c + A[:3, 3]) - A[:3, :3] @ c
    return M @ np.asarray(T_init, np.float64)


def register_reference(dst_dump, src_dump, T_init, prm, max_iterations=30):
    """The whole call -> dict(transformation, fitness, inlier_rmse, information, success, iterations, inliers, candidates, anchor,
    trace = one dict per linearisation as RegistrationResult.trace, plus `fragile`)."""
    T_init = np.asarray(T_init, np.float64)
    why = check_arguments(T_init, prm, max_iterations)
    if why is not None:
        raise ValueError(why)
    P = Problem(dst_dump, src_dump, T_init, prm)
    out = dict(transformation=T_init.copy(), fitness=0.0, inlier_rmse=0.0, information=np.zeros((6, 6)), success=False, iterations=0,
               inliers=0, candidates=0, anchor=P.c.copy(), trace=[])
    if len(P.ts) == 0:
        return out
    A = np.eye(4)
    status = 0
    lin = None
    for it in range(int(max_iterations)):
        lin = linearise(dst_dump, src_dump, T_init, A, prm, P)
        xi, degenerate = solve(lin.H, lin.g, lin.inliers)
        status = 2 if degenerate else 0
        A0 = A
        if not degenerate:
            A = exp_se3(xi) @ A0
            if np.linalg.norm(xi[:3]) + np.linalg.norm(xi[3:]) < CONVERGED:
                status = 1
        out["trace"].append(dict(iteration=it, status=status, inliers=lin.inliers, candidates=lin.candidates, sq_error=lin.e, A=A0.copy(),
                                 H=lin.H, g=lin.g, xi=xi, fragile=lin.fragile))
        if status != 0:
            break
    moved = not np.array_equal(A, np.eye(4))
    out.update(transformation=compose(P.c, A, T_init) if moved else T_init.copy(), information=lin.H, inliers=lin.inliers,
               candidates=lin.candidates, fitness=lin.inliers / lin.candidates if lin.candidates else 0.0,
               inlier_rmse=float(np.sqrt(lin.e / lin.inliers)) if lin.inliers else 0.0, iterations=len(out["trace"]),
               success=bool(status != 2 and lin.inliers >= MIN_INLIERS))
    return out
