"""numpy restatement of the TSDF point queries (include/hipvol.h, hv_tsdf_sample_points and hv_tsdf_check_frame) on a dump() tuple -
test infrastructure, no GPU, never touches the library.

The arithmetic follows the contract operation by operation in float64 (every product and sum its own numpy call: nothing is
contracted), so the outputs here and the library's are meant to agree bit for bit.  Where a decision sits on a boundary of the rules
(some component of r within FRAGILE_BAND of 0, 0.5 or 1: a one-ulp difference in g changes the cell or the nearest voxel) the point
is marked FRAGILE for the tests that compare two implementations.  The mean colours are the dump's own ((double)sum / (double)weight,
as hv_tsdf_dump computes them).
"""
import numpy as np

from tests import raycast_reference as rr

FRAGILE_BAND = 1e-9
OUTSIDE, UNOBSERVED, NEAREST, TRILINEAR = 0, 1, 2, 3
INVALID, UNKNOWN, CONSISTENT, IN_FRONT, BEHIND = 0, 1, 2, 3, 4


def _tri(r, f):
    """phi and (dphi/dr0, dphi/dr1, dphi/dr2) of the eight values f, in the contract's order of operations."""
    u0, u1, u2 = 1 - r[0], 1 - r[1], 1 - r[2]
    c00, c01 = u2 * f[0] + r[2] * f[4], u2 * f[3] + r[2] * f[7]
    c10, c11 = u2 * f[1] + r[2] * f[5], u2 * f[2] + r[2] * f[6]
    b0, b1 = u1 * c00 + r[1] * c01, u1 * c10 + r[1] * c11
    phi = u0 * b0 + r[0] * b1
    e0 = b1 - b0
    e1 = u0 * (c01 - c00) + r[0] * (c11 - c10)
    e2 = u0 * (u1 * (f[4] - f[0]) + r[1] * (f[7] - f[3])) + r[0] * (u1 * (f[5] - f[1]) + r[1] * (f[6] - f[2]))
    return phi, (e0, e1, e2)


def locate(p, voxel_length):
    """The contract's cell of points p [n,3] float64 -> (ok [n], g0 [3][n] int64, r [3][n]), as the library leaves them: ok accumulates
    over the axes, g0 is 0 from the first refused axis on, r of a refused point means nothing."""
    vl = np.float64(voxel_length)
    ok = np.ones(len(p), bool)
    g0, r = [], []
    for a in range(3):
        g = p[:, a] / vl - 0.5
        ok &= np.abs(g) < 1.0e9
        f = np.floor(g)
        g0.append(np.where(ok, f, 0.0).astype(np.int64))
        r.append(g - f)
    return ok, g0, r


def sample_points(dump, voxel_length, sdf_trunc, points, weight_threshold=0.0):
    """-> dict of sdf [n] f32, gradient [n,3] f32, color [n,3] f32, weight [n] f32, status [n] u8, fragile [n] bool for points [n,3]
    (float32 is widened first)."""
    p = np.asarray(points).astype(np.float64).reshape(-1, 3)
    n = len(p)
    vl, trunc, thr = np.float64(voxel_length), np.float64(sdf_trunc), np.float64(weight_threshold)
    empty = len(np.asarray(dump[0]).reshape(-1, 3)) == 0
    grid = None if empty else rr._Grid(dump)
    colour = None if empty else np.asarray(dump[3], np.float64).reshape(len(grid.codes), -1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        ok, g0, r = locate(p, vl)
        g0 = [np.where(ok, x, 0) for x in g0]  # (the library's g0 of a refused point is not used either)
        r = [np.where(ok, x, 0.0) for x in r]
        fragile = np.zeros(n, bool)
        for a in range(3):
            fragile |= ok & ((np.abs(r[a]) < FRAGILE_BAND) | (np.abs(r[a] - 0.5) < FRAGILE_BAND) | (np.abs(r[a] - 1.0) < FRAGILE_BAND))
    out = {"sdf": np.zeros(n, np.float32), "gradient": np.zeros((n, 3), np.float32), "color": np.zeros((n, 3), np.float32),
           "weight": np.zeros(n, np.float32), "status": np.zeros(n, np.uint8), "fragile": fragile}
    if n == 0 or empty:  # (an empty map holds no unit: every point is OUTSIDE)
        return out

    def voxel(gx, gy, gz):
        row, word = grid.locate(gx, gy, gz)
        rr_ = np.maximum(row, 0)
        held = row >= 0
        w = np.where(held, grid.weight[rr_, word], np.float32(0)).astype(np.float64)
        return held, w, grid.tsdf[rr_, word].astype(np.float64), colour[rr_, word]

    nheld, nw, nt, nc = voxel(*[g0[a] + (r[a] >= 0.5) for a in range(3)])
    nheld = nheld & ok
    nobs = nheld & (nw > thr)
    all8 = np.ones(n, bool)
    f_t, f_c = [], []
    for _i, sx, sy, sz in rr._corners():
        held, w, t, c = voxel(g0[0] + sx, g0[1] + sy, g0[2] + sz)
        all8 &= held & (w > thr)
        f_t.append(t)
        f_c.append(c)
    tri = nobs & all8
    near = nobs & ~all8
    out["status"] = np.where(~nheld, OUTSIDE, np.where(~nobs, UNOBSERVED, np.where(all8, TRILINEAR, NEAREST))).astype(np.uint8)
    phi, e = _tri(r, f_t)
    scale = trunc / vl
    with np.errstate(invalid="ignore", over="ignore"):
        out["sdf"] = np.where(tri, (trunc * phi).astype(np.float32), np.where(near, (trunc * nt).astype(np.float32), np.float32(0)))
        for a in range(3):
            out["gradient"][:, a] = np.where(tri, (scale * e[a]).astype(np.float32), np.float32(0))
        for k in range(3):
            m, _ = _tri(r, [c[:, k] for c in f_c])
            out["color"][:, k] = np.where(tri, (m / 255.0).astype(np.float32), np.where(near, (nc[:, k] / 255.0).astype(np.float32), np.float32(0)))
    out["weight"] = np.where(nobs, nw, 0.0).astype(np.float32)
    return out


def classify(sdf, status, valid, tolerance):
    """The class rule on the float32 sdf of a sample (widened, compared with tolerance in double)."""
    s = np.asarray(sdf, np.float32).astype(np.float64)
    tol = np.float64(tolerance)
    known = np.asarray(valid, bool) & (np.asarray(status) >= NEAREST)
    cls = np.where(s > tol, IN_FRONT, np.where(s < -tol, BEHIND, CONSISTENT))
    return np.where(~np.asarray(valid, bool), INVALID, np.where(~known, UNKNOWN, cls)).astype(np.uint8)


def frame_points(depth, intr, T_cw, depth_scale, depth_min, depth_max):
    """The contract's depth and point steps -> (valid [H,W] bool, points [H,W,3] float64; rows of invalid pixels mean nothing)."""
    raw = np.asarray(depth)
    H, W = raw.shape
    d = raw.astype(np.float32) / np.float32(depth_scale)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(d) & (d.astype(np.float64) > np.float64(depth_min)) & (d.astype(np.float64) <= np.float64(depth_max))
    fx, fy, cx, cy = (np.float64(x) for x in intr)
    T = np.asarray(T_cw, np.float64)
    Rwc = T[:3, :3].T
    twc = [-((Rwc[k, 0] * T[0, 3] + Rwc[k, 1] * T[1, 3]) + Rwc[k, 2] * T[2, 3]) for k in range(3)]
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    z = np.where(valid, d, np.float32(0)).astype(np.float64)
    a = (u - cx) / fx
    x = a * z
    b = (v - cy) / fy
    y = b * z
    P = np.stack([((Rwc[k, 0] * x + Rwc[k, 1] * y) + Rwc[k, 2] * z) + twc[k] for k in range(3)], axis=-1)
    return valid, P


def check_frame(dump, voxel_length, sdf_trunc, depth, intr, T_cw, depth_scale=1.0, depth_min=0.1, depth_max=3.0, weight_threshold=0.0,
                tolerance=None):
    """-> dict of sdf [H,W] f32, cls [H,W] u8, count [5] int64, fragile [H,W] bool (valid pixels whose point is fragile)."""
    tol = 0.5 * float(sdf_trunc) if tolerance is None else tolerance
    valid, P = frame_points(depth, intr, T_cw, depth_scale, depth_min, depth_max)
    H, W = valid.shape
    s = sample_points(dump, voxel_length, sdf_trunc, P.reshape(-1, 3), weight_threshold)
    cls = classify(s["sdf"], s["status"], valid.reshape(-1), tol)
    sdf = np.where(cls >= CONSISTENT, s["sdf"], np.float32(0)).astype(np.float32)
    return {"sdf": sdf.reshape(H, W), "cls": cls.reshape(H, W), "count": np.bincount(cls, minlength=5).astype(np.int64),
            "fragile": (s["fragile"] & valid.reshape(-1)).reshape(H, W)}
