"""The cross-view consistency check of hv_depth_consistency (include/hipvol.h, rules C1 - C7), restated in plain numpy.  Rule C2 is
rule M3 of the plane sweep, by the function of tests/mvs_reference.py.  Every float step is float32, operation for operation: numpy
rounds each float32 operation once, as the kernel does (the library is built without contraction and with IEEE division).  The GPU
is held to this bit for bit (tests/test_gpu_depth_consistency.py)."""
import numpy as np

from tests import mvs_reference as mr

DEFAULTS = dict(max_reproj_error=1.0, inv_depth_tol=0.0, rel_depth_tol=0.01, min_consistent=1, max_violations=0, fuse=True)
F = np.float32


def is_depth(z):
    """Rules C1 and C2: z > 0 and z < inf (a NaN fails both)"""
    with np.errstate(invalid="ignore"):
        return (z > F(0)) & (z < F(np.inf))


def forward(view, z):
    """Rule C2 for one view [3,4] and the depth map z [H,W].  -> (seen bool, ur, vr float32 - the integer pixel, +0.0 for 0 -, zs)"""
    H, W = z.shape
    view = np.asarray(view, F).reshape(3, 4)
    valid = is_depth(z)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = (F(1.0) / z).astype(F)
        x = np.arange(W, dtype=F)[None, :]
        y = np.arange(H, dtype=F)[:, None]
        q = [(((view[i, 0] * x + view[i, 1] * y) + view[i, 2]) + w * view[i, 3]).astype(F) for i in range(3)]
        ur, vr = np.rint(q[0] / q[2]), np.rint(q[1] / q[2])
        seen = valid & (q[2] > F(0)) & (ur >= F(0)) & (ur <= F(W - 1)) & (vr >= F(0)) & (vr <= F(H - 1))
        zs = (z * q[2]).astype(F)
    ur = np.where(seen, ur, F(0)).astype(np.int64).astype(F)
    vr = np.where(seen, vr, F(0)).astype(np.int64).astype(F)
    return seen, ur, vr, zs


def backward(back_view, ur, vr, d):
    """Rule C3 for one view.  -> (q2, e2, zb, wb) float32 [H,W]"""
    H, W = d.shape
    m = np.asarray(back_view, F).reshape(3, 4)
    x = np.arange(W, dtype=F)[None, :]
    y = np.arange(H, dtype=F)[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        ws = (F(1.0) / d).astype(F)
        q = [(((m[i, 0] * ur + m[i, 1] * vr) + m[i, 2]) + ws * m[i, 3]).astype(F) for i in range(3)]
        xb, yb, zb = (q[0] / q[2]).astype(F), (q[1] / q[2]).astype(F), (d * q[2]).astype(F)
        ex, ey = (xb - x).astype(F), (yb - y).astype(F)
        e2 = (ex * ex + ey * ey).astype(F)
        wb = (F(1.0) / zb).astype(F)
    return q[2], e2, zb, wb


def depth_consistency(depth, source_depths, views, back_views, *, max_reproj_error=1.0, inv_depth_tol=0.0, rel_depth_tol=0.01,
                      min_consistent=1, max_violations=0, fuse=True, return_parts=False):
    """-> (depth float32 [H,W], counts uint8 [H,W,4]: agree, occluded, violated, seen, stats (valid, kept, agree sum)) [, parts]"""
    z = np.asarray(depth, F)
    H, W = z.shape
    sources = [np.asarray(s, F) for s in source_depths]
    N = len(sources)
    views, back_views = np.asarray(views, F).reshape(-1, 3, 4), np.asarray(back_views, F).reshape(-1, 3, 4)
    assert 1 <= N <= 4 and len(views) == N and len(back_views) == N and 0 <= min_consistent <= N and 0 <= max_violations <= N
    assert all(s.shape == (H, W) for s in sources)
    max_e2 = F(max_reproj_error) * F(max_reproj_error)
    valid = is_depth(z)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = (F(1.0) / z).astype(F)
        tol = (F(inv_depth_tol) + F(rel_depth_tol) * w).astype(F)
    agree, occluded, violated, seen_n = (np.zeros((H, W), np.int32) for _ in range(4))
    acc = z.copy()
    parts = []
    for s in range(N):
        seen, ur, vr, zs = forward(views[s], z)
        d = np.where(seen, sources[s][vr.astype(np.int64), ur.astype(np.int64)], F(0)).astype(F)
        has = seen & is_depth(d)
        q2, e2, zb, wb = backward(back_views[s], ur, vr, d)
        with np.errstate(invalid="ignore"):
            ok = has & (q2 > F(0)) & (e2 <= max_e2) & (np.abs((wb - w).astype(F)) <= tol)
            occ = has & ~ok & (d < zs)
        vio = has & ~ok & ~occ
        seen_n += seen
        agree += ok
        occluded += occ
        violated += vio
        with np.errstate(invalid="ignore", over="ignore"):
            acc = np.where(ok, (acc + zb).astype(F), acc)
        parts.append(dict(seen=seen, ur=ur, vr=vr, zs=zs, d=d, has=has, q2=q2, e2=e2, zb=zb, wb=wb, agree=ok, occluded=occ, violated=vio))
    kept = valid & (agree >= int(min_consistent)) & (violated <= int(max_violations))
    with np.errstate(invalid="ignore", over="ignore"):
        fused = (acc / (agree + 1).astype(F)).astype(F)
    out = np.where(kept, fused if fuse else z, F(0)).astype(F)
    counts = np.stack([agree, occluded, violated, seen_n], axis=-1).astype(np.uint8)
    stats = (int(valid.sum()), int(kept.sum()), int(agree.sum()))
    if return_parts:
        return out, counts, stats, dict(views=parts, valid=valid, kept=kept, w=w, tol=tol, max_e2=max_e2)
    return out, counts, stats
