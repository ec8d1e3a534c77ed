"""The plane-sweep matcher of hv_mvs_sgm (include/hipvol.h, rules M1 - M10), restated in plain numpy.  The rules it shares with the
stereo matcher (grey, census, paths, winner, uniqueness, sub-pixel) are the functions of tests/stereo_reference.py; the speckle step
is tests/speckle_reference.py.  Every float step is float32, operation for operation: numpy rounds each float32 operation once, as
the kernels do (the library is built without contraction and with IEEE division).  The GPU is held to this bit for bit
(tests/test_gpu_mvs.py)."""
import numpy as np

from tests import speckle_reference as kr
from tests import stereo_reference as sr

DEFAULTS = dict(num_planes=128, p1=10, p2=120, uniqueness_ratio=15, min_views=1, paths=8, speckle_window_size=0, speckle_range=1)
INVALID = sr.INVALID_D16


def plane_parameters(min_depth, max_depth, num_planes):
    """Rule M2's constants: double arithmetic with exactly these operations, rounded once.  -> (w0, step16) float32"""
    inv_far = 0.0 if np.isinf(max_depth) else 1.0 / float(max_depth)
    with np.errstate(over="ignore"):
        return np.float32(inv_far), np.float32((1.0 / float(min_depth) - inv_far) / (16.0 * float(int(num_planes) - 1)))


def inverse_depth(w0, step16, k16):
    """Rules M2 and M9: w = w0 + float(k16) * step16, one float32 multiply and one add.  k16 = 16 k for plane k.  -> float32"""
    return (np.float32(w0) + np.asarray(k16).astype(np.float32) * np.float32(step16)).astype(np.float32)


def project(view, H, W, w):
    """Rule M3 for one view [3,4] and the inverse depths w [D].  -> (seen bool, ur, vr, q2, u float32), each [H,W,D]"""
    m = np.asarray(view, np.float32).reshape(3, 4)
    x = np.arange(W, dtype=np.float32)[None, :, None]
    y = np.arange(H, dtype=np.float32)[:, None, None]
    w = np.asarray(w, np.float32)[None, None, :]
    q = []
    for i in range(3):
        a = (m[i, 0] * x + m[i, 1] * y) + m[i, 2]
        q.append((a + w * m[i, 3]).astype(np.float32))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u, v = (q[0] / q[2]).astype(np.float32), (q[1] / q[2]).astype(np.float32)
        ur, vr = np.rint(u), np.rint(v)
        seen = (q[2] > np.float32(0)) & (ur >= np.float32(0)) & (ur <= np.float32(W - 1)) & (vr >= np.float32(0)) & (vr <= np.float32(H - 1))
    shape = (H, W, w.shape[2])
    return tuple(np.broadcast_to(a, shape) for a in (seen, ur, vr, q[2], u))


def seen_count(views, H, W, w):
    """-> n int32 [H,W,D]: the views that see (x, y, k)"""
    return sum(project(v, H, W, w)[0].astype(np.int32) for v in views)


def cost_terms(census_ref, census_sources, views, w):
    """-> (sum, n) int32 [H,W,D] of rule M4"""
    H, W = census_ref.shape
    total = np.zeros((H, W, len(w)), np.int32)
    n = np.zeros((H, W, len(w)), np.int32)
    for cs, view in zip(census_sources, views):
        seen, ur, vr, _, _ = project(view, H, W, w)
        xi = np.where(seen, ur, 0).astype(np.int64)
        yi = np.where(seen, vr, 0).astype(np.int64)
        ham = sr.popcount64(census_ref[:, :, None] ^ cs[yi, xi])
        total += np.where(seen, ham, 0)
        n += seen
    return total, n


def cost_volume(total, n, min_views):
    """Rule M4: (2 sum + n) / (2 n) with C division (nothing is negative) where n >= min_views, else 64.  -> int32 [H,W,D]"""
    return np.where(n >= int(min_views), (2 * total + n) // (2 * np.maximum(n, 1)), 64).astype(np.int32)


def depth_out(index, w0, step16):
    """Rule M9.  -> float32 [H,W]"""
    wv = inverse_depth(w0, step16, index)
    ok = (np.asarray(index) != INVALID) & ~(wv <= np.float32(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (np.float32(1.0) / np.where(ok, wv, np.float32(1.0))).astype(np.float32)
    return np.where(ok, z, np.float32(0.0)).astype(np.float32)


def multiview_sgm(ref, sources, views, *, min_depth, max_depth=np.inf, num_planes=128, p1=10, p2=120, uniqueness_ratio=15, min_views=1,
                  paths=8, speckle_window_size=0, speckle_range=1, return_parts=False):
    """-> (index int16 [H,W] in sixteenths of a plane, -16 = invalid; depth float32 [H,W]) [, parts: C, S, n, k_star, w]"""
    D = int(num_planes)
    views = np.asarray(views, np.float32).reshape(-1, 3, 4)
    N = len(sources)
    assert D % 16 == 0 and 16 <= D <= 256 and 1 <= N <= 4 and len(views) == N and 1 <= min_views <= N, (D, N, min_views)
    w0, step16 = plane_parameters(min_depth, max_depth, D)
    w = inverse_depth(w0, step16, 16 * np.arange(D))
    cref = sr.census(sr.grey(ref))
    H, W = cref.shape
    total, n = cost_terms(cref, [sr.census(sr.grey(s)) for s in sources], views, w)
    C = cost_volume(total, n, min_views)
    S = sr.aggregate(C, int(p1), int(p2), int(paths))
    k_star = sr.winner(S)
    n_star = np.take_along_axis(n, k_star[..., None], axis=2)[..., 0]
    valid = sr.unique(S, k_star, uniqueness_ratio) & (n_star >= int(min_views))  # M5, M6
    index = sr.disparity_out(sr.subpixel(S, k_star), valid)  # M7
    if int(speckle_window_size) > 0:  # M8
        index = kr.filter_speckles(index, int(speckle_window_size), 16 * int(speckle_range), new_val=INVALID).image
    depth = depth_out(index, w0, step16)
    if return_parts:
        return index, depth, dict(C=C, S=S, n=n, sum=total, k_star=k_star, w=w, valid=valid)
    return index, depth
