"""The census semi-global stereo matcher of hv_stereo_sgm (include/hipvol.h), restated in plain numpy: one function per numbered
rule of the header's comment.  Integer arithmetic throughout (int32 / int64 arrays), float32 only in rule 10.  The GPU is held to
this bit for bit (tests/test_gpu_stereo.py); tests/golden/stereo_sgm_tiny.npz pins this file against later edits."""
import numpy as np

CENSUS_W, CENSUS_H = 9, 7
INVALID_D16 = -16
DEFAULTS = dict(num_disparities=128, p1=10, p2=120, uniqueness_ratio=15, max_diff=1, paths=8)
# (dx, dy) of the step from q to p: the first four are paths = 4
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))

_POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def grey(img):
    """Rule 1: one channel as is; three channels (c0 + 2 c1 + c2 + 2) >> 2.  -> int32 [H,W]"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)), (a.dtype, a.shape)
    if a.ndim == 2:
        return a.astype(np.int32)
    c = a.astype(np.int32)
    return (c[..., 0] + 2 * c[..., 1] + c[..., 2] + 2) >> 2


def census(g):
    """Rule 2: 9 x 7 window, centre excluded, bit = neighbour < centre, replicated border.  -> uint64 [H,W] (62 bits used)"""
    H, W = g.shape
    ry, rx = CENSUS_H // 2, CENSUS_W // 2
    pad = np.pad(g, ((ry, ry), (rx, rx)), mode="edge")
    out = np.zeros((H, W), np.uint64)
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            if dy == 0 and dx == 0:
                continue
            out = (out << np.uint64(1)) | (pad[ry + dy:ry + dy + H, rx + dx:rx + dx + W] < g).astype(np.uint64)
    return out


def popcount64(a):
    return _POPCOUNT8[np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1, dtype=np.int32)


def cost_volume(census_left, census_right, D):
    """Rule 3: C(y,x,d) = popcount(cL(y,x) ^ cR(y,x-d)) for x - d >= 0, else 64.  -> int32 [H,W,D]"""
    H, W = census_left.shape
    C = np.full((H, W, D), 64, np.int32)
    for d in range(min(D, W)):
        C[:, d:, d] = popcount64(census_left[:, d:] ^ census_right[:, :W - d])
    return C


def _step(C_p, L_q, p1, p2):
    """L(p,.) from L(q,.) for rows of pixels: C_p, L_q int32 [N,D]."""
    big = np.int32(1 << 20)
    M = L_q.min(axis=1, keepdims=True)
    lo = np.concatenate([np.full_like(L_q[:, :1], big), L_q[:, :-1]], axis=1) + p1  # L(q,d-1) + P1, absent at d = 0
    hi = np.concatenate([L_q[:, 1:], np.full_like(L_q[:, :1], big)], axis=1) + p1   # L(q,d+1) + P1, absent at d = D-1
    return C_p + np.minimum(np.minimum(L_q, lo), np.minimum(hi, M + p2)) - M


def aggregate_path(C, dx, dy, p1, p2):
    """Rule 4, one path direction: q = p - (dx, dy); L(p,.) = C(p,.) where q is outside the image.  -> int32 [H,W,D]"""
    H, W, D = C.shape
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(C[:, x], L[:, x - dx], p1, p2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    for i, y in enumerate(ys):
        L[y] = C[y]
        if i == 0:
            continue
        xq = np.arange(W) - dx
        inside = (xq >= 0) & (xq < W)
        L[y, inside] = _step(C[y, inside], L[y - dy, xq[inside]], p1, p2)
    return L


def aggregate(C, p1, p2, paths):
    """Rule 4: S = sum of L over the 4 or 8 paths.  -> int32 [H,W,D], every entry <= paths * (64 + P2)"""
    assert paths in (4, 8) and 0 < p1 <= p2 <= 1023, (paths, p1, p2)
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS[:paths]:
        S += aggregate_path(C, dx, dy, p1, p2)
    return S


def winner(S):
    """Rule 5: the smallest d attaining min_d S(p,d).  -> int32 [H,W]"""
    return S.argmin(axis=2).astype(np.int32)


def unique(S, d_star, uniqueness_ratio):
    """Rule 6: False where some d with |d - d*| > 1 has S(p,d) (100 - u) < S(p,d*) 100.  -> bool [H,W]"""
    D = S.shape[2]
    best = np.take_along_axis(S, d_star[..., None], axis=2)
    far = np.abs(np.arange(D, dtype=np.int32)[None, None, :] - d_star[..., None]) > 1
    return ~(far & (S * (100 - int(uniqueness_ratio)) < best * 100)).any(axis=2)


def right_disparity(S):
    """Rule 7, first part: dR(y,xr) = the smallest d attaining the minimum of S(y, xr + d, d) over xr + d < W.  -> int32 [H,W]"""
    H, W, D = S.shape
    big = np.int32(1 << 30)
    R = np.full((H, W, D), big, np.int32)
    for d in range(min(D, W)):
        R[:, :W - d, d] = S[:, d:, d]
    return R.argmin(axis=2).astype(np.int32)


def left_right_consistent(d_star, d_right, max_diff):
    """Rule 7: False where x - d* < 0 or |dR(y, x - d*) - d*| > max_diff; all True for a negative max_diff.  -> bool [H,W]"""
    H, W = d_star.shape
    if max_diff < 0:
        return np.ones((H, W), bool)
    xr = np.arange(W, dtype=np.int32)[None, :] - d_star
    ok = xr >= 0
    dr = np.take_along_axis(d_right, np.clip(xr, 0, W - 1), axis=1)
    return ok & (np.abs(dr - d_star) <= int(max_diff))


def _cdiv(a, b):
    """C division of integer arrays: truncates toward zero (b > 0)."""
    return np.where(a >= 0, a // b, -((-a) // b))


def subpixel(S, d_star):
    """Rule 8: d16 in sixteenths; the parabola offset for 0 < d* < D-1, 16 d* otherwise.  -> int32 [H,W]"""
    D = S.shape[2]
    inner = (d_star > 0) & (d_star < D - 1)
    dm = np.clip(d_star - 1, 0, D - 1)[..., None]
    dp = np.clip(d_star + 1, 0, D - 1)[..., None]
    s0 = np.take_along_axis(S, d_star[..., None], axis=2)[..., 0]
    sm = np.take_along_axis(S, dm, axis=2)[..., 0]
    sp = np.take_along_axis(S, dp, axis=2)[..., 0]
    den = np.maximum(sm + sp - 2 * s0, 1)
    off = _cdiv((sm - sp) * 16 + den, 2 * den)
    return (16 * d_star + np.where(inner, off, 0)).astype(np.int32)


def disparity_out(d16, valid):
    """Rule 9: int16, d16 where valid, -16 elsewhere."""
    return np.where(valid, d16, INVALID_D16).astype(np.int16)


def depth_out(disparity16, bf, min_depth=0.0, max_depth=np.inf):
    """Rule 10: depth = (bf * 16f) / float(d16), one float32 multiply and one divide; 0 where d16 <= 0, where the result is
    < min_depth, or > max_depth when max_depth is finite.  -> float32"""
    d16 = np.asarray(disparity16).astype(np.int32)
    num = np.float32(bf) * np.float32(16.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (num / np.where(d16 > 0, d16, 1).astype(np.float32)).astype(np.float32)
    out = np.where(d16 > 0, q, np.float32(0.0)).astype(np.float32)
    out[out < np.float32(min_depth)] = 0.0
    if np.isfinite(max_depth):
        out[out > np.float32(max_depth)] = 0.0
    return out


def stereo_sgm(left, right, num_disparities=128, p1=10, p2=120, uniqueness_ratio=15, max_diff=1, paths=8, bf=None, min_depth=0.0,
               max_depth=np.inf, return_volume=False):
    """-> (disparity int16 [H,W], depth float32 [H,W] or None when bf is None) [, S]"""
    D = int(num_disparities)
    assert D % 16 == 0 and 16 <= D <= 256 and 0 <= uniqueness_ratio <= 99, (D, uniqueness_ratio)
    assert np.shape(left) == np.shape(right)
    C = cost_volume(census(grey(left)), census(grey(right)), D)
    S = aggregate(C, int(p1), int(p2), int(paths))
    d_star = winner(S)
    valid = unique(S, d_star, uniqueness_ratio) & left_right_consistent(d_star, right_disparity(S), int(max_diff))
    disp = disparity_out(subpixel(S, d_star), valid)
    depth = None if bf is None else depth_out(disp, bf, min_depth, max_depth)
    return (disp, depth, S) if return_volume else (disp, depth)
