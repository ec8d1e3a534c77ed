"""The census semi-global stereo matcher of hv_stereo_sgm (include/hipvol.h), restated in plain numpy: one function per numbered
rule of the header's comment.  Integer arithmetic throughout (int32 / int64 arrays), float32 only in rule 10.  The GPU is held to
this bit for bit (tests/test_gpu_stereo.py, tests/test_gpu_stereo_planted.py); tests/golden/stereo_sgm_tiny.npz pins this file
against later edits.

Every rule function takes variant=<name>: the WRONG readings listed in VARIANTS - the ways the kernels of
pyslam_amd/csrc/hv_stereo.hip in particular can go wrong (how they divide the disparities among lanes, slots, loop iterations and
tiles of a row) and the ways the rules themselves can be misread.  variant=None is the right reading.
tests/test_stereo_planted_cpu.py proves that the planted cases of tests/stereo_cases.py tell each of them from the right reading;
events() counts how often an input reaches the places where they differ.

The work-division readings speak the kernels' language: the path kernel holds L(q,.) in one wave, lane l the VPL consecutive
disparities l VPL .. l VPL + VPL - 1 (values_per_lane(D) = 1, 2, 4 for D <= 64, 128, 256) - a ROW of 16 lanes holds 16 VPL
disparities, a SLOT is d mod VPL; the winner kernel gives a pixel 16 lanes that loop over d, d + 16, ..., and works in TILES of
256 left pixels of a row."""
import numpy as np

CENSUS_W, CENSUS_H = 9, 7
INVALID_D16 = -16
DEFAULTS = dict(num_disparities=128, p1=10, p2=120, uniqueness_ratio=15, max_diff=1, paths=8)
# (dx, dy) of the step from q to p: the first four are paths = 4
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))
WIN_TILE = 256  # left pixels of a row that the winner kernel's workgroup takes
STARTS_PER_GROUP = 4  # path starts (waves) per workgroup of the path kernel

VARIANTS = (
    # -- work division
    "m_first_16_lanes",         # M(q) over the first row of 16 lanes only: d < 16 VPL
    "m_without_row1",           # M(q) without the lanes 16..31
    "m_without_row2",           # M(q) without the lanes 32..47
    "m_without_row3",           # M(q) without the lanes 48..63
    "no_lane_neighbours",       # d-1 of a lane's first slot and d+1 of its last slot absent: the lost neighbour-lane shuffle
    "below_wraps_at_0",         # d-1 at d = 0 not absent: what lane 0 gets from a shuffle from below, its own last slot L(q, VPL-1)
    "above_wraps_at_top",       # d+1 at d = D-1 not absent: what lane 63 gets from a shuffle from above, its own first slot L(q, D-VPL)
    "winner_first_16",          # d* searched in d < 16 only: one iteration of the winner's loop
    "unique_first_16",          # rule 6 searched in d < 16 only
    "dr_same_tile",             # dR from the votes of left pixels in the right pixel's own tile of 256 only
    "dr_without_right_tile",    # dR without the votes of the tile to the right (d <= 255: the same pixels as dr_same_tile)
    "diagonal_side_starts_zero",  # diagonal paths that start on the side column start with L = 0 instead of C
    "last_starts_dropped",      # the last n mod 4 path starts of a direction never run: L = 0 along them
    # -- rules
    "winner_tie_largest",       # rule 5 with the largest best d
    "dr_tie_largest",           # rule 7's dR with the largest best d
    "unique_le",                # rule 6 with <=
    "unique_gap0",              # rule 6 with |d - d*| > 0
    "unique_gap2",              # rule 6 with |d - d*| > 2
    "lr_clamped",               # rule 7 without its x - d* < 0 clause: the index clamped to 0 and compared
    "lr_strict",                # rule 7 with < max_diff
    "subpixel_floor",           # rule 8 with floor division
    "subpixel_at_ends",         # rule 8 applied at d* = 0 and D-1 too, the neighbours clamped
    "census_le",                # rule 2 with <=
    "census_zero_border",       # rule 2 with a border of zeros
    "census_7x9",               # rule 2 with a window 7 wide and 9 high
    "cost_0_outside",           # rule 3 with 0 where x - d < 0
    "cost_clamped_outside",     # rule 3 read from the right image's column 0 where x - d < 0
    "no_minus_m",               # rule 4 without its - M(q)
    "grey_no_round",            # rule 1 without the + 2
    "grey_weight_c0",           # rule 1 with the weight 2 on channel 0
    "depth_min_le",             # rule 10 cutting depth <= min_depth
    "depth_max_inf",            # rule 10 with max_depth taken as infinite
)

_POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def values_per_lane(D):
    """The consecutive disparities one lane of the path kernel holds."""
    return 1 if D <= 64 else 2 if D <= 128 else 4


def grey(img, variant=None):
    """Rule 1: one channel as is; three channels (c0 + 2 c1 + c2 + 2) >> 2.  -> int32 [H,W]"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)), (a.dtype, a.shape)
    if a.ndim == 2:
        return a.astype(np.int32)
    c = a.astype(np.int32)
    if variant == "grey_no_round":
        return (c[..., 0] + 2 * c[..., 1] + c[..., 2]) >> 2
    if variant == "grey_weight_c0":
        return (2 * c[..., 0] + c[..., 1] + c[..., 2] + 2) >> 2
    return (c[..., 0] + 2 * c[..., 1] + c[..., 2] + 2) >> 2


def census(g, variant=None):
    """Rule 2: 9 x 7 window, centre excluded, bit = neighbour < centre, replicated border.  -> uint64 [H,W] (62 bits used)"""
    H, W = g.shape
    ry, rx = CENSUS_H // 2, CENSUS_W // 2
    if variant == "census_7x9":
        ry, rx = rx, ry
    if variant == "census_zero_border":
        pad = np.pad(g, ((ry, ry), (rx, rx)), mode="constant")
    else:
        pad = np.pad(g, ((ry, ry), (rx, rx)), mode="edge")
    out = np.zeros((H, W), np.uint64)
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            if dy == 0 and dx == 0:
                continue
            nb = pad[ry + dy:ry + dy + H, rx + dx:rx + dx + W]
            out = (out << np.uint64(1)) | (nb <= g if variant == "census_le" else nb < g).astype(np.uint64)
    return out


def popcount64(a):
    return _POPCOUNT8[np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1, dtype=np.int32)


def cost_volume(census_left, census_right, D, variant=None):
    """Rule 3: C(y,x,d) = popcount(cL(y,x) ^ cR(y,x-d)) for x - d >= 0, else 64.  -> int32 [H,W,D]"""
    H, W = census_left.shape
    C = np.full((H, W, D), 0 if variant == "cost_0_outside" else 64, np.int32)
    for d in range(min(D, W)):
        C[:, d:, d] = popcount64(census_left[:, d:] ^ census_right[:, :W - d])
    if variant == "cost_clamped_outside":
        for d in range(1, D):
            C[:, :d, d] = popcount64(census_left[:, :d] ^ census_right[:, :1])
    return C


def _step(C_p, L_q, p1, p2, variant=None):
    """L(p,.) from L(q,.) for rows of pixels: C_p, L_q int32 [N,D]."""
    big = np.int32(1 << 20)
    D = L_q.shape[1]
    vpl = values_per_lane(D)
    if variant == "m_first_16_lanes":
        M = L_q[:, :16 * vpl].min(axis=1, keepdims=True)
    elif variant in ("m_without_row1", "m_without_row2", "m_without_row3"):
        r = int(variant[-1])
        keep = np.ones(D, bool)
        keep[16 * vpl * r:16 * vpl * (r + 1)] = False
        M = L_q[:, keep].min(axis=1, keepdims=True)
    else:
        M = L_q.min(axis=1, keepdims=True)
    lo = np.concatenate([np.full_like(L_q[:, :1], big), L_q[:, :-1]], axis=1) + p1  # L(q,d-1) + P1, absent at d = 0
    hi = np.concatenate([L_q[:, 1:], np.full_like(L_q[:, :1], big)], axis=1) + p1   # L(q,d+1) + P1, absent at d = D-1
    if variant == "no_lane_neighbours":
        lo[:, 0::vpl] = big + p1
        hi[:, vpl - 1::vpl] = big + p1
    elif variant == "below_wraps_at_0":
        lo[:, 0] = L_q[:, vpl - 1] + p1
    elif variant == "above_wraps_at_top" and D == 64 * vpl:  # (below that, the lane above the last one holds an absent L)
        hi[:, D - 1] = L_q[:, D - vpl] + p1
    out = C_p + np.minimum(np.minimum(L_q, lo), np.minimum(hi, M + p2))
    return out if variant == "no_minus_m" else out - M


def path_start_index(H, W, dx, dy):
    """The number of the path start (the kernel's wave) whose path runs through each pixel: with dx != 0 the H pixels of the column
    the direction leaves from come first, in y, then with dy != 0 the pixels of the row it leaves from, in x (without the corner
    when the column holds it already).  -> (index int32 [H,W], number of starts)"""
    y, x = np.meshgrid(np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32), indexing="ij")
    if dy == 0:
        return y, H
    if dx == 0:
        return x, W
    xs = x if dx > 0 else W - 1 - x  # steps back to the side column
    ys = y if dy > 0 else H - 1 - y  # steps back to the start row
    side = xs <= ys
    x_start = x - dx * ys            # where the path meets the start row, for the others
    k = x_start - 1 if dx > 0 else x_start
    return np.where(side, y - dy * xs, H + k).astype(np.int32), H + W - 1


def aggregate_path(C, dx, dy, p1, p2, variant=None):
    """Rule 4, one path direction: q = p - (dx, dy); L(p,.) = C(p,.) where q is outside the image.  -> int32 [H,W,D]"""
    H, W, D = C.shape
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(C[:, x], L[:, x - dx], p1, p2, variant)
    else:
        ys = range(H) if dy > 0 else range(H - 1, -1, -1)
        for i, y in enumerate(ys):
            L[y] = C[y]
            if variant == "diagonal_side_starts_zero" and dx != 0:
                L[y, 0 if dx > 0 else W - 1] = 0
            if i == 0:
                continue
            xq = np.arange(W) - dx
            inside = (xq >= 0) & (xq < W)
            L[y, inside] = _step(C[y, inside], L[y - dy, xq[inside]], p1, p2, variant)
    if variant == "last_starts_dropped":
        index, n = path_start_index(H, W, dx, dy)
        L[index >= n - n % STARTS_PER_GROUP] = 0
    return L


def aggregate(C, p1, p2, paths, variant=None):
    """Rule 4: S = sum of L over the 4 or 8 paths.  -> int32 [H,W,D], every entry <= paths * (64 + P2)"""
    assert paths in (4, 8) and 0 < p1 <= p2 <= 1023, (paths, p1, p2)
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS[:paths]:
        S += aggregate_path(C, dx, dy, p1, p2, variant)
    return S


def winner(S, variant=None):
    """Rule 5: the smallest d attaining min_d S(p,d).  -> int32 [H,W]"""
    if variant == "winner_first_16":
        return S[..., :16].argmin(axis=2).astype(np.int32)
    if variant == "winner_tie_largest":
        return (S.shape[2] - 1 - S[..., ::-1].argmin(axis=2)).astype(np.int32)
    return S.argmin(axis=2).astype(np.int32)


def unique(S, d_star, uniqueness_ratio, variant=None):
    """Rule 6: False where some d with |d - d*| > 1 has S(p,d) (100 - u) < S(p,d*) 100.  -> bool [H,W]"""
    D = S.shape[2]
    best = np.take_along_axis(S, d_star[..., None], axis=2)
    d = np.arange(D, dtype=np.int32)[None, None, :]
    far = np.abs(d - d_star[..., None]) > {"unique_gap0": 0, "unique_gap2": 2}.get(variant, 1)
    if variant == "unique_first_16":
        far = far & (d < 16)
    if variant == "unique_le":
        return ~(far & (S * (100 - int(uniqueness_ratio)) <= best * 100)).any(axis=2)
    return ~(far & (S * (100 - int(uniqueness_ratio)) < best * 100)).any(axis=2)


def right_volume(S, variant=None):
    """R(y,xr,d) = S(y, xr + d, d) where xr + d < W, 2^30 elsewhere: what the left pixels vote for the right pixel xr.  -> int32 [H,W,D]"""
    H, W, D = S.shape
    big = np.int32(1 << 30)
    R = np.full((H, W, D), big, np.int32)
    for d in range(min(D, W)):
        R[:, :W - d, d] = S[:, d:, d]
    if variant in ("dr_same_tile", "dr_without_right_tile"):
        xr = np.arange(W, dtype=np.int32)[:, None]
        tile_of_vote = (xr + np.arange(D, dtype=np.int32)[None, :]) // WIN_TILE
        lost = tile_of_vote != xr // WIN_TILE if variant == "dr_same_tile" else tile_of_vote == xr // WIN_TILE + 1
        R[:, lost] = big
    return R


def right_disparity(S, variant=None):
    """Rule 7, first part: dR(y,xr) = the smallest d attaining the minimum of S(y, xr + d, d) over xr + d < W.  -> int32 [H,W]"""
    R = right_volume(S, variant)
    if variant == "dr_tie_largest":
        return (S.shape[2] - 1 - R[..., ::-1].argmin(axis=2)).astype(np.int32)
    return R.argmin(axis=2).astype(np.int32)


def left_right_consistent(d_star, d_right, max_diff, variant=None):
    """Rule 7: False where x - d* < 0 or |dR(y, x - d*) - d*| > max_diff; all True for a negative max_diff.  -> bool [H,W]"""
    H, W = d_star.shape
    if max_diff < 0:
        return np.ones((H, W), bool)
    xr = np.arange(W, dtype=np.int32)[None, :] - d_star
    ok = xr >= 0
    if variant == "lr_clamped":
        ok = np.ones((H, W), bool)
    dr = np.take_along_axis(d_right, np.clip(xr, 0, W - 1), axis=1)
    if variant == "lr_strict":
        return ok & (np.abs(dr - d_star) < int(max_diff))
    return ok & (np.abs(dr - d_star) <= int(max_diff))


def _cdiv(a, b):
    """C division of integer arrays: truncates toward zero (b > 0)."""
    return np.where(a >= 0, a // b, -((-a) // b))


def subpixel_terms(S, d_star):
    """-> (numerator, denominator) of rule 8's offset: (S(d*-1) - S(d*+1)) 16 + den and 2 den, the neighbours clamped to [0, D)."""
    D = S.shape[2]
    dm = np.clip(d_star - 1, 0, D - 1)[..., None]
    dp = np.clip(d_star + 1, 0, D - 1)[..., None]
    s0 = np.take_along_axis(S, d_star[..., None], axis=2)[..., 0]
    sm = np.take_along_axis(S, dm, axis=2)[..., 0]
    sp = np.take_along_axis(S, dp, axis=2)[..., 0]
    # (for 0 < d* < D-1 the max() never binds: d* is the smallest minimiser, so S(d*-1) > S(d*) and S(d*+1) >= S(d*): den >= 1)
    den = np.maximum(sm + sp - 2 * s0, 1)
    return (sm - sp) * 16 + den, 2 * den


def subpixel(S, d_star, variant=None):
    """Rule 8: d16 in sixteenths; the parabola offset for 0 < d* < D-1, 16 d* otherwise.  -> int32 [H,W]"""
    D = S.shape[2]
    inner = (d_star > 0) & (d_star < D - 1)
    if variant == "subpixel_at_ends":
        inner = np.ones_like(inner)
    num, den2 = subpixel_terms(S, d_star)
    off = num // den2 if variant == "subpixel_floor" else _cdiv(num, den2)
    return (16 * d_star + np.where(inner, off, 0)).astype(np.int32)


def disparity_out(d16, valid):
    """Rule 9: int16, d16 where valid, -16 elsewhere."""
    return np.where(valid, d16, INVALID_D16).astype(np.int16)


def depth_out(disparity16, bf, min_depth=0.0, max_depth=np.inf, variant=None):
    """Rule 10: depth = (bf * 16f) / float(d16), one float32 multiply and one divide; 0 where d16 <= 0, where the result is
    < min_depth, or > max_depth when max_depth is finite.  -> float32"""
    d16 = np.asarray(disparity16).astype(np.int32)
    num = np.float32(bf) * np.float32(16.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (num / np.where(d16 > 0, d16, 1).astype(np.float32)).astype(np.float32)
    out = np.where(d16 > 0, q, np.float32(0.0)).astype(np.float32)
    if variant == "depth_min_le":
        out[out <= np.float32(min_depth)] = 0.0
    else:
        out[out < np.float32(min_depth)] = 0.0
    if np.isfinite(max_depth) and variant != "depth_max_inf":
        out[out > np.float32(max_depth)] = 0.0
    return out


def volume(left, right, num_disparities=128, p1=10, p2=120, paths=8, variant=None, **_):
    """Rules 1 to 4.  -> S int32 [H,W,D]"""
    D = int(num_disparities)
    assert D % 16 == 0 and 16 <= D <= 256, D
    assert np.shape(left) == np.shape(right)
    C = cost_volume(census(grey(left, variant), variant), census(grey(right, variant), variant), D, variant)
    return aggregate(C, int(p1), int(p2), int(paths), variant)


def finish(S, uniqueness_ratio=15, max_diff=1, bf=None, min_depth=0.0, max_depth=np.inf, variant=None, **_):
    """Rules 5 to 10 on a given S.  -> (disparity int16 [H,W], depth float32 [H,W] or None when bf is None)"""
    assert 0 <= uniqueness_ratio <= 99, uniqueness_ratio
    d_star = winner(S, variant)
    valid = unique(S, d_star, uniqueness_ratio, variant) & left_right_consistent(d_star, right_disparity(S, variant), int(max_diff), variant)
    disp = disparity_out(subpixel(S, d_star, variant), valid)
    depth = None if bf is None else depth_out(disp, bf, min_depth, max_depth, variant)
    return disp, depth


def stereo_sgm(left, right, num_disparities=128, p1=10, p2=120, uniqueness_ratio=15, max_diff=1, paths=8, bf=None, min_depth=0.0,
               max_depth=np.inf, return_volume=False, variant=None):
    """-> (disparity int16 [H,W], depth float32 [H,W] or None when bf is None) [, S]"""
    S = volume(left, right, num_disparities, p1, p2, paths, variant)
    disp, depth = finish(S, uniqueness_ratio, max_diff, bf, min_depth, max_depth, variant)
    return (disp, depth, S) if return_volume else (disp, depth)


EVENTS = (
    "m_row0", "m_row1", "m_row2", "m_row3",          # M(q) attained by one d only, in that row of 16 lanes
    "m_slot0", "m_slot1", "m_slot2", "m_slot3",      # ... in that slot of its lane
    "valid_row0", "valid_row1", "valid_row2", "valid_row3",  # a valid pixel's d* in that row of 16 lanes
    "valid_d_ge_16",         # a valid pixel's d* found by a later iteration of the winner's loop
    "valid_d0", "valid_dlast",  # a valid pixel with d* = 0, D-1
    "dstar_tie",             # min S attained by more than one d
    "dr_tie",                # the right pixel's minimum attained by more than one d
    "dr_from_right_tile",    # dR comes from a left pixel of the tile to the right of the right pixel's
    "dr_from_left_tile",     # ... to the left: impossible, the voter is x = xr + d >= xr
    "unique_rejects",        # rule 6 rejects
    "unique_equality",       # a valid pixel, some far d with S(d) (100 - u) == S(d*) 100, S(d*) > 0
    "winner_left_of_image",  # rule 6 holds and x - d* < 0
    "lr_diff_eq_max", "lr_diff_eq_max_plus_1",  # rule 6 holds, x - d* >= 0, |dR - d*| = max_diff, max_diff + 1
    "subpixel_negative_inexact",  # a valid pixel, 0 < d* < D-1, the numerator negative and no multiple of the denominator
    "depth_eq_min", "depth_eq_max",  # a depth that equals the cut
)


def events(left, right, num_disparities=128, p1=10, p2=120, uniqueness_ratio=15, max_diff=1, paths=8, bf=None, min_depth=0.0,
           max_depth=np.inf):
    """How often the input reaches the places where the wrong readings differ from the right one: {name of EVENTS: count}, counted
    on the restatement's own per-path L and S (the m_* counts are steps q -> p, summed over the paths; the others are pixels)."""
    D = int(num_disparities)
    vpl = values_per_lane(D)
    n = dict.fromkeys(EVENTS, 0)
    C = cost_volume(census(grey(left)), census(grey(right)), D)
    H, W, _ = C.shape
    S = np.zeros_like(C)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for dx, dy in DIRECTIONS[:int(paths)]:
        L = aggregate_path(C, dx, dy, int(p1), int(p2))
        S += L
        has_p = (x + dx >= 0) & (x + dx < W) & (y + dy >= 0) & (y + dy < H)  # q has a successor: its M(q) is used
        M = L.min(axis=2)
        alone = has_p & ((L == M[..., None]).sum(axis=2) == 1)
        at = L.argmin(axis=2)
        for r in range(4):
            n[f"m_row{r}"] += int((alone & (at // (16 * vpl) == r)).sum())
            n[f"m_slot{r}"] += int((alone & (at % vpl == r)).sum()) if r < vpl else 0
    d_star = winner(S)
    s_best = S.min(axis=2)
    uniq = unique(S, d_star, uniqueness_ratio)
    R = right_volume(S)
    d_right = R.argmin(axis=2).astype(np.int32)
    valid = uniq & left_right_consistent(d_star, d_right, int(max_diff))
    for r in range(4):
        n[f"valid_row{r}"] = int((valid & (d_star // (16 * vpl) == r)).sum())
    n["valid_d_ge_16"] = int((valid & (d_star >= 16)).sum())
    n["valid_d0"], n["valid_dlast"] = int((valid & (d_star == 0)).sum()), int((valid & (d_star == D - 1)).sum())
    n["dstar_tie"] = int(((S == s_best[..., None]).sum(axis=2) > 1).sum())
    n["dr_tie"] = int(((R == R.min(axis=2)[..., None]).sum(axis=2) > 1).sum())
    tile_of_vote, tile = (x + d_right) // WIN_TILE, x // WIN_TILE
    n["dr_from_right_tile"], n["dr_from_left_tile"] = int((tile_of_vote > tile).sum()), int((tile_of_vote < tile).sum())
    n["unique_rejects"] = int((~uniq).sum())
    far = np.abs(np.arange(D, dtype=np.int32)[None, None, :] - d_star[..., None]) > 1
    equal = (far & (S * (100 - int(uniqueness_ratio)) == s_best[..., None] * 100)).any(axis=2)
    n["unique_equality"] = int((valid & equal & (s_best > 0)).sum())
    n["winner_left_of_image"] = int((uniq & (x - d_star < 0)).sum())
    if max_diff >= 0:
        diff = np.abs(np.take_along_axis(d_right, np.clip(x - d_star, 0, W - 1), axis=1) - d_star)
        seen = uniq & (x - d_star >= 0)
        n["lr_diff_eq_max"], n["lr_diff_eq_max_plus_1"] = int((seen & (diff == max_diff)).sum()), int((seen & (diff == max_diff + 1)).sum())
    num, den2 = subpixel_terms(S, d_star)
    n["subpixel_negative_inexact"] = int((valid & (d_star > 0) & (d_star < D - 1) & (num < 0) & (num % den2 != 0)).sum())
    if bf is not None:
        depth = depth_out(disparity_out(subpixel(S, d_star), valid), bf)
        n["depth_eq_min"] = int(((depth > 0) & (depth == np.float32(min_depth))).sum())
        n["depth_eq_max"] = int(((depth > 0) & (depth == np.float32(max_depth))).sum())
    return n
