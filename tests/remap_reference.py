"""hv_remap and the rectify step of hv_tsdf_set_rectify_maps (include/hipvol.h), restated - test infrastructure, no GPU, no library.
Written from the header's text: every coordinate is decided by plain Python on one float32 value at a time (integers and float64),
the pixels are then fetched by flat index.  It shares no code with oracle/host_prep.py or pyslam_amd/csrc/hv_prep.hip.

COORDINATES  r = round-half-to-even(float32 v).  For linear interpolation v is first multiplied by 32 IN FLOAT32 (mul32()).  A
             coordinate that is NaN, +-inf, or whose rounded value does not fit int32 is OUTSIDE: the pixel takes the border value.
BORDER       constant 0 (0.0 for float images), for every tap that lies outside [0, H) x [0, W).
NEAREST      dst[y, x] = src[r(map_y[y, x]), r(map_x[y, x])] for uint8, float32, int32 with 1..4 interleaved channels, and uint16 with
             one (the depth of the batched rectify step).  Values are copied, never converted.
LINEAR u8    sx = r(32 map_x); ix = sx >> 5, fx = sx & 31 (arithmetic shift, two's-complement mask: floor and a non-negative
             remainder for negative sx), the same in y.  Taps (iy, ix) (iy, ix+1) (iy+1, ix) (iy+1, ix+1) with the integer weights
             w00 = (32-fx)(32-fy) 32, w01 = fx (32-fy) 32, w10 = (32-fx) fy 32, w11 = fx fy 32 (sum 2^15); (sum + 2^14) >> 15.
LINEAR f32   the same ix, fx; weights (1-fx/32)(1-fy/32) ... (multiples of 2^-10, exact in float32).  remap_linear_f32() returns the
             sum of the four products IN FLOAT64 and the bound GAMMA4 * sum_k w_k |p_k| (GAMMA4 = 4u / (1 - 4u), u = 2^-24: four
             products and three additions in float32, contracted into FMAs or not - Higham, Accuracy and Stability, lemma 3.1).
             Where every pixel is an integer with |p| < 2^13 all products and partial sums are float32 numbers and the float32
             result IS the float64 one (is_exact_image()).  NaN / inf pixels propagate as IEEE arithmetic has it: a zero weight
             times inf is NaN.
BATCH        rectify_frames(depth [B,H,W] u16|f32, rgb [B,H,W,3] u8, map_x, map_y): nearest depth, linear u8 colour, per frame.

Every function takes variant=<name>: the WRONG readings listed in VARIANTS.  tests/test_remap_reference_cpu.py proves that the
planted cases of tests/remap_cases.py tell each of them from the right reading.
"""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24
GAMMA4 = 4 * U / (1 - 4 * U)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

VARIANTS = (
    "half_away",         # rounding half away from zero
    "floor",             # floor instead of rounding
    "trunc",             # truncation instead of rounding
    "c_divmod",          # C's / and % instead of >> and & for negative sx
    "border_replicate",  # clamped border instead of 0
    "w_swapped",         # w01 and w10 swapped
    "xy_swapped",        # map_x and map_y swapped
    "no_half",           # the missing + 2^14
    "row_stride_H",      # a row stride of H instead of W
    "channel_stride_3",  # a channel stride fixed at 3
    "nan_as_zero",       # a NaN coordinate read as 0
    "via_float32",       # an int32 / uint16 value passed through float32
    "frame0_colour",     # every frame of a batch read at frame 0's colour offset
    "colour_offset_npx",  # a colour frame offset of f H W instead of f H W 3
)


def mul32(v):
    """32 v as the library evaluates it: one float32 multiplication."""
    with np.errstate(over="ignore", invalid="ignore"):
        return F32(v) * F32(32.0)


def round_coord(v, variant=None):
    """One float32 coordinate -> its integer, or None where it is outside whatever the image."""
    v = float(F32(v))
    if v != v:
        return 0 if variant == "nan_as_zero" else None
    if math.isinf(v):
        return None
    if variant == "half_away":
        r = int(math.floor(abs(v) + 0.5))
        r = -r if v < 0 else r
    elif variant == "floor":
        r = math.floor(v)
    elif variant == "trunc":
        r = int(v)
    else:
        r = round(v)  # Python rounds halves to even, exactly
    return r if INT32_MIN <= r <= INT32_MAX else None


def split5(s, variant=None):
    """sx -> (ix, fx)."""
    if variant == "c_divmod":
        q = abs(s) // 32
        q = -q if s < 0 else q
        return q, s - 32 * q
    return s >> 5, s & 31


def nearest_taps(map_x, map_y, variant=None):
    """-> y [n], x [n] int64, valid [n] bool (False: the coordinate itself is outside), row-major over the map."""
    mx, my = np.asarray(map_x, F32), np.asarray(map_y, F32)
    assert mx.shape == my.shape and mx.ndim == 2
    if variant == "xy_swapped":
        mx, my = my, mx
    ys, xs, ok = [], [], []
    for vx, vy in zip(mx.ravel(), my.ravel()):
        x, y = round_coord(vx, variant), round_coord(vy, variant)
        good = x is not None and y is not None
        ys.append(y if good else 0), xs.append(x if good else 0), ok.append(good)
    return np.array(ys, np.int64), np.array(xs, np.int64), np.array(ok, bool)


def linear_taps(map_x, map_y, variant=None):
    """-> iy, ix, fy, fx [n] int64 and valid [n]."""
    mx, my = np.asarray(map_x, F32), np.asarray(map_y, F32)
    assert mx.shape == my.shape and mx.ndim == 2
    if variant == "xy_swapped":
        mx, my = my, mx
    rows, ok = [], []
    for vx, vy in zip(mx.ravel(), my.ravel()):
        sx, sy = round_coord(mul32(vx), variant), round_coord(mul32(vy), variant)
        good = sx is not None and sy is not None
        rows.append(split5(sy, variant) + split5(sx, variant) if good else (0, 0, 0, 0))
        ok.append(good)
    t = np.array(rows, np.int64).reshape(-1, 4)
    return t[:, 0], t[:, 2], t[:, 1], t[:, 3], np.array(ok, bool)


def fetch(src, y, x, valid, variant=None):
    """src [H,W] or [H,W,C] -> [n, C] of src's dtype: the pixel at (y, x), 0 where it is outside."""
    src = np.asarray(src)
    H, W = src.shape[:2]
    C = 1 if src.ndim == 2 else src.shape[2]
    flat = src.reshape(-1)
    if variant == "border_replicate":
        y, x, inside = np.clip(y, 0, H - 1), np.clip(x, 0, W - 1), valid
    else:
        inside = valid & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    row = H if variant == "row_stride_H" else W
    step = 3 if variant == "channel_stride_3" else C
    out = np.zeros((len(y), C), src.dtype)
    for c in range(C):
        idx = (y * row + x) * step + c
        ok = inside & (idx >= 0) & (idx < flat.size)
        out[ok, c] = flat[idx[ok]]
    return out


def _through_float32(src):
    info = np.iinfo(src.dtype)
    return np.clip(src.astype(F32).astype(np.float64), info.min, info.max).astype(src.dtype)


def remap_nearest(src, map_x, map_y, variant=None):
    src = np.asarray(src)
    assert src.dtype in (np.uint8, np.float32, np.int32, np.uint16) and src.shape[:2] == np.shape(map_x)
    if variant == "via_float32" and src.dtype in (np.int32, np.uint16):
        src = _through_float32(src)
    y, x, ok = nearest_taps(map_x, map_y, variant)
    return fetch(src, y, x, ok, variant).reshape(src.shape)


def _four(src, map_x, map_y, variant):
    iy, ix, fy, fx, ok = linear_taps(map_x, map_y, variant)
    taps = [fetch(src, iy + dy, ix + dx, ok, variant) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
    return taps, fy, fx


def remap_linear_u8(src, map_x, map_y, variant=None):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.shape[:2] == np.shape(map_x)
    (p00, p01, p10, p11), fy, fx = _four(src, map_x, map_y, variant)
    w00, w01, w10, w11 = (32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32
    if variant == "w_swapped":
        w01, w10 = w10, w01
    s = sum(p.astype(np.int64) * w[:, None] for p, w in ((p00, w00), (p01, w01), (p10, w10), (p11, w11)))
    r = (s + (0 if variant == "no_half" else 1 << 14)) >> 15
    return np.clip(r, 0, 255).astype(np.uint8).reshape(src.shape)


def remap_linear_f32(src, map_x, map_y, variant=None):
    """-> (value float64, bound float64), both of src's shape.  |float32 result - value| <= bound; on an exact image the bound is
    irrelevant: the float32 result equals the value."""
    src = np.asarray(src)
    assert src.dtype == np.float32 and src.shape[:2] == np.shape(map_x)
    (p00, p01, p10, p11), fy, fx = _four(src, map_x, map_y, variant)
    gx, gy = fx / 32.0, fy / 32.0
    w00, w01, w10, w11 = (1 - gx) * (1 - gy), gx * (1 - gy), (1 - gx) * gy, gx * gy
    if variant == "w_swapped":
        w01, w10 = w10, w01
    with np.errstate(invalid="ignore"):
        terms = [p.astype(np.float64) * w[:, None] for p, w in ((p00, w00), (p01, w01), (p10, w10), (p11, w11))]
        value = ((terms[0] + terms[1]) + terms[2]) + terms[3]
        bound = GAMMA4 * sum(np.abs(t) for t in terms)
    return value.reshape(src.shape), bound.reshape(src.shape)


def is_exact_image(src):
    """Integers with |p| < 2^13: the weights are multiples of 2^-10 in [0, 1] that sum to 1, so every product and every partial sum
    is a multiple of 2^-10 of magnitude below 2^13 - at most 23 significant bits, a float32 number.  No float32 operation rounds."""
    src = np.asarray(src)
    return bool(np.isfinite(src).all() and (src == np.rint(src)).all() and (np.abs(src) < 2 ** 13).all())


def rectify_frames(depth, rgb, map_x, map_y, variant=None):
    """depth [B,H,W] uint16|float32, rgb [B,H,W,3] uint8 -> the same shapes: nearest depth, linear colour, frame by frame."""
    depth, rgb = np.asarray(depth), np.asarray(rgb)
    B, H, W = depth.shape
    assert rgb.shape == (B, H, W, 3) and rgb.dtype == np.uint8 and depth.dtype in (np.uint16, np.float32)
    npx = H * W
    flat = np.ascontiguousarray(rgb).reshape(-1)
    d_out, c_out = np.empty_like(depth), np.empty_like(rgb)
    for f in range(B):
        d_out[f] = remap_nearest(depth[f], map_x, map_y, variant)
        if variant == "frame0_colour":
            frame = rgb[0]
        elif variant == "colour_offset_npx":
            frame = flat[f * npx: f * npx + 3 * npx].reshape(H, W, 3)
        else:
            frame = rgb[f]
        c_out[f] = remap_linear_u8(frame, map_x, map_y, variant)
    return d_out, c_out
