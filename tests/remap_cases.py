"""Planted maps and images for hv_remap and the rectify step (tests/remap_reference.py states the contract) - test infrastructure,
no GPU.  One thread owns one output pixel, so the images are tiny: SHAPES (H, W) are one pixel, one row, one column, 5x7, exactly one
workgroup (16x16), 257 pixels in a row (one workgroup and one pixel) and 17x31 (527 pixels: a partial last workgroup, no multiple of
64).  None but 16x16 is square: a row stride of H, or map_x taken for map_y, cannot hide.

maps() lists every named case; each family says what it plants.  images name the pixel values that kernels get wrong.
"""
import collections
import functools

import numpy as np

F32 = np.float32
SHAPES = ((1, 1), (1, 9), (9, 1), (5, 7), (16, 16), (1, 257), (17, 31))
Case = collections.namedtuple("Case", "name family H W map_x map_y")

NONFINITE = (float("nan"), float("inf"), float("-inf"), 3e9, -3e9)
# just inside / outside int32 after the multiplication by 32 (float32 spacing is 4 below 2^26, 8 above), and for nearest
EDGE = (67108860.0, 67108864.0, -67108864.0, -67108872.0, 2147483520.0, 2147483648.0, -2147483648.0, -2147483904.0)


def _identity(H, W):
    yy, xx = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    return np.ascontiguousarray(xx), np.ascontiguousarray(yy)


def _cycled(H, W, xs, ys, transposed=False):
    """Pixel i takes xs[i % n] and ys[(i // n + i) % m]: both lists are run through from the first pixel on, and every (x, y) pair
    occurs where H W >= n m (n + 1 and m have no common factor for the lists used here).  transposed: the roles swapped."""
    i = np.arange(H * W)
    xs, ys = np.asarray(xs, F32), np.asarray(ys, F32)
    if transposed:
        ax, ay = (i // len(ys) + i) % len(xs), i % len(ys)
    else:
        ax, ay = i % len(xs), (i // len(xs) + i) % len(ys)
    return xs[ax].reshape(H, W), ys[ay].reshape(H, W)


def nearest_tie_values(n):
    """k + 0.5 for even and odd k, on both sides of 0 and of n - 1."""
    return [-1.5, -0.5, 0.5, 1.5, 2.5, n - 1.5, n - 0.5, n + 0.5]


def linear_tie_ks(n):
    """k with 32 v = k + 0.5: even and odd, negative, around the last pixel."""
    return [-33, -32, -2, -1, 0, 1, 2, 3, 32 * (n - 1) - 1, 32 * (n - 1), 32 * (n - 1) + 1, 32 * n - 1]


def border_values(n):
    """In (-1, 0), on pixel 0, inside with a fraction, on the last pixel, in (n-1, n)."""
    return [-0.75, -0.25, 0.0, 0.40625 if n > 1 else 0.0, float(n - 1), n - 1 + 0.25, n - 1 + 0.75]


def _sprinkle(H, W, values):
    """Identity maps with each value in map_x only, in map_y only, in both - spread over the image, as many as fit."""
    mx, my = _identity(H, W)
    trios = [(v, where) for v in values for where in ("x", "y", "xy")]
    step = max(1, (H * W) // len(trios))
    for k, (v, where) in enumerate(trios[: H * W]):
        y, x = divmod(k * step, W)
        if "x" in where:
            mx[y, x] = v
        if "y" in where:
            my[y, x] = v
    return mx, my


@functools.lru_cache(maxsize=None)
def maps():
    out = []

    def add(name, family, H, W, mx, my):
        mx, my = np.ascontiguousarray(mx, F32), np.ascontiguousarray(my, F32)
        assert mx.shape == my.shape == (H, W)
        mx.setflags(write=False), my.setflags(write=False)
        out.append(Case(f"{name}_{H}x{W}", family, H, W, mx, my))

    rng = np.random.default_rng(20240)
    for H, W in SHAPES:
        mx, my = _identity(H, W)
        add("identity", "identity", H, W, mx, my)
        add("border", "border", H, W, *_cycled(H, W, border_values(W), border_values(H)))
        perm = rng.permutation(H * W)
        add("permutation", "permutation", H, W, (perm % W).reshape(H, W), (perm // W).reshape(H, W))
        add("nonfinite", "nonfinite", H, W, *_sprinkle(H, W, NONFINITE))
    for H, W in ((1, 9), (9, 1), (5, 7), (17, 31)):
        mx, my = _identity(H, W)
        add("shift_in", "shift", H, W, mx + 1, my - 1 if H > 1 else my)
    mx, my = _identity(5, 7)
    add("shift_out_x", "shift", 5, 7, mx + 9, my)
    add("shift_out_y", "shift", 5, 7, mx, my - 6)
    for H, W in ((1, 1), (1, 9), (9, 1), (5, 7), (17, 31)):
        for t in (False, True):
            tag = "_t" if t else ""
            add("nearest_ties" + tag, "nearest_ties", H, W, *_cycled(H, W, nearest_tie_values(W), nearest_tie_values(H), t))
            add("linear_ties" + tag, "linear_ties", H, W,
                *_cycled(H, W, [(k + 0.5) / 32 for k in linear_tie_ks(W)], [(k + 0.5) / 32 for k in linear_tie_ks(H)], t))
    for q in range(4):  # all 32 x 32 (fx, fy) pairs once, 256 to a workgroup, every tap inside
        i = np.arange(256)
        n = q * 256 + i
        add(f"fxfy_q{q}", "fxfy", 16, 16, ((i % 15) + (n % 32) / 32.0).reshape(16, 16), (((i // 16) % 15) + (n // 32) / 32.0).reshape(16, 16))
    for H, W in ((5, 7), (1, 257), (17, 31)):
        add("int32_edge", "int32_edge", H, W, *_sprinkle(H, W, EDGE))
    return tuple(out)


def case(name):
    return {c.name: c for c in maps()}[name]


@functools.lru_cache(maxsize=None)
def camera_maps(H, W):
    """The maps a fused camera of H x W is rectified with: name -> (map_x, map_y).  permutation: whole pixels, every one from
    elsewhere; half_pixel: colour blends two and four neighbours, depth ties; border: fractions on every side and corner;
    nonfinite: NaN, +-inf, +-3e9 in x, in y and in both - depth 0 there, nothing is fused."""
    rng = np.random.default_rng([H, W, 7])
    perm = rng.permutation(H * W)
    mx, my = _identity(H, W)
    half_y = my + np.where(np.arange(W)[None] % 2 == 0, F32(0.25), F32(0.0)).astype(F32)
    out = {"permutation": ((perm % W).reshape(H, W).astype(F32), (perm // W).reshape(H, W).astype(F32)),
           "half_pixel": (mx + F32(0.5), half_y), "border": _cycled(H, W, border_values(W), border_values(H)),
           "nonfinite": _sprinkle(H, W, NONFINITE)}
    for pair in out.values():
        for m in pair:
            m.setflags(write=False)
    return out


IMAGE_KINDS = ("u8", "u8_white", "i32", "u16", "f32_exact", "f32_random", "f32_special")


@functools.lru_cache(maxsize=None)
def image(kind, H, W, C=1):
    """Read-only [H,W] (C == 1) or [H,W,C].
    u8          random, with 0 and 255 planted       u8_white    all 255: any blend of inside taps is 255
    i32         random over all of int32, with 2^24+1, -1, INT32_MIN, INT32_MAX (no float32 keeps 2^24+1)
    u16         random over all of uint16, with 32768 and 65535 (no int16 keeps them)
    f32_exact   integers in (-2^13, 2^13): float32 interpolation is exact (remap_reference.is_exact_image)
    f32_random  both signs, magnitudes 1e-30 .. 1e30      f32_special  NaN, +-inf and -0.0 among ordinary values"""
    rng = np.random.default_rng([IMAGE_KINDS.index(kind), H, W, C])
    shape = (H, W) if C == 1 else (H, W, C)
    n = H * W * C

    def planted(a, values):
        flat = a.reshape(-1)
        at = rng.permutation(n)[: len(values)]
        flat[at] = values[: len(at)]
        return a

    if kind == "u8":
        a = planted(rng.integers(0, 256, shape).astype(np.uint8), np.array([255, 0, 255, 0], np.uint8))
    elif kind == "u8_white":
        a = np.full(shape, 255, np.uint8)
    elif kind == "i32":
        a = planted(rng.integers(-(1 << 31), 1 << 31, shape).astype(np.int32), np.array([(1 << 24) + 1, -1, -(1 << 31), (1 << 31) - 1], np.int32))
    elif kind == "u16":
        a = planted(rng.integers(0, 1 << 16, shape).astype(np.uint16), np.array([32768, 65535, 32767, 0], np.uint16))
    elif kind == "f32_exact":
        a = planted(rng.integers(-(1 << 13) + 1, 1 << 13, shape).astype(F32), np.array([8191, -8191], F32))
    elif kind == "f32_random":
        a = (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-30, 30, shape)).astype(F32)
    elif kind == "f32_special":
        a = planted(rng.normal(0, 100, shape).astype(F32), np.array([np.nan, -0.0, np.inf, -np.inf], F32))
    else:
        raise KeyError(kind)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def batch(B, H, W, u16):
    """depth [B,H,W] (uint16 with every value above 32767, or float32), rgb [B,H,W,3]: every frame differs from every other in
    every pixel and channel.  Depths are a slanted plane around 1 m (u16: around 40000, for depth_scale 40000), so that the frames
    can also be fused."""
    assert B <= 8
    i = np.arange(H * W).reshape(H, W)
    steps = (i * 5) % 7
    if u16:
        depth = np.stack([(40000 + 700 * f + 90 * steps).astype(np.uint16) for f in range(B)])
        assert depth.min() > 32767
    else:
        depth = np.stack([(1.0 + 0.0175 * f + 0.00225 * steps).astype(F32) for f in range(B)])
    rng = np.random.default_rng([B, H, W])
    base = rng.integers(0, 256, (H, W, 3))
    base[0, 0], base[-1, -1] = 255, 0
    rgb = np.stack([((base + 31 * f) % 256).astype(np.uint8) for f in range(B)])
    for a in (depth, rgb):
        for f in range(B):
            for g in range(f):
                assert (a[f] != a[g]).all()
    depth.setflags(write=False), rgb.setflags(write=False)
    return depth, rgb
