"""Planted inputs of the speckle filter, shared by the CPU and GPU tests (tests/speckle_reference.py is the restatement they are held
to).  Every case: (name, image, params) with params = dict(max_speckle_size, max_diff, new_val[, depth]).  T_W x T_H is the tile of
the labelling kernel; the regions are placed inside a tile, across its seams and around a corner where four tiles meet."""
import numpy as np

from tests.speckle_reference import TILE_H as T_H
from tests.speckle_reference import TILE_W as T_W

INV = -16   # an invalid disparity
BASE = 160  # a valid one (10 px)
EDGE_SHAPES = ((1, 1), (1, 7), (7, 1), (T_H - 1, T_W + 1), (2 * T_H + 3, 2 * T_W + 5))
BIG = (2 * T_H + 3, 2 * T_W + 5)
GRID3 = (3 * T_H, 3 * T_W)
FULL_FRAME = (480, 752)
K = 6        # the size threshold of size_threshold
MD = 16      # the difference threshold of the int16 cases: one pixel of disparity
NAN_PAYLOAD = 0x7FC12345  # a quiet NaN with a payload


def levels(H, W, seed, invalid=0.3):
    """int16 [H,W]: four levels 16 apart, about 30 % invalid"""
    rng = np.random.default_rng(seed)
    a = (BASE + 16 * rng.integers(0, 4, (H, W))).astype(np.int16)
    a[rng.random((H, W)) < invalid] = INV
    return a


def blank(shape=GRID3):
    return np.full(shape, INV, np.int16)


# (y, x) of the four-tile corner blob relative to the corner (cy, cx) = first pixel of the lower right tile: K pixels, 4-connected,
# at least one in each of the four tiles; EXTRA makes it K + 1
CORNER_BLOB = ((-1, -2), (-1, -1), (-1, 0), (0, -1), (0, 0), (0, 1))
CORNER_EXTRA = (0, 2)


def size_threshold():
    """Blobs of exactly K and K + 1 pixels: inside a tile, across a vertical seam, across a horizontal seam, around a corner.
    -> (image, {place: (pixels of the K blob, pixels of the K + 1 blob)})"""
    a = blank()
    where = {
        "inside": ([(3, x) for x in range(5, 5 + K)], [(6, x) for x in range(5, 6 + K)]),
        "vertical_seam": ([(3, x) for x in range(T_W - 3, T_W - 3 + K)], [(6, x) for x in range(T_W - 4, T_W - 3 + K)]),
        "horizontal_seam": ([(y, 20) for y in range(T_H - 3, T_H - 3 + K)], [(y, 24) for y in range(T_H - 4, T_H - 3 + K)]),
        "corner": ([(T_H + dy, T_W + dx) for dy, dx in CORNER_BLOB],
                   [(2 * T_H + dy, 2 * T_W + dx) for dy, dx in CORNER_BLOB + (CORNER_EXTRA,)]),
    }
    for small, large in where.values():
        assert len(small) == K and len(large) == K + 1
        for y, x in small + large:
            a[y, x] = BASE
    return a, where


def diff_threshold():
    """Pairs of neighbours that differ by exactly MD and by MD + 1: side by side and one above the other, inside a tile and across
    a seam.  -> (image, [(pixel, pixel, difference)])"""
    a = blank()
    pairs = [((3, 5), (3, 6), MD), ((6, 5), (6, 6), MD + 1), ((3, 10), (4, 10), MD), ((3, 14), (4, 14), MD + 1),
             ((3, T_W - 1), (3, T_W), MD), ((6, T_W - 1), (6, T_W), MD + 1), ((T_H - 1, 20), (T_H, 20), MD), ((T_H - 1, 24), (T_H, 24), MD + 1)]
    for p, q, d in pairs:
        a[p], a[q] = BASE, BASE + d
    return a, pairs


def ramp():
    """One row that rises by MD per pixel over 2 T_W + 5 pixels"""
    return (MD * np.arange(2 * T_W + 5, dtype=np.int16))[None, :].copy()


def checkerboard(shape=(T_H + 3, T_W + 5)):
    y, x = np.indices(shape)
    return np.where((x + y) % 2 == 0, BASE, INV).astype(np.int16)


def snake(shape=GRID3):
    """A one-pixel-wide path through the image between invalid walls: the even rows, joined at alternating ends by one pixel of the
    odd row between them.  -> (image, the path's pixels in order)"""
    H, W = shape
    a = blank(shape)
    path = []
    for y in range(0, H, 2):
        xs = range(W) if (y // 2) % 2 == 0 else range(W - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < H:
            path.append((y + 1, path[-1][1]))
    for p in path:
        a[p] = BASE
    return a, path


def comb(shape=GRID3):
    """Vertical teeth (the even columns) joined only by the last row"""
    a = blank(shape)
    a[:, ::2] = BASE
    a[-1, :] = BASE
    return a


def float_depth(H=T_H + 3, W=T_W + 5, seed=9):
    """A depth-like float32 image in steps of 0.25 with 0.0 (invalid), -0.0 (invalid too), NaN and +inf pixels, some of them side by
    side"""
    rng = np.random.default_rng(seed)
    a = (1.0 + 0.25 * rng.integers(0, 4, (H, W))).astype(np.float32)
    a[rng.random((H, W)) < 0.2] = 0.0
    a[2, 3] = a[2, 4] = np.nan     # two NaNs side by side never link
    a[5, 7] = a[6, 7] = np.inf     # inf - inf is NaN: neither do these
    a[9, 9] = np.nan
    a[11, 2] = np.inf
    a[4, 20] = a[4, 21] = a[8, 30] = -0.0
    a[1, T_W - 1], a[1, T_W] = 2.0, 2.25   # across the seam at exactly max_diff
    a[3, T_W - 1], a[3, T_W] = 2.0, np.float32(2.25) + np.float32(2.0 ** -21)  # and one ulp past it
    return a


def companion_depth(shape, seed=4):
    """float32 depth beside a disparity image: random, with payload NaNs and a -0.0 that must keep their bits where nothing is removed"""
    rng = np.random.default_rng(seed)
    d = (0.5 + 4.0 * rng.random(shape)).astype(np.float32)
    flat = d.ravel().view(np.uint32)
    flat[::37] = NAN_PAYLOAD
    flat[5::41] = 0x80000000
    return d


def _planted():
    cases = []

    def add(name, image, max_speckle_size, max_diff, new_val=INV, **more):
        image = np.ascontiguousarray(image)
        image.setflags(write=False)
        cases.append((name, image, dict(max_speckle_size=int(max_speckle_size), max_diff=max_diff, new_val=new_val, **more)))

    for H, W in EDGE_SHAPES:
        a = levels(H, W, seed=H * 1000 + W)
        for size in sorted({0, 1, 5, H * W}):  # (one pixel: H W = 1 is there already)
            for md in (0, 16):
                add(f"edges_{H}x{W}_s{size}_d{md}", a, size, md)
    add("size_threshold", size_threshold()[0], K, MD)
    add("diff_threshold", diff_threshold()[0], 1, MD)
    add("ramp", ramp(), 2 * T_W + 4, MD)
    add("checkerboard_s1", checkerboard(), 1, MD)
    add("checkerboard_s0", checkerboard(), 0, MD)
    s, path = snake()
    add("snake", s, len(path) - 1, MD)
    raised = s.copy()
    raised[path[len(path) // 2]] += MD + 1  # the pixel itself becomes a region of one between the two halves
    add("snake_raised", raised, len(path) // 2 - 1, MD)
    step = s.copy()
    for p in path[len(path) // 2:]:
        step[p] += MD + 1
    add("snake_step", step, len(path) // 2, MD)
    add("comb", comb(), comb().size, MD)
    flat = np.full(BIG, BASE, np.int16)
    add("one_component_kept", flat, flat.size - 1, MD)
    add("one_component_removed", flat, flat.size, MD)
    full = np.full(FULL_FRAME, BASE, np.int16)
    add("one_component_full_frame", full, full.size - 1, MD)
    ext = np.array([[-32768, 32767, 0], [5, 0, 0]], np.int16)
    add("extremes_d65535", ext, 1, 65535, new_val=0)
    add("extremes_d65534", ext, 1, 65534, new_val=0)
    add("extremes_newval_min", ext, 1, MD, new_val=-32768)
    # valid pixels within max_diff of the invalid value between them: they do not link through it
    add("near_invalid", np.array([[-8, INV, 0]], np.int16), 1, MD)
    add("float_depth", float_depth(), 2, 0.25, new_val=0.0)
    a = levels(*BIG, seed=77)
    add("companion", a, 5, MD, depth=companion_depth(a.shape))
    return cases


PLANTED = _planted()  # [(name, image, params)]
SMALL = [c for c in PLANTED if c[1].size <= GRID3[0] * GRID3[1]]


def planted(name):
    """-> (image, params) of the named case"""
    return next(c[1:] for c in PLANTED if c[0] == name)
