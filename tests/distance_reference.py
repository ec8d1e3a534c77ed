"""numpy restatement of the TSDF distance field (include/hipvol.h, hv_tsdf_distance_field) on a dump() tuple - test infrastructure, no
GPU, never touches the library.

Everything up to the square root is integer arithmetic on squared voxel distances, so the outputs here and the library's agree bit
for bit with no fragile points: the states come from comparisons of the dump's own float32 values, the transform is three windowed
min-plus passes over int64, and the distance is one float32 square root and one float32 product.
"""
import numpy as np

R16 = 16
UNKNOWN, FREE, INSIDE, SITE = 0, 1, 2, 4
INF = np.int64(1) << 40
MAX_SHAPE, MAX_RADIUS = 4096, 1024


def states(dump, lo, shape, weight_threshold=0.0):
    """State (UNKNOWN / FREE / INSIDE) of the voxels lo + [0, shape) of the map, uint8 [shape]: the units of the dump that meet the
    range are copied in, everything else is UNKNOWN."""
    keys, tsdf, weight = np.asarray(dump[0], np.int64).reshape(-1, 3), np.asarray(dump[1], np.float32), np.asarray(dump[2], np.float32)
    lo, shape = np.asarray(lo, np.int64), np.asarray(shape, np.int64)
    out = np.zeros(tuple(shape), np.uint8)
    hi = lo + shape  # exclusive
    for row, key in enumerate(keys):
        v0 = key * R16
        a, b = np.maximum(v0, lo), np.minimum(v0 + R16, hi)
        if np.any(a >= b):
            continue
        src = tuple(slice(int(a[d] - v0[d]), int(b[d] - v0[d])) for d in range(3))
        dst = tuple(slice(int(a[d] - lo[d]), int(b[d] - lo[d])) for d in range(3))
        t = tsdf[row].reshape(R16, R16, R16)[src]  # dump order: x * 256 + y * 16 + z
        w = weight[row].reshape(R16, R16, R16)[src]
        with np.errstate(invalid="ignore"):
            out[dst] = np.where(w.astype(np.float64) > np.float64(weight_threshold), np.where(t <= np.float32(0), INSIDE, FREE), UNKNOWN)
    return out


def classify(dump, origin, shape, weight_threshold=0.0):
    """cls uint8 [shape]: the state, with SITE OR-ed on where one of the six axis neighbours in the MAP (inside the box or not) is
    observed and of the other state."""
    origin, shape = np.asarray(origin, np.int64), np.asarray(shape, np.int64)
    ext = states(dump, origin - 1, shape + 2, weight_threshold)
    core = tuple(slice(1, 1 + int(n)) for n in shape)
    s = ext[core]
    other = np.where(s == UNKNOWN, np.uint8(255), s ^ np.uint8(3))
    site = np.zeros(s.shape, bool)
    for axis in range(3):
        for step in (-1, 1):
            sl = list(core)
            sl[axis] = slice(1 + step, 1 + step + int(shape[axis]))
            site |= ext[tuple(sl)] == other
    return (s | np.where(site, np.uint8(SITE), np.uint8(0))).astype(np.uint8)


def window_pass(g, axis, radius):
    """out(i) = min over |i' - i| <= radius of g(i') + (i - i')^2 along `axis` (int64; INF = no value)."""
    g = np.moveaxis(g, axis, 0)
    out = g.copy()
    for k in range(1, min(int(radius), g.shape[0] - 1) + 1):
        kk = np.int64(k * k)
        np.minimum(out[k:], g[:-k] + kk, out=out[k:])
        np.minimum(out[:-k], g[k:] + kk, out=out[:-k])
    return np.moveaxis(out, 0, axis)


def transform(site, radius):
    """dist2 uint32 [shape] of a boolean site grid: the three windowed passes along x, y, z, then the cap at radius^2."""
    g = np.where(site, np.int64(0), INF)
    for axis in range(3):
        g = window_pass(g, axis, radius)
    return np.minimum(g, np.int64(radius) * np.int64(radius)).astype(np.uint32)


def brute_force(site, radius):
    """The same by definition: every cell against every site of the box, capped at radius^2."""
    shape = site.shape
    cells = np.stack(np.meshgrid(*(np.arange(n, dtype=np.int64) for n in shape), indexing="ij"), -1).reshape(-1, 3)
    sites = cells[site.reshape(-1)]
    best = np.full(len(cells), np.int64(radius) * np.int64(radius), np.int64)
    for s in sites:
        np.minimum(best, ((cells - s) ** 2).sum(axis=1), out=best)
    return best.reshape(shape).astype(np.uint32)


def finish(cls, dist2, voxel_length, radius):
    """-> distance float32, stats (unknown, free, inside, sites, far)."""
    root = np.sqrt(dist2.astype(np.float32))  # correctly rounded; sqrt(0) = 0
    sign = np.where((cls & 3) == INSIDE, np.float32(-1), np.float32(1))
    distance = (sign * (root * np.float32(voxel_length))).astype(np.float32)
    state = cls & 3
    stats = (int((state == UNKNOWN).sum()), int((state == FREE).sum()), int((state == INSIDE).sum()), int(((cls & SITE) != 0).sum()),
             int((dist2 == np.uint32(radius * radius)).sum()))
    return distance, stats


def distance_field(dump, voxel_length, origin, shape, radius, weight_threshold=0.0, cls=None):
    """-> dict of distance f32, dist2 u32, cls u8 (each [shape]) and stats, for the box origin + [0, shape) of the dump's map.
    cls: a classify() result of the same box and threshold to reuse."""
    assert all(1 <= int(n) <= MAX_SHAPE for n in shape) and 1 <= int(radius) <= MAX_RADIUS
    if cls is None:
        cls = classify(dump, origin, shape, weight_threshold)
    dist2 = transform((cls & SITE) != 0, radius)
    distance, stats = finish(cls, dist2, voxel_length, radius)
    return {"distance": distance, "dist2": dist2, "cls": cls, "stats": stats}
