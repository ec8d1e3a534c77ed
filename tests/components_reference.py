"""numpy restatement of the surface components of the TSDF map (include/hipvol.h, hv_tsdf_surface_components and
hv_tsdf_remove_components) on a dump() tuple - test infrastructure, no GPU, never touches the library.

Every definition is integer, so the outputs here and the library's agree bit for bit: the sites are tests/distance_reference.classify's
over a box that covers the map plus one voxel, the labelling is a plain union-find over the site list (hooking to the smaller root and
pointer jumping to a fixed point), the numbering is by the lexicographically smallest site, and the removal rule is the Chebyshev test
of the contract taken literally: nearest SMALL site and nearest KEPT site in the maximum norm, per voxel - not the separable dilation
the library runs.
"""
import itertools

import numpy as np

from tests import distance_reference as dr

R16 = 16
NV = R16 ** 3
MAX_MARGIN = 16
_LOCAL = np.stack(np.meshgrid(np.arange(R16), np.arange(R16), np.arange(R16), indexing="ij"), -1).reshape(NV, 3)  # dump order
# the 13 offsets after (0, 0, 0) in (x, y, z) order: every adjacent pair once
FORWARD = tuple(o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0))


def site_coordinates(dump, weight_threshold=0.0):
    """Global voxel indices [N,3] int64 of the sites of the dump's map, in (x, y, z) order."""
    keys = np.asarray(dump[0], np.int64).reshape(-1, 3)
    if len(keys) == 0:
        return np.zeros((0, 3), np.int64)
    lo = keys.min(axis=0) * R16 - 1
    shape = (keys.max(axis=0) - keys.min(axis=0) + 1) * R16 + 2
    cls = dr.classify(dump, lo, shape, weight_threshold)
    return np.argwhere((cls & dr.SITE) != 0).astype(np.int64) + lo  # argwhere: C order = (x, y, z) order


def site_grid(coords):
    """-> (boolean grid over the sites' bounding box, its origin)."""
    lo = coords.min(axis=0)
    grid = np.zeros(tuple(coords.max(axis=0) - lo + 1), bool)
    grid[tuple((coords - lo).T)] = True
    return grid, lo


def union_find(n, a, b):
    """Roots [n] of the graph with edges (a[i], b[i]): hook every edge's larger root to the smaller, jump pointers, until nothing
    changes.  The root of a class is its smallest member."""
    parent = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        m = np.minimum(ra, rb)
        before = parent.copy()
        np.minimum.at(parent, ra, m)
        np.minimum.at(parent, rb, m)
        while True:
            jumped = parent[parent]
            if np.array_equal(jumped, parent):
                break
            parent = jumped
        if np.array_equal(parent, before):
            return parent


def label_sites(coords):
    """Component number per site of coords [N,3] (in (x, y, z) order), canonical: components numbered by their smallest site."""
    n = len(coords)
    if n == 0:
        return np.zeros(0, np.int32)
    lo = coords.min(axis=0) - 1
    shape = coords.max(axis=0) - lo + 2
    index = np.full(tuple(shape), -1, np.int64)
    index[tuple((coords - lo).T)] = np.arange(n)
    ea, eb = [], []
    for off in FORWARD:
        other = index[tuple((coords - lo + np.array(off)).T)]
        hit = other >= 0
        ea.append(np.flatnonzero(hit))
        eb.append(other[hit])
    root = union_find(n, np.concatenate(ea), np.concatenate(eb))
    # coords are sorted, so a class's root (its smallest member) IS its seed and the roots are in seed order
    roots = np.unique(root)
    return np.searchsorted(roots, root).astype(np.int32)


def components(dump, weight_threshold=0.0):
    """-> dict: seed [C,3] i32, sites [C] i64, lo, hi [C,3] i32, site_index [N,3] i32, site_label [N] i32 (rows by unit key, then dump
    order), stats (units, sites, components, largest)."""
    coords = site_coordinates(dump, weight_threshold)
    label = label_sites(coords)
    C = int(label.max()) + 1 if len(label) else 0
    seed, lo, hi = np.zeros((C, 3), np.int32), np.zeros((C, 3), np.int32), np.zeros((C, 3), np.int32)
    count = np.bincount(label, minlength=C).astype(np.int64)
    if C:
        first = np.unique(label, return_index=True)[1]  # the first row of each label in (x, y, z) order
        seed = coords[first].astype(np.int32)
        big = np.iinfo(np.int64)
        l, h = np.full((C, 3), big.max), np.full((C, 3), big.min)
        np.minimum.at(l, label, coords)
        np.maximum.at(h, label, coords)
        lo, hi = l.astype(np.int32), h.astype(np.int32)
    key, local = coords >> 4, coords & 15
    order = np.lexsort((local[:, 2], local[:, 1], local[:, 0], key[:, 2], key[:, 1], key[:, 0])) if len(coords) else np.zeros(0, np.int64)
    return {"seed": seed, "sites": count, "lo": lo, "hi": hi, "site_index": coords[order].astype(np.int32).reshape(-1, 3),
            "site_label": label[order].astype(np.int32), "stats": (len(np.asarray(dump[0]).reshape(-1, 3)), len(coords), C, int(count.max()) if C else 0)}


def _nearest_chebyshev(points, sites, limit):
    """Per point: is some site within Chebyshev distance `limit`?  The nearest site in the maximum norm (a k-d tree query with
    p = inf; the coordinates are integers, so `limit + 0.5` as an exclusive bound is exact); without scipy every point against every
    site, in chunks."""
    near = np.zeros(len(points), bool)
    if len(sites) == 0 or len(points) == 0:
        return near
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    if cKDTree is not None:
        d, _ = cKDTree(sites).query(points, k=1, p=np.inf, distance_upper_bound=limit + 0.5)
        return np.isfinite(d)
    step = max(1, (1 << 24) // len(sites))
    for i in range(0, len(points), step):
        d = np.abs(points[i:i + step, None, :] - sites[None, :, :]).max(axis=2)
        near[i:i + step] = (d <= limit).any(axis=1)
    return near


def remove_components(dump, min_sites, margin, weight_threshold=0.0, ref=None):
    """-> (the dump afterwards, stats (components, components_removed, sites, sites_removed, voxels_reset, units_changed,
    units_emptied)).  A voxel with weight > 0 is reset when it is a SMALL site, or a SMALL site lies within Chebyshev distance
    `margin` and no KEPT site does.  ref: components(dump, weight_threshold), to reuse."""
    assert min_sites >= 1 and 0 <= margin <= MAX_MARGIN
    keys, tsdf, weight, colour = (np.array(a, copy=True) for a in dump)
    ref = components(dump, weight_threshold) if ref is None else ref
    small_label = ref["sites"] < min_sites
    is_small = small_label[ref["site_label"]] if len(ref["site_label"]) else np.zeros(0, bool)
    sites = ref["site_index"].astype(np.int64)
    small, kept = sites[is_small], sites[~is_small]
    stats = [ref["stats"][2], int(small_label.sum()), ref["stats"][1], int(is_small.sum()), 0, 0, 0]
    if len(small):
        k64 = np.asarray(keys, np.int64).reshape(-1, 3)
        # only units within reach of a SMALL site can change: the rest of the map is not visited (the test stays literal per voxel)
        s_lo, s_hi = small.min(axis=0) - margin, small.max(axis=0) + margin
        for row, key in enumerate(k64):
            if np.any(key * R16 + R16 - 1 < s_lo) or np.any(key * R16 > s_hi):
                continue
            w = weight[row]
            held = np.flatnonzero(w > 0)
            if len(held) == 0:
                continue
            g = key * R16 + _LOCAL[held]
            close = lambda s: s[(np.abs(s - (key * R16 + 7.5)).max(axis=1) <= 8 + margin)]  # sites that can reach this unit
            s_near, k_near = close(small), close(kept)
            in_small = _nearest_chebyshev(g, s_near, 0)
            reset = in_small | (_nearest_chebyshev(g, s_near, margin) & ~_nearest_chebyshev(g, k_near, margin))
            n = int(reset.sum())
            if n == 0:
                continue
            at = held[reset]
            tsdf[row, at], weight[row, at], colour[row, at] = 0.0, 0.0, 0.0
            stats[4] += n
            stats[5] += 1
            stats[6] += int(not (weight[row] > 0).any())
    return (keys, tsdf, weight, colour), tuple(stats)


def empty_units(dump):
    """Keys of the units of a dump whose weights are all 0: what prune(empty=True) releases."""
    keys, weight = np.asarray(dump[0]).reshape(-1, 3), np.asarray(dump[2])
    return keys[~(weight > 0).any(axis=1)] if len(keys) else keys
