"""The speckle filter of hv_filter_speckles (include/hipvol.h, rules S1 - S7), restated in plain numpy - twice, independently:
    labels_flood   breadth-first flood fill from every unlabelled valid pixel in row-major order, the way cv2.filterSpeckles does it
    labels_union   union-find over the list of linked neighbour pairs (hooking the larger root under the smaller, pointer jumping)
tests/test_speckle_reference_cpu.py holds the two to each other on every planted case of tests/speckle_cases.py; the GPU is held to
filter_speckles() bit for bit (tests/test_gpu_speckle.py).

The flood fill takes variant=<name>: the WRONG readings listed in VARIANTS, the ways the rules can be misread or a kernel can go
wrong.  variant=None is the right reading.  The CPU test proves that named cases tell each of them from the right reading.

TILE_W x TILE_H is the tile of pyslam_amd/csrc/hv_speckle.hip's k_sp_local (SP_TILE_W, SP_TILE_H): the test shapes are stated in
terms of it, so that regions lie inside a tile, across a seam and around a corner of four tiles."""
import collections

import numpy as np

TILE_W, TILE_H = 64, 16
INVALID_D16 = -16  # new_val of a disparity image: stereo_reference.INVALID_D16

VARIANTS = (
    "connect8",        # S2 over the 8 neighbours
    "seed_diff",       # S2 against the region's first pixel instead of the neighbour
    "link_lt",         # S2 with <
    "remove_lt",       # S6 with <
    "diff_wraps",      # S2's int16 difference taken in int16
    "invalid_links",   # S2 without its "both are valid"
    "label_largest",   # S4 with the largest index
    "size_16bit",      # S5 kept in 16 bits
)

Result = collections.namedtuple("Result", "image depth labels stats")
STATS = ("valid_pixels", "components", "largest", "removed_components", "removed_pixels")


def default_new_val(image):
    return float(INVALID_D16) if np.asarray(image).dtype == np.int16 else 0.0


def _typed(image, new_val, max_diff):
    """-> (image as int16 or float32 [H,W], new_val and max_diff of the image's type)"""
    a = np.asarray(image)
    if a.dtype == np.int16:
        assert float(new_val) == int(new_val) and -32768 <= int(new_val) <= 32767
        return a, np.int16(int(new_val)), int(np.floor(max_diff))
    assert a.dtype == np.float32, a.dtype
    return a, np.float32(new_val), np.float32(max_diff)


def valid_mask(image, new_val):
    """S1"""
    a, nv, _ = _typed(image, new_val, 0)
    return a != nv  # (NaN != x is True; -0.0 != 0.0 is False)


def near(a, b, max_diff, variant=None):
    """S2's |a - b| <= max_diff for arrays (or scalars) of one type; says nothing about validity."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.int16:
        if variant == "diff_wraps":
            with np.errstate(over="ignore"):
                d = np.abs((a - b).astype(np.int16)).astype(np.int32)  # abs(-32768) stays -32768
        else:
            d = np.abs(a.astype(np.int32) - b.astype(np.int32))
        return d < max_diff if variant == "link_lt" else d <= max_diff
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)  # float32 throughout; NaN for NaN operands and inf - inf
        return d < max_diff if variant == "link_lt" else d <= max_diff


def _steps(variant):
    return ((0, 1), (1, 0), (0, -1), (-1, 0)) + (((1, 1), (1, -1), (-1, 1), (-1, -1)) if variant == "connect8" else ())


def labels_flood(image, new_val, max_diff, variant=None):
    """S3 and S4 by flood fill.  -> (labels int32 [H,W], -1 = invalid; valid bool [H,W]; the labels before the -1s went in)"""
    a, nv, md = _typed(image, new_val, max_diff)
    H, W = a.shape
    valid = a != nv
    member = np.ones_like(valid) if variant == "invalid_links" else valid
    flat = a.ravel()
    labels = np.full(H * W, -1, np.int64)
    taken = ~member.ravel()
    for seed in np.flatnonzero(member.ravel()):
        if taken[seed]:
            continue
        taken[seed] = True
        region, front = [np.array([seed])], np.array([seed])
        while front.size:
            fy, fx = front // W, front % W
            found = []
            for dy, dx in _steps(variant):
                y, x = fy + dy, fx + dx
                ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
                src, dst = front[ok], (y * W + x)[ok]
                ok = ~taken[dst] & near(flat[dst], flat[seed] if variant == "seed_diff" else flat[src], md, variant)
                found.append(dst[ok])
            front = np.unique(np.concatenate(found))
            taken[front] = True
            region.append(front)
        region = np.concatenate(region)
        labels[region] = region.max() if variant == "label_largest" else region.min()
    every = labels.reshape(H, W)  # (the invalid_links reading labels the invalid pixels of a region too)
    return np.where(valid, every, -1).astype(np.int32), valid, every


def labels_union(image, new_val, max_diff):
    """S3 and S4 by union-find over the linked pairs.  -> (labels int32 [H,W], valid bool [H,W])"""
    a, nv, md = _typed(image, new_val, max_diff)
    H, W = a.shape
    valid = a != nv
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    right = valid[:, :-1] & valid[:, 1:] & near(a[:, :-1], a[:, 1:], md)
    down = valid[:-1] & valid[1:] & near(a[:-1], a[1:], md)
    u = np.concatenate([idx[:, :-1][right], idx[:-1][down]])
    v = np.concatenate([idx[:, 1:][right], idx[1:][down]])
    parent = np.arange(H * W, dtype=np.int64)
    while True:
        ru, rv = parent[u], parent[v]  # roots: parent is flat at the top of every round
        open_ = ru != rv
        if not open_.any():
            break
        np.minimum.at(parent, np.maximum(ru, rv)[open_], np.minimum(ru, rv)[open_])
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    return np.where(valid, parent.reshape(H, W), -1).astype(np.int32), valid


def filter_speckles(image, max_speckle_size, max_diff, new_val=None, depth=None, variant=None, method="flood"):
    """S1 - S7.  -> Result(image, depth or None, labels int32, stats dict); the inputs are not written."""
    assert int(max_speckle_size) >= 0 and np.isfinite(max_diff) and max_diff >= 0
    new_val = default_new_val(image) if new_val is None else new_val
    a, nv, _ = _typed(image, new_val, max_diff)
    if method == "union":
        assert variant is None
        labels, valid = labels_union(a, new_val, max_diff)
    else:
        labels, valid, every = labels_flood(a, new_val, max_diff, variant)
    n = a.size
    if variant == "invalid_links":  # the regions hold invalid pixels too
        count = np.bincount(every.ravel(), minlength=n)
        size_of_pixel = count[every]
        roots = np.zeros(n, bool)
        roots[np.unique(every[valid])] = True
        sizes_at_roots = count[roots]
    else:
        count = np.bincount(labels[valid].astype(np.int64), minlength=n)
        size_of_pixel = np.where(valid, count[np.where(valid, labels, 0)], 0)
        sizes_at_roots = count[count > 0]
    if variant == "size_16bit":
        size_of_pixel, sizes_at_roots = size_of_pixel & 0xffff, sizes_at_roots & 0xffff
    small = (lambda s: s < max_speckle_size) if variant == "remove_lt" else (lambda s: s <= max_speckle_size)
    gone = valid & small(size_of_pixel)
    out = a.copy()
    out[gone] = nv
    out_depth = None
    if depth is not None:
        out_depth = np.array(depth, np.float32, copy=True)
        assert out_depth.shape == a.shape
        out_depth[gone] = np.float32(0.0)
    stats = dict(valid_pixels=int(valid.sum()), components=int(sizes_at_roots.size), largest=int(sizes_at_roots.max()) if sizes_at_roots.size else 0,
                 removed_components=int(small(sizes_at_roots).sum()), removed_pixels=int(gone.sum()))
    return Result(out, out_depth, labels, stats)


def same_bits(a, b):
    """Two arrays of one shape and type hold the same bits (float32: NaN payloads and the sign of zero included)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return bool(np.array_equal(a, b))


def stats_tuple(stats):
    return tuple(int(stats[k] if isinstance(stats, dict) else getattr(stats, k)) for k in STATS)
