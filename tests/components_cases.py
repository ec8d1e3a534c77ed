"""The planted maps the surface-component tests share (tests/test_components_reference_cpu.py on the CPU,
tests/test_gpu_tsdf_components.py on the GPU) - test infrastructure, no GPU.  Everything is built with tests/planted_states.py:
voxel 0.02, sdf_trunc 0.08 (a band of four voxels), fixed seeds.

Coordinates below are GLOBAL VOXEL INDICES (voxel q has its centre at (q + 0.5) * VOX; its unit is q >> 4).
"""
import functools
import itertools

import numpy as np

from tests import distance_cases as dc
from tests import planted_states as ps
from tests import sample_cases as sc

VOX, TRUNC, R16 = ps.VOX, ps.TRUNC, ps.R


def _band(distance, keys, weight=4):
    """tsdf = distance / TRUNC where |distance| <= TRUNC, nothing observed elsewhere; units without an observed voxel are dropped."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    d = distance(ps.centres(keys))
    band = np.abs(d) <= TRUNC
    keep = band.any(axis=1)
    keys, d, band = keys[keep], d[keep], band[keep]
    colour = np.random.default_rng(17).integers(0, 256, d.shape + (3,)).astype(np.float64)
    return ps.finish(keys, (d / TRUNC).astype(np.float32), np.where(band, weight, 0).astype(np.float32), colour)


def _voxels(entries):
    """entries: (global voxel index, tsdf) pairs, each observed with weight 3; every other voxel of the units they fall into is
    unobserved."""
    units = sorted({tuple(int(c) >> 4 for c in q) for q, _ in entries})
    t, w = np.zeros((len(units), ps.NV), np.float32), np.zeros((len(units), ps.NV), np.float32)
    for q, value in entries:
        row = units.index(tuple(int(c) >> 4 for c in q))
        x, y, z = (int(c) & 15 for c in q)
        t[row, (x * R16 + y) * R16 + z], w[row, (x * R16 + y) * R16 + z] = value, 3.0
    return ps.finish(np.array(units, np.int64), t, w, np.full(t.shape + (3,), 90.0))


# ---- 1. two blobs --------------------------------------------------------------------------------------------------------------
BIG_RADIUS, SMALL_RADIUS = 6, 3          # voxels
SMALL_CENTRE = (2 * R16 + 8, 8, 8)       # a lattice corner in the middle of unit (2, 0, 0): radius + band = 7 voxels stay inside it


@functools.lru_cache(maxsize=None)
def two_blobs_states():
    """A sphere of radius 6 voxels centred on the corner the eight units (-1..0)^3 share, and one of radius 3 voxels inside unit
    (2, 0, 0): two components; the second has the fewer sites."""
    big = lambda p: np.linalg.norm(p, axis=-1) - BIG_RADIUS * VOX
    small = lambda p: np.linalg.norm(p - np.array(SMALL_CENTRE) * VOX, axis=-1) - SMALL_RADIUS * VOX
    return sc.concat(_band(big, list(itertools.product((-1, 0), repeat=3))), _band(small, [(2, 0, 0)]))


# ---- 2. corner touch -----------------------------------------------------------------------------------------------------------
def _pair(inside, free):
    return [(inside, -0.5), (free, 0.5)]


@functools.lru_cache(maxsize=None)
def corner_touch_states(gap=1):
    """Two blobs of two sites each (one INSIDE voxel and its FREE +-x neighbour, nothing else observed): sites (-2, -1, -1),
    (-1, -1, -1) in unit (-1, -1, -1) and (gap - 1, 0, 0), (gap, 0, 0) in unit (0, 0, 0).  gap = 1: the only adjacent pair of the two
    blobs is (-1, -1, -1) - (0, 0, 0), a difference of (1, 1, 1) across the unit corner: one component of four sites.  gap = 2: the
    nearest pair differs by (2, 1, 1): two components."""
    return _voxels(_pair((-2, -1, -1), (-1, -1, -1)) + _pair((gap, 0, 0), (gap - 1, 0, 0)))


# ---- 3. serpentine -------------------------------------------------------------------------------------------------------------
TUBE_RADIUS = 2
SERPENTINE_ROWS, SERPENTINE_X = (8, 24, 40, 56), (8, 88)  # y of the four runs (one per unit row), the x range they span (six units)


def _serpentine_path():
    """Corner points of the tube's axis in the plane z = 8: runs along x at y = 8, 24, 40, 56, joined by U-turns at alternating ends."""
    pts, (x0, x1) = [], SERPENTINE_X
    for i, y in enumerate(SERPENTINE_ROWS):
        pts += [(x0, y, 8), (x1, y, 8)] if i % 2 == 0 else [(x1, y, 8), (x0, y, 8)]
    return np.array(pts, np.float64)


def _distance_to_path(p, path):
    best = np.full(p.shape[:-1], np.inf)
    for a, b in zip(path[:-1], path[1:]):
        ab = b - a
        s = np.clip(((p - a) @ ab) / (ab @ ab), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(p - (a + s[..., None] * ab), axis=-1))
    return best


@functools.lru_cache(maxsize=None)
def serpentine_states():
    """A tube of radius 2 voxels whose axis winds through the 6 x 4 units (0..5, 0..3, 0) with three U-turns: ONE component, 24 units.
    The runs are 16 voxels apart, their sites (radius about 2) at least 10: nothing but the tube itself joins them."""
    path = _serpentine_path() * VOX
    tube = lambda p: _distance_to_path(p, path) - TUBE_RADIUS * VOX
    states = _band(tube, list(itertools.product(range(6), range(4), (0,))))
    assert len(states[0]) == 24
    return states


# ---- 4. dust -------------------------------------------------------------------------------------------------------------------
DUST_UNITS, DUST_PITCH = 4, 4  # 4 x 4 x 4 units of FREE space, one INSIDE voxel at every (4 i, 4 j, 4 k)
DUST_COMPONENTS = (DUST_UNITS * R16 // DUST_PITCH) ** 3                                             # 16^3 = 4096
DUST_SITES = 7 * DUST_COMPONENTS - 3 * (DUST_UNITS * R16 // DUST_PITCH) ** 2                        # 27 904: see dust_states


@functools.lru_cache(maxsize=None)
def dust_states():
    """Isolated single INSIDE voxels in observed FREE space on a pitch of 4 voxels.  Each is a component of its own: the voxel and its
    six axis neighbours, 7 sites - one fewer for every coordinate that is 0, where the neighbour at -1 lies in a unit the map does not
    hold; the sites of two neighbouring specks (at 4 i + 1 and 4 i + 3) differ by 2 and are not adjacent.  A pitch of 4 leaves room
    for 64 specks per unit, so more than 4000 components need 64 units: 4 x 4 x 4, 4096 components.  A quarter of the specks per
    axis sit at local coordinate 0: on unit faces, edges and corners, their components cross into two, three and four units."""
    keys = np.array(list(itertools.product(range(DUST_UNITS), repeat=3)), np.int64)
    tsdf = np.full((len(keys), ps.NV), 0.5, np.float32)
    speck = ((ps._IDX % DUST_PITCH) == 0).all(axis=1)
    tsdf[:, speck] = -0.25
    return ps.finish(keys, tsdf, np.full(tsdf.shape, 2.0, np.float32), np.full(tsdf.shape + (3,), 128.0))


# name -> (states, the weight thresholds the tests run, hand-derived component counts per threshold or None)
STATES = {
    "two blobs": (two_blobs_states, (0.0,), (2,)),
    "corner touch": (corner_touch_states, (0.0,), (1,)),
    "corner apart": (functools.partial(corner_touch_states, 2), (0.0,), (2,)),
    "serpentine": (serpentine_states, (0.0,), (1,)),
    "dust": (dust_states, (0.0,), (DUST_COMPONENTS,)),
    "oblique": (dc.oblique_states, (0.0,), (1,)),
    "mixed weights": (dc.mixed_weight_states, (0.0, 2.0), None),
    "no site": (dc.no_site_states, (0.0,), (0,)),
    "lone inside": (dc.lone_inside_states, (0.0,), (1,)),
    "cluster": (sc.cluster_states, (0.0, 3.0), None),
}

MARGINS = (0, 1, 4, 16)


def min_sites_axis(largest):
    """The issue's axis: 1, 8, half the largest component, largest + 1 (distinct values, each >= 1)."""
    return tuple(sorted({1, 8, max(1, largest // 2), largest + 1}))
