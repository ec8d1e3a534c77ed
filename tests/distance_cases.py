"""The planted maps, boxes and radii the distance-field tests share (tests/test_distance_reference_cpu.py on the CPU,
tests/test_gpu_tsdf_distance.py on the GPU) - test infrastructure, no GPU.  Everything is built from fixed seeds with
tests/planted_states.py: voxel 0.02, sdf_trunc 0.08, a few dozen units per state.
"""
import functools
import itertools

import numpy as np

from tests import planted_states as ps
from tests import sample_cases as sc

VOX, TRUNC, R16 = ps.VOX, ps.TRUNC, ps.R

# (origin, shape) in voxels: unit borders at -16 / 0 / 16, lines shorter and longer than a wave and no multiple of 64, a dimension of
# 1, a box equal to one unit, and (with the radii below) a radius above every dimension
BOXES = (((0, 0, 0), (1, 1, 1)), ((-21, -5, 11), (37, 40, 43)), ((-16, 0, 16), (16, 16, 16)), ((3, -40, -1), (1, 70, 3)),
         ((-33, -33, -33), (65, 17, 33)))
RADII = (1, 3, 16, 64)

PLANE_UNITS = tuple(itertools.product(range(-2, 2), repeat=3))  # voxels -32 .. 31 per axis
OBLIQUE_NORMAL = np.array([0.36, 0.48, 0.8])                     # unit length
OBLIQUE_POINT = np.array([0.013, -0.007, 0.021])


def slab_distance(p):
    """Signed distance to the plane x = 0: the zero crossing lies on the border of units -1 and 0."""
    return np.asarray(p)[..., 0]


def oblique_distance(p):
    return (np.asarray(p) - OBLIQUE_POINT) @ OBLIQUE_NORMAL


def _plane(distance, keys, weights):
    """tsdf = distance / TRUNC where |distance| <= TRUNC (the truncation band), nothing observed elsewhere; only units that hold an
    observed voxel are kept.  weights: seed -> integer weights per voxel."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    d = distance(ps.centres(keys))
    band = np.abs(d) <= TRUNC
    keep = band.any(axis=1)
    keys, d, band = keys[keep], d[keep], band[keep]
    weight = np.where(band, weights(d.shape), 0).astype(np.float32)
    colour = np.random.default_rng(5).integers(0, 256, d.shape + (3,)).astype(np.float64)
    return ps.finish(keys, (d / TRUNC).astype(np.float32), weight, colour)


@functools.lru_cache(maxsize=None)
def slab_states():
    """An axis-aligned plane, x = 0, over 2 x 4 x 4 units."""
    return _plane(slab_distance, [k for k in PLANE_UNITS if k[0] in (-1, 0)], lambda shape: np.full(shape, 4))


@functools.lru_cache(maxsize=None)
def oblique_states():
    """A plane with normal (0.36, 0.48, 0.8) through OBLIQUE_POINT, in the units of PLANE_UNITS its band meets."""
    return _plane(oblique_distance, PLANE_UNITS, lambda shape: np.full(shape, 4))


@functools.lru_cache(maxsize=None)
def mixed_weight_states():
    """The oblique plane with weights 1 and 3 mixed: weight_threshold = 2 takes half of the voxels, and with them sites, away."""
    return _plane(oblique_distance, PLANE_UNITS, lambda shape: np.random.default_rng(9).choice([1, 3], shape))


@functools.lru_cache(maxsize=None)
def no_site_states():
    """Observed voxels (a share unobserved) that are all FREE: no sign change, no site at all."""
    keys, tsdf, weight, colour = ps.random_units(np.array([(-1, -1, 0), (0, -1, 0), (0, 0, 1), (-2, 0, -1)], np.int64), 31)
    return ps.finish(keys, np.abs(tsdf) + np.float32(0.01), weight, colour)


LONE_VOXEL = (-32, -32, -32)  # voxel (0, 0, 0) of unit (-2, -2, -2): three of its six neighbours lie in other units


@functools.lru_cache(maxsize=None)
def lone_inside_states():
    """The eight units around the unit corner at voxel (-32, -32, -32), every voxel FREE (tsdf 0.5, weight 2) except the one INSIDE
    voxel at the corner: seven sites in four units."""
    keys = np.array(list(itertools.product((-3, -2), repeat=3)), np.int64)
    tsdf = np.full((len(keys), ps.NV), 0.5, np.float32)
    row = int(np.flatnonzero((keys == -2).all(axis=1))[0])
    tsdf[row, 0] = -0.25
    return ps.finish(keys, tsdf, np.full(tsdf.shape, 2.0, np.float32), np.full(tsdf.shape + (3,), 128.0))


# name -> (states, the weight thresholds the GPU equality test runs)
STATES = {
    "slab": (slab_states, (0.0,)),
    "oblique": (oblique_states, (0.0,)),
    "cluster": (sc.cluster_states, (0.0, 3.0)),
    "no site": (no_site_states, (0.0,)),
    "lone inside": (lone_inside_states, (0.0,)),
    "mixed weights": (mixed_weight_states, (0.0, 2.0)),
}

# the accuracy test's box: inside the voxels -32 .. 31 the planes are planted over
ACCURACY_BOX = ((-20, -18, -21), (40, 37, 43))
ACCURACY_RADIUS = 64  # above every dimension of the box: nothing is capped


def cell_centres(origin, shape):
    """World positions [shape, 3] of the cells' voxel centres."""
    idx = np.stack(np.meshgrid(*(np.arange(n, dtype=np.int64) for n in shape), indexing="ij"), -1) + np.asarray(origin, np.int64)
    return (idx + 0.5) * VOX


def to_nearest_face(shape):
    """Per cell: the distance in voxels from its centre to the nearest face of the box."""
    axes = [np.minimum(np.arange(n) + 0.5, n - 0.5 - np.arange(n)) for n in shape]
    gx, gy, gz = np.meshgrid(*axes, indexing="ij")
    return np.minimum(np.minimum(gx, gy), gz)
