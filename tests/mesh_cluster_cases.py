"""Planted voxel states (tests/planted_states.py: VOX 0.02, TRUNC 0.08) for the vertex-clustered mesh - test infrastructure, no GPU.

Every voxel of a case is observed with weight 1 unless said otherwise, and any |tsdf| < 0.02 is pushed to +-0.02: no vertex sits on a
voxel centre (the interpolation parameter stays in [0.0196, 0.9804]), so tests/mesh_cluster_reference.owners_from_positions reads
every vertex's owner voxel from its position without ambiguity."""
import functools
import itertools

import numpy as np

from tests import planted_states as ps

NORMAL = np.array([0.48, 0.6, 0.64])  # unit length
OFFSET = 0.013
PLANE_KEYS = np.array(list(itertools.product((-1, 0), repeat=3)), np.int64)
SPHERE_KEY = (5, -7, 3)
SPHERE_RADIUS = 0.09
CELLS = (2, 4, 8, 16)
CORNER = (2, -3, 1)  # case (d): the eight units around the corner (CORNER + 1) * 16 voxels


def _push(tsdf):
    t = np.asarray(tsdf, np.float32).copy()
    small = np.abs(t) < np.float32(0.02)
    t[small] = np.where(t[small] < 0, np.float32(-0.02), np.float32(0.02))
    return t


def _observed(keys, distance, seed):
    """All voxels of `keys` observed once, tsdf = clip(distance / TRUNC) pushed off zero, random colours."""
    rng = np.random.default_rng(1000 + seed)
    tsdf = _push(np.clip(distance / ps.TRUNC, -1.0, 1.0))
    return ps.finish(keys, tsdf, np.ones(tsdf.shape, np.float32), rng.integers(0, 256, tsdf.shape + (3,)).astype(np.float64))


def _plane_distance(keys):
    return ps.centres(keys) @ NORMAL - OFFSET


def _join(*states):
    return ps.finish(*(np.concatenate([s[k] for s in states]) for k in range(4)))


def _sphere():
    """A sphere inside the lone unit SPHERE_KEY, its centre a quarter voxel off the unit's centre."""
    centre = (np.array(SPHERE_KEY) + 0.5) * ps.UNIT + 0.25 * ps.VOX
    return _observed([SPHERE_KEY], np.linalg.norm(ps.centres([SPHERE_KEY]) - centre, axis=-1) - SPHERE_RADIUS, 1)


def smooth():
    """(a) the plane through the eight units {-1, 0}^3 (clusters in units with negative keys) and the sphere."""
    return _join(_observed(PLANE_KEYS, _plane_distance(PLANE_KEYS), 0), _sphere())


def rough():
    """(b) the same plane with N(0, 1.5 voxel) noise on the signed distance: clusters joined by several full triangles, and thin
    folds whose two sides land on the same three clusters."""
    d = _plane_distance(PLANE_KEYS)
    return _join(_observed(PLANE_KEYS, d + np.random.default_rng(2).normal(0.0, 1.5 * ps.VOX, d.shape), 2), _sphere())


def two_faced():
    """(c) a slab 1.6 voxels thick around the plane: two surfaces of opposite orientation inside one cell."""
    return _observed(PLANE_KEYS, np.abs(_plane_distance(PLANE_KEYS)) - 0.8 * ps.VOX, 3)


def no_triangles():
    """(d) one sign change at a unit corner.  Of the eight units around the corner only the eight voxels that meet there are
    observed, the one of the highest unit negative: ONE valid cube, owned by the lowest unit, whose three crossing edges belong to
    three other units.  Three units hold a vertex and no triangle, the lowest unit holds the triangle and no vertex (a map as a
    whole cannot have vertices without a triangle: a vertex needs a mixed cube with all eight corners observed)."""
    parts = []
    for d in itertools.product((0, 1), repeat=3):
        local = tuple(0 if s else ps.R - 1 for s in d)
        parts.append(ps.single_voxel(tuple(int(c + s) for c, s in zip(CORNER, d)), local, tsdf=-0.5 if d == (1, 1, 1) else 0.25, weight=1,
                                     colour=(40 * sum(d), 200 - 30 * d[0], 17 + 100 * d[2])))
    return _join(*parts)


def no_surface():
    """(e) a unit observed on one side of the surface only."""
    return _observed([(1, 2, -3)], np.full((1, ps.NV), 0.05), 4)


def lone_sphere():
    """The sphere alone: at cell 16 its 384 vertices are ONE cluster (six full waves of members) and every triangle is degenerate -
    a result with a vertex and no triangle."""
    return _sphere()


CASES = {"smooth": smooth, "rough": rough, "two-faced": two_faced, "no triangles": no_triangles, "no surface": no_surface,
         "lone sphere": lone_sphere}


@functools.lru_cache(maxsize=None)
def states(name):
    """Shared between the tests: nothing of it may be written to."""
    return CASES[name]()


def duplicates_and_reversed(vertex_cluster, triangles):
    """Of the full triangles mapped through vertex_cluster: (kept triples, distinct ones, the largest multiplicity, distinct triples
    whose reverse orientation is also present)."""
    t = np.asarray(vertex_cluster, np.int64)[np.asarray(triangles, np.int64).reshape(-1, 3)]
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    if len(t) == 0:
        return 0, 0, 0, 0
    shift = np.argmin(t, axis=1)
    t = np.stack([t[np.arange(len(t)), (shift + j) % 3] for j in range(3)], axis=1)
    distinct, counts = np.unique(t, axis=0, return_counts=True)
    have = {tuple(r) for r in distinct.tolist()}
    rev = sum((a, c, b) in have for a, b, c in have)
    return len(t), len(distinct), int(counts.max()), rev
