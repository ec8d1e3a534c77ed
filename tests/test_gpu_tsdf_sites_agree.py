"""The two kernels that classify the map's surface sites (k_dist_classify, k_cc_sites) share one halo (hv_tsdf_sites.h): on the
smallest map at which that halo can go wrong they name the same sites, and both name the sites of tests/distance_reference.py.

Four planted units (tests/planted_states.py): three form an L - (0,0,0), (1,0,0), (0,1,0) - and one, (3,0,0), stands two units
away.  So some unit faces see a held neighbour, some an absent one, and one unit has no neighbour at all.  The sign of the tsdf
follows a smooth field of the GLOBAL voxel index, so FREE / INSIDE changes cross unit faces, run along unit edges and lie in the
interior; the weights are 0 .. 5, and the second threshold lies between two of them.  Integer sets, compared for equality.
"""
import functools

import numpy as np
import pytest

from tests import distance_reference as dr
from tests import planted_states as ps
from tests.test_gpu_tsdf_deintegrate import assert_bitwise
from tests.test_gpu_tsdf_edges import volume

pytestmark = pytest.mark.gpu

KEYS = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (3, 0, 0)], np.int64)
THRESHOLDS = (0.0, 2.5)  # 2.5: between the planted weights 2 and 3


def four_units():
    rng = np.random.default_rng(41)
    g = (KEYS.reshape(-1, 1, 3) * ps.R + ps._IDX[None]).astype(np.float64)  # global voxel index [U, 4096, 3]
    # zero sets at non-integer positions, through the faces x = 16 and y = 16, along the edge x = y = 16 and inside the units
    field = np.sin(g[..., 0] * 0.41 + 0.3) * np.cos(g[..., 1] * 0.37 - 0.2) + 0.6 * np.sin(g[..., 2] * 0.53 + g[..., 0] * 0.11 + 0.7)
    tsdf = np.clip(0.5 * field, -1.0, 1.0).astype(np.float32)
    weight = rng.integers(0, 6, tsdf.shape).astype(np.float32)
    colour = rng.integers(0, 256, tsdf.shape + (3,)).astype(np.float64)
    return ps.finish(KEYS, tsdf, weight, colour)


@functools.lru_cache(maxsize=None)
def planted():
    states = four_units()
    vol = ps.plant(volume(ps.VOX, ps.TRUNC), states)
    dump = vol.dump()
    assert_bitwise(dump, ps.as_dump(states))
    return vol, dump


def box():
    """Every voxel of the four units and one unit of margin around them: (origin, shape) in voxels."""
    lo = (KEYS.min(axis=0) - 1) * ps.R
    hi = (KEYS.max(axis=0) + 2) * ps.R - 1
    return lo, hi - lo + 1


def rows(a):
    a = np.asarray(a, np.int64).reshape(-1, 3)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_distance_field_and_surface_components_name_the_sites_of_the_restatement(threshold):
    vol, dump = planted()
    origin, shape = box()
    centre = lambda idx: (np.asarray(idx, np.float64) + 0.5) * ps.VOX
    field = vol.distance_field((centre(origin), centre(origin + shape - 1)), ps.VOX, weight_threshold=threshold, pad=False, outputs=("cls",))
    assert np.array_equal(field.origin, origin) and field.shape == tuple(shape) and field.distance is None
    from_distance = rows(np.argwhere(field.cls & dr.SITE) + origin)
    from_components = rows(vol.surface_components(weight_threshold=threshold, sites=True).site_index)
    ref_cls = dr.classify(dump, origin, shape, threshold)
    expected = rows(np.argwhere(ref_cls & dr.SITE) + origin)
    print(f"threshold {threshold}: {len(expected)} sites")
    assert np.array_equal(from_distance, from_components)
    assert np.array_equal(from_distance, expected) and np.array_equal(from_components, expected)
    assert np.array_equal(field.cls, ref_cls)
    # the case holds what it is there for: sites on unit faces, on unit edges and inside, in every unit, beside held and absent units
    local = expected & 15
    border = ((local == 0) | (local == 15)).sum(axis=1)
    assert (border == 0).any() and (border == 1).any() and (border >= 2).any()
    assert len(np.unique(expected >> 4, axis=0)) == len(KEYS)
    at = lambda x, y: (expected[:, 0] == x) & (expected[:, 1] == y)
    assert (expected[:, 0] == 15).any() and (expected[:, 0] == 16).any()  # the face between (0,0,0) and (1,0,0), from both sides
    assert (expected[:, 0] == 31).any() and (expected[:, 0] == 48).any()  # faces towards the absent unit (2,0,0)
    assert at(15, 15).any() and at(15, 16).any() and at(16, 15).any()    # around the edge x = y = 16, whose fourth unit is absent


def test_the_threshold_between_two_weights_changes_the_sites():
    _, dump = planted()
    origin, shape = box()
    a, b = (dr.classify(dump, origin, shape, t) & dr.SITE for t in THRESHOLDS)
    assert a.any() and b.any() and not np.array_equal(a, b)
