"""CPU: the numpy restatement of the distance field (tests/distance_reference.py) against a structurally independent brute-force
evaluator, and what its number means on two planted planes (tests/distance_cases.py).  No GPU, no library call.
"""
import numpy as np
import pytest

from tests import distance_cases as dc
from tests import distance_reference as dr
from tests import planted_states as ps


@pytest.mark.parametrize("shape, density", [((20, 18, 22), 0.0), ((20, 18, 22), 0.002), ((20, 18, 22), 0.05), ((1, 1, 1), 1.0),
                                            ((1, 19, 2), 0.1), ((7, 1, 22), 0.3), ((5, 6, 7), 1.0)])
def test_separable_passes_equal_brute_force(shape, density):
    """Random site sets (the empty one and the full one included), radii below and above the box size.  Integer lattices are full of
    ties (several sites at one squared distance); both evaluators must give the one minimum."""
    rng = np.random.default_rng([int(density * 1000)] + list(shape))
    site = rng.random(shape) < density
    for radius in (1, 2, 3, 5, 16, 40):
        got, want = dr.transform(site, radius), dr.brute_force(site, radius)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (shape, density, radius, int((got != want).sum()))
        assert got.max() <= radius * radius and (got[site] == 0).all()
        if not site.any():
            assert (got == radius * radius).all()


def test_ties_and_the_cap():
    """Two sites at equal distance from the cells between them; a site at exactly the radius is capped to the same value as none."""
    site = np.zeros((9, 1, 1), bool)
    site[0], site[8] = True, True
    assert dr.transform(site, 10)[:, 0, 0].tolist() == [0, 1, 4, 9, 16, 9, 4, 1, 0]
    assert dr.transform(site, 3)[:, 0, 0].tolist() == [0, 1, 4, 9, 9, 9, 4, 1, 0]
    site = np.zeros((4, 5, 1), bool)
    site[0, 0] = True
    got = dr.transform(site, 5)
    assert got[3, 4, 0] == 25 and got[3, 3, 0] == 18 and np.array_equal(got, dr.brute_force(site, 5))
    _, stats = dr.finish(np.where(site, dr.FREE | dr.SITE, dr.FREE).astype(np.uint8), got, 0.02, 5)
    assert stats == (0, 20, 0, 1, 1)


def test_classification_rules():
    """Sites across a unit corner at negative indices; an UNKNOWN neighbour makes no site; a neighbour outside the box does."""
    dump = ps.as_dump(dc.lone_inside_states())
    lone = np.array(dc.LONE_VOXEL)
    cls = dr.classify(dump, lone - 2, (5, 5, 5))
    want = np.full((5, 5, 5), dr.FREE, np.uint8)
    want[2, 2, 2] = dr.INSIDE | dr.SITE
    for axis in range(3):
        for step in (-1, 1):
            at = [2, 2, 2]
            at[axis] += step
            want[tuple(at)] = dr.FREE | dr.SITE
    assert np.array_equal(cls, want)
    # a box of one cell beside the lone voxel: the neighbour that makes it a site is outside the box
    assert dr.classify(dump, lone + (1, 0, 0), (1, 1, 1)).item() == dr.FREE | dr.SITE
    # beyond the planted units everything is UNKNOWN, and the FREE voxels on the rim are no sites
    rim = dr.classify(dump, (-50, -40, -40), (4, 3, 3))
    assert (rim[:2] == dr.UNKNOWN).all() and (rim[2:] == dr.FREE).all()
    # weight thresholds: the lone voxel (weight 2) is unobserved at threshold 2, and with it every site goes
    assert not (dr.classify(dump, lone - 2, (5, 5, 5), 2.0) != dr.UNKNOWN).any()
    # no sign change, no site
    none = dr.classify(ps.as_dump(dc.no_site_states()), (-33, -17, -17), (50, 34, 50))
    assert ((none & 3) == dr.FREE).sum() > 1000 and not (none & dr.SITE).any() and not ((none & 3) == dr.INSIDE).any()
    # mixed weights: threshold 2 removes sites
    mixed = ps.as_dump(dc.mixed_weight_states())
    lo, hi = (dr.classify(mixed, *dc.ACCURACY_BOX, thr) for thr in (0.0, 2.0))
    assert 0 < ((hi & dr.SITE) != 0).sum() < 0.7 * ((lo & dr.SITE) != 0).sum()


@pytest.mark.parametrize("name", ["slab", "oblique"])
def test_distance_against_the_analytic_plane(name):
    """What the number means.  The field is the distance to the nearest site CENTRE.  Both voxels of a sign-changing lattice edge are
    sites and the zero crossing lies on that edge between their centres, so every site centre lies within one voxel length of the
    surface: the field under-reports the true distance by at most one voxel length.  The foot point of a cell on a plane lies in a
    lattice cube that the plane cuts, and a cut cube has a sign-changing edge, hence a site centre within the cube's diagonal,
    sqrt(3) voxel lengths, of the foot point: the field over-reports by at most sqrt(3) voxel lengths.  Cells whose analytic
    distance plus two voxels is less than their distance to the nearest box face have all of that neighbourhood inside the box;
    the radius is above every dimension, so nothing is capped.  1e-3 voxel covers the float32 roundings of the square root and
    the product.  Measured here, in voxel lengths: slab -0.5000003 .. -0.5 (its sites lie half a voxel on either side of the
    plane), oblique -0.794 .. +0.194."""
    states, analytic = {"slab": (dc.slab_states, dc.slab_distance), "oblique": (dc.oblique_states, dc.oblique_distance)}[name]
    origin, shape = dc.ACCURACY_BOX
    res = dr.distance_field(ps.as_dump(states()), dc.VOX, origin, shape, dc.ACCURACY_RADIUS)
    truth = analytic(dc.cell_centres(origin, shape)) / dc.VOX  # voxels, signed
    interior = np.abs(truth) + 2.0 < dc.to_nearest_face(shape)
    assert interior.sum() > 5000
    err = np.abs(res["distance"].astype(np.float64)) / dc.VOX - np.abs(truth)
    print(f"{name}: {int(interior.sum())} interior cells, |distance| - |analytic| in [{err[interior].min():.7f}, {err[interior].max():.7f}] voxel lengths")
    assert err[interior].min() >= -(1.0 + 1e-3) and err[interior].max() <= np.sqrt(3.0) + 1e-3
    # the sign is the map's: observed cells carry the sign of their tsdf, unobserved ones are positive
    observed = (res["cls"] & 3) != dr.UNKNOWN
    assert observed.sum() > 1000
    assert np.array_equal(np.signbit(res["distance"][observed]), truth[observed] <= 0.0)
    assert not np.signbit(res["distance"][~observed]).any()
    assert res["stats"][4] == 0  # nothing is far
