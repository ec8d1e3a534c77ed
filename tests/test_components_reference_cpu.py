"""CPU: the numpy restatement of the surface components (tests/components_reference.py) against an independent labelling
(scipy.ndimage.label with the full 3 x 3 x 3 structure), hand-derived component counts of the planted states
(tests/components_cases.py), and the two properties the contract claims for the removal: it is idempotent and creates no site.
"""
import functools

import numpy as np
import pytest

from tests import components_cases as cc
from tests import components_reference as cr
from tests import planted_states as ps

CASES = [(name, thr) for name, (_, thresholds, _) in cc.STATES.items() for thr in thresholds]


@functools.lru_cache(maxsize=None)
def dump_of(name):
    return ps.as_dump(cc.STATES[name][0]())


@functools.lru_cache(maxsize=None)
def reference(name, threshold):
    return cr.components(dump_of(name), threshold)


@pytest.mark.parametrize("name,threshold", CASES)
def test_partition_equals_scipy_label(name, threshold):
    """The same partition of the same sites, up to renumbering; and the table describes it."""
    from scipy import ndimage
    ref = reference(name, threshold)
    coords = ref["site_index"].astype(np.int64)
    units, n, C, largest = ref["stats"]
    assert n == len(coords) == len(ref["site_label"]) and units == len(dump_of(name)[0])
    if n == 0:
        assert C == 0 and largest == 0
        return
    grid, lo = cr.site_grid(coords)
    theirs, count = ndimage.label(grid, structure=np.ones((3, 3, 3)))
    assert count == C
    pairs = np.unique(np.stack([ref["site_label"].astype(np.int64), theirs[tuple((coords - lo).T)]], axis=1), axis=0)
    assert len(pairs) == C and len(np.unique(pairs[:, 0])) == C and len(np.unique(pairs[:, 1])) == C  # a bijection of the labels
    # the table: sizes, boxes, seeds in increasing (x, y, z) order, each the smallest site of its component
    assert np.array_equal(ref["sites"], np.bincount(ref["site_label"], minlength=C)) and int(ref["sites"].max()) == largest
    seeds = [tuple(s) for s in ref["seed"].tolist()]
    assert seeds == sorted(seeds) and len(set(seeds)) == C
    for c in (0, C // 2, C - 1):
        mine = coords[ref["site_label"] == c]
        assert tuple(ref["seed"][c]) == min(map(tuple, mine.tolist()))
        assert np.array_equal(ref["lo"][c], mine.min(axis=0)) and np.array_equal(ref["hi"][c], mine.max(axis=0))
    # the site list: by unit key, then dump order
    rows = [tuple(k) + tuple(l) for k, l in zip((coords >> 4).tolist(), (coords & 15).tolist())]
    assert rows == sorted(rows) and len(set(rows)) == n


def test_hand_derived_counts():
    for name, (_, thresholds, expected) in cc.STATES.items():
        if expected is None:
            continue
        for thr, count in zip(thresholds, expected):
            assert reference(name, thr)["stats"][2] == count, (name, thr)
    blobs = reference("two blobs", 0.0)
    assert blobs["sites"][0] > blobs["sites"][1] > 8  # the sphere on the corner comes first ((-x, ..) seed) and is the larger
    assert (blobs["lo"][0] < 0).all() and (blobs["hi"][0] >= 0).all() and (blobs["lo"][1] >> 4 == (2, 0, 0)).all() and (blobs["hi"][1] >> 4 == (2, 0, 0)).all()
    assert reference("corner touch", 0.0)["sites"].tolist() == [4] and reference("corner apart", 0.0)["sites"].tolist() == [2, 2]
    tube = reference("serpentine", 0.0)
    assert len(np.unique(tube["site_index"] >> 4, axis=0)) == 24  # the one component has sites in every unit
    dust = reference("dust", 0.0)
    assert dust["stats"][1] == cc.DUST_SITES and dust["stats"][3] == 7 and sorted(set(dust["sites"].tolist())) == [4, 5, 6, 7]
    assert int((dust["sites"] == 7).sum()) == 15 ** 3
    assert reference("mixed weights", 2.0)["stats"][2] > reference("mixed weights", 0.0)["stats"][2]  # half of the sheet gone: it falls apart


# state, threshold, the whole min_sites x margin grid?  (the two large states run min_sites 8 and half the largest at margins 1 and 16)
REMOVALS = [("two blobs", 0.0, True), ("corner apart", 0.0, True), ("lone inside", 0.0, True), ("mixed weights", 2.0, False), ("cluster", 0.0, False)]


@pytest.mark.parametrize("name,threshold,whole", REMOVALS)
def test_removal_is_idempotent_and_creates_no_site(name, threshold, whole):
    dump = dump_of(name)
    before = reference(name, threshold)
    sites_before = set(map(tuple, before["site_index"].tolist()))
    largest = before["stats"][3]
    for min_sites in cc.min_sites_axis(largest) if whole else (8, max(1, largest // 2)):
        small = set(np.flatnonzero(before["sites"] < min_sites).tolist())
        for margin in cc.MARGINS if whole else (1, 16):
            after, stats = cr.remove_components(dump, min_sites, margin, threshold, ref=before)
            assert stats[0] == before["stats"][2] and stats[1] == len(small) and stats[3] == int(before["sites"][sorted(small)].sum())
            again = cr.components(after, threshold)
            sites_after = set(map(tuple, again["site_index"].tolist()))
            # no new site; exactly the kept components' sites remain, in the same components
            kept = {tuple(s) for s, l in zip(before["site_index"].tolist(), before["site_label"].tolist()) if l not in small}
            assert sites_after <= sites_before and sites_after == kept, (name, min_sites, margin)
            assert again["stats"][2] == before["stats"][2] - len(small)
            assert np.array_equal(again["sites"], np.delete(before["sites"], sorted(small)))
            twice, stats2 = cr.remove_components(after, min_sites, margin, threshold)
            assert stats2[1] == stats2[3] == stats2[4] == stats2[5] == 0, (name, min_sites, margin, stats2)
            for a, b in zip(twice, after):
                assert np.array_equal(a, b)
            if not small:
                assert stats[4] == 0
            else:
                assert stats[4] >= stats[3] and stats[5] >= 1


def test_margin_takes_the_band_along_and_spares_the_kept_surface():
    """two blobs, min_sites between the two sizes: margin 0 resets the small sphere's sites only; margin 4 (the band) empties its
    unit; the big sphere's units are untouched at every margin."""
    dump = dump_of("two blobs")
    ref = reference("two blobs", 0.0)
    min_sites = int(ref["sites"][1]) + 1
    keys = dump[0]
    row = int(np.flatnonzero((keys == (2, 0, 0)).all(axis=1))[0])
    for margin in cc.MARGINS:
        after, stats = cr.remove_components(dump, min_sites, margin, ref=ref)
        for k in range(len(keys)):
            if k != row:
                assert all(np.array_equal(a[k], b[k]) for a, b in zip(after, dump))
        assert stats[1] == 1 and stats[3] == int(ref["sites"][1]) and stats[5] == 1
        if margin == 0:
            assert stats[4] == stats[3] and stats[6] == 0
        if margin >= 4:
            assert stats[6] == 1 and not (after[2][row] > 0).any() and len(cr.empty_units(after)) == 1
