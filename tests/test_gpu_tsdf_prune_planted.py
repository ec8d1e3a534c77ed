"""GPU: ScalableTSDFVolume.prune (hv_prune.hip) on planted units (tests/planted_states.py) - what a fused map never shows it:
units whose only observed voxel sits in one chosen word of the weight plane (every lane, component and iteration group of
hv_tsdf_unit_has_weight), more units in use than k_prune_plan has threads (several flags per thread, prefix[] read across threads),
and a pool order set by the order of the planting calls, so that which survivors move is known.

Every case is held bit for bit to tests/prune_reference.py on the volume's own dump, stats included, runs
tests/test_gpu_tsdf_prune.py::assert_consistent, and prunes a second time, which must release nothing.  The pool order after a prune
is held to the plan the contract describes (expected_pool_order).  hv_tsdf_import_numerators claims a unit whose payload is all
zero, so empty units are planted as they are.

Measured on the MI355X when the file was written: every case equal to the restatement and to the restated plan; with
hv_tsdf_unit_has_weight stopping one iteration group early (scratch copy) the three one-voxel cases fail and nothing else does.
Nothing here takes longer than 1 s.
"""
import numpy as np
import pytest

from tests import planted_states as ps
from tests.prune_reference import prune_reference
from tests.test_gpu_tsdf_deintegrate import assert_bitwise
from tests.test_gpu_tsdf_edges import cuda, intrinsic, stack, tiny_frames
from tests.test_gpu_tsdf_prune import assert_consistent

pytestmark = pytest.mark.gpu

VOX, TRUNC = ps.VOX, ps.TRUNC
UNIT = VOX * ps.R


def volume(max_blocks=1 << 12):
    from pyslam_amd.volumetric import ScalableTSDFVolume

    return ScalableTSDFVolume(VOX, TRUNC, max_blocks=max_blocks)


def plant_empty(vol, keys, chunk=256):
    """All-zero units through import_numerators, `chunk` at a time from one zero payload (tens of MB however many there are)."""
    keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 3)
    zeros = np.zeros((min(chunk, len(keys)), ps.NV, 5), np.float32)
    for lo in range(0, len(keys), chunk):
        part = np.ascontiguousarray(keys[lo:lo + chunk])
        vol.import_numerators(part, zeros[:len(part)])


def key_set(keys):
    return {tuple(int(x) for x in k) for k in np.asarray(keys).reshape(-1, 3)}


def expected_pool_order(pool_keys, keep):
    """The plan of hv_tsdf_prune restated: with `kept` survivors, those at a pool index below kept stay where they are and the j-th
    survivor at or above kept goes into the j-th hole below it.  -> (pool keys after, number of moves)"""
    keep = np.asarray(keep, bool)
    kept = int(keep.sum())
    out = np.array(pool_keys[:kept], copy=True)
    holes = np.flatnonzero(~keep[:kept])
    movers = np.flatnonzero(keep[kept:]) + kept
    assert len(holes) == len(movers)
    out[holes] = pool_keys[movers]
    return out, len(movers)


def prune_and_check(vol, empty=True, lo=None, hi=None):
    """One prune held to the restatement on the volume's own dump, to the restated plan on its own pool order, and repeated.
    -> (dump before, dump after, stats, moves)"""
    from pyslam_amd.volumetric import unit_range_of_bounds

    bounds = None
    if lo is not None:
        bounds = ((np.asarray(lo, np.float64) + 0.5) * UNIT, (np.asarray(hi, np.float64) + 0.5) * UNIT)
        ulo, uhi = unit_range_of_bounds(bounds, VOX, ps.R)
        assert ulo.tolist() == list(lo) and uhi.tolist() == list(hi)
    before, pool = vol.dump(), vol.unit_keys()
    cap = vol.max_blocks()
    ref, stats = prune_reference(before, empty, lo, hi)
    survivors = key_set(ref[0])
    order, moves = expected_pool_order(pool, [tuple(int(x) for x in k) in survivors for k in pool])
    st = vol.prune(empty=empty, bounds=bounds)
    assert st.as_tuple() == stats, (st.as_tuple(), stats)
    after = vol.dump()
    assert_bitwise(after, ref)
    assert_consistent(vol, stats[3])
    np.testing.assert_array_equal(vol.unit_keys(), order)
    assert vol.max_blocks() == cap
    again = vol.prune(empty=empty, bounds=bounds)
    assert again.as_tuple() == (stats[3], 0, 0, stats[3])
    assert_bitwise(vol.dump(), ref)
    np.testing.assert_array_equal(vol.unit_keys(), order)
    return before, after, stats, moves


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["survivors", "empties", "together"])
def test_one_observed_voxel_keeps_its_unit(first):
    """~330 units whose only observed voxel visits every lane, component and iteration group of the emptiness test, interleaved in
    key order with as many all-zero units.  Planted survivors first nothing moves; empties first every survivor sits above `kept`
    and moves; in one call the claim pass decides."""
    states, words = ps.one_voxel_units()
    n = len(states[0])
    hollow = ps.empty_units(states[0].astype(np.int64) + [0, 10, 0])  # the same x, a larger y: alternating in (x, y, z) order
    vol = volume()
    if first == "together":
        both = tuple(np.concatenate([a, b]) for a, b in zip(states, hollow))
        ps.plant(vol, both)
    else:
        for part in ((states, hollow) if first == "survivors" else (hollow, states)):
            ps.plant(vol, part)
    pool = vol.unit_keys()
    assert len(pool) == 2 * n  # an all-zero payload claims its unit
    if first != "together":
        mine, theirs = (states, hollow) if first == "survivors" else (hollow, states)
        assert key_set(pool[:n]) == key_set(mine[0]) and key_set(pool[n:]) == key_set(theirs[0])
    ones = key_set(states[0])
    is_one = np.array([tuple(int(x) for x in k) in ones for k in vol.dump()[0]])
    assert is_one[::2].all() and not is_one[1::2].any()  # interleaved in key order
    before, after, stats, moves = prune_and_check(vol)
    assert stats == (2 * n, 0, n, n)
    assert moves == {"survivors": 0, "empties": n}.get(first, moves)
    assert_bitwise(after, ps.as_dump(states))  # every unit comes back with its voxel, at its key
    np.testing.assert_array_equal(np.argmax(after[2], axis=1), words)
    assert ((after[2] > 0).sum(axis=1) == 1).all()


# 2 ---------------------------------------------------------------------------------------------------------------------------
KEPT = 40


def kept_keys(count=KEPT):
    j = np.arange(count, dtype=np.int64)
    return np.stack([3 * j - 20, j % 4 + 1, j % 3], axis=1)  # some of them where the tiny camera looks


def empty_keys(count):
    j = np.arange(count, dtype=np.int64)
    return np.stack([j % 97 - 48, -3 - j // 97, j % 5 - 2], axis=1)


PATTERNS = {
    "kept last": lambda e: (("E", e), ("K", KEPT)),
    "kept first": lambda e: (("K", KEPT), ("E", e)),
    "alternating": lambda e: (("K", 10), ("E", e // 2), ("K", KEPT - 10), ("E", e - e // 2)),
    "kept after a few": lambda e: (("E", KEPT), ("K", KEPT), ("E", e - KEPT)),
}


def planted_pattern(used, pattern, seed=21):
    """`used` units, KEPT of them with arbitrary contents, planted call by call as PATTERNS[pattern] says.  -> (volume, kept states)"""
    kept = ps.random_units(kept_keys(), seed)
    hollow = empty_keys(used - KEPT)
    assert not key_set(kept[0]) & key_set(hollow)
    # the kept units in the order the calls plant them (kept[0] is key-sorted: any split of it will do)
    vol = volume(1 << 12)
    k0 = e0 = 0
    expect = []
    for what, count in PATTERNS[pattern](used - KEPT):
        if what == "K":
            part = tuple(x[k0:k0 + count] for x in kept)
            ps.plant(vol, part)
            expect.append(key_set(part[0]))
            k0 += count
        else:
            plant_empty(vol, hollow[e0:e0 + count])
            expect.append(key_set(hollow[e0:e0 + count]))
            e0 += count
    assert k0 == KEPT and e0 == used - KEPT
    pool = vol.unit_keys()
    assert len(pool) == used == vol.num_blocks()
    at = 0
    for group in expect:  # pool order at call granularity
        assert key_set(pool[at:at + len(group)]) == group
        at += len(group)
    return vol, kept


@pytest.mark.parametrize("used,pattern", [(1025, "kept last"), (1025, "kept first"), (1025, "alternating"), (2049, "kept last"),
                                          (2049, "kept first"), (2049, "alternating"), (1023, "kept last"), (1024, "kept last")])
def test_plan_with_more_units_than_threads(used, pattern):
    """used = 1025 and 2049: ceil(used / 1024) = 2 and 3 flags per thread of k_prune_plan, the last threads' ranges empty or cut
    short, `kept` in another thread's range; 1023 and 1024: one flag per thread, on both sides of the step."""
    vol, kept = planted_pattern(used, pattern)
    before, after, stats, moves = prune_and_check(vol)
    assert stats == (used, 0, used - KEPT, KEPT)
    assert moves == {"kept last": min(KEPT, used - KEPT), "kept first": 0, "alternating": KEPT - 10}[pattern]
    assert_bitwise(after, ps.as_dump(kept))


# 3 ---------------------------------------------------------------------------------------------------------------------------
BOX_LO, BOX_HI = (-3, -2, -1), (2, 1, 4)
BOX_OBSERVED = ((-3, -2, -1), (2, 1, 4), (0, 0, 0), (-3, 1, 4), (2, -2, -1),    # inside: both corners of the box among them
                (3, 1, 4), (-3, -2, -2), (-4, 0, 0), (0, 2, 0), (5, 5, 5)) + ps.RIM_UNITS  # outside: one step past a face, and the rim
BOX_EMPTY = ((-3, -2, 4), (2, 1, -1), (1, 0, 1),  # inside and empty
             (3, -2, -1), (0, 0, 5), (ps.B - 1, 1, -ps.B), (-ps.B, -ps.B, -ps.B))  # outside and empty: counted as outside


@pytest.mark.parametrize("empty", [True, False])
@pytest.mark.parametrize("box", ["planted keys", "rim"])
def test_box_and_emptiness_on_planted_keys(box, empty):
    """unit_lo / unit_hi equal to planted keys (the edges are inclusive), negative indices, the rim of the key range."""
    vol = volume()
    ps.plant(vol, ps.random_units(np.array(BOX_OBSERVED, np.int64), 31))
    ps.plant(vol, ps.empty_units(BOX_EMPTY))
    lo, hi = (BOX_LO, BOX_HI) if box == "planted keys" else ((-ps.B, -1, -ps.B), (ps.B - 1, ps.B - 1, 5))
    before, after, stats, moves = prune_and_check(vol, empty=empty, lo=lo, hi=hi)
    keys = np.array(BOX_OBSERVED + BOX_EMPTY, np.int64)
    outside = np.any((keys < lo) | (keys > hi), axis=1)
    inside_empty = int((~outside[len(BOX_OBSERVED):]).sum())
    assert stats == (len(keys), int(outside.sum()), inside_empty if empty else 0, len(keys) - int(outside.sum()) - (inside_empty if empty else 0))
    assert stats[1] > 0 and stats[3] > 0 and inside_empty > 0 and outside[len(BOX_OBSERVED):].any()
    held = key_set(after[0])
    if box == "planted keys":
        assert {BOX_LO, BOX_HI} <= held and not {(3, 1, 4), (-3, -2, -2)} & held
    else:
        assert set(ps.RIM_UNITS) <= held and (-ps.B, -ps.B, -ps.B) not in held


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_the_pruned_map_still_works(monkeypatch):
    """2049 units, the survivors right above `kept`: they move down and the slots they leave are the first a later claim pass hands
    out.  Four frames fused into the pruned volume give, bit for bit, what they give in a fresh volume planted with the survivors."""
    monkeypatch.setenv("HV_TSDF_SWEEP", "2")
    vol, kept = planted_pattern(2049, "kept after a few")
    before, after, stats, moves = prune_and_check(vol)
    assert stats == (2049, 0, 2049 - KEPT, KEPT) and moves == KEPT
    fresh = volume()
    ps.plant(fresh, kept)
    s, frames = tiny_frames(0, 4)
    d, c, T = stack(frames)
    for v in (vol, fresh):
        v.integrate_batch(*cuda(d, c), intrinsic(s), T)
    out = vol.dump()
    assert len(out[0]) > KEPT + 100 and key_set(kept[0]) & (key_set(out[0]) - key_set(kept[0])) == set()
    touched = ~np.all(out[2][np.array([tuple(k) in key_set(kept[0]) for k in out[0]])] == after[2], axis=1)
    assert touched.any()  # some survivors were fused on top of
    assert_bitwise(out, fresh.dump())
    assert_consistent(vol, len(out[0]))
