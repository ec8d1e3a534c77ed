"""GPU: ScalableTSDFVolume.integrate_volume (hv_merge.hip) on planted voxel states (tests/planted_states.py) - the branches a
map fused from depth images never reaches.  Everything is held to the numpy restatement (tests/merge_reference.py) run on the
planted volumes' OWN dumps, by the rules of tests/test_gpu_tsdf_merge.py::assert_matches_restatement: dumps equal off the fragile
voxels, whose share is capped at 1e-4 (tests/test_planted_states_cpu.py shows it is 0.0 for every transform used here), stats
equal to the restatement's.  Exact rotations with a whole-voxel translation put every voxel on a boundary of the rules and are held
to the permuted source instead (weights and colour sums exact, tsdf within 2^-23).

Voxel 0.02, sdf_trunc 0.08; at most ~100 destination units per case.

Measured on the MI355X when the file was written: every case held to the restatement is equal to it bit for bit (fragile share 0 for
the generic transforms; max colour-sum and tsdf difference 0 on the cases where every voxel is on a boundary); the exact rotations
reproduce the permuted source with a tsdf error <= 2.9e-14.  With the range guard of hv_tsdf_unit taken out, test_rim_of_the_key_range
[identity] and [z-3] fail and nothing else in the merge and ray-cast suites does; with R and R^T swapped in the host code 21 of the
tests here fail.
"""
import numpy as np
import pytest

from tests import merge_reference as mr
from tests import planted_states as ps
from tests.test_gpu_tsdf_deintegrate import assert_bitwise
from tests.test_gpu_tsdf_edges import cuda, intrinsic, stack, tiny_frames, volume
from tests.test_gpu_tsdf_merge import assert_consistent, assert_matches_restatement, fuse, merges_that_leave_untouched
from tests.test_merge_reference_cpu import GENERIC, assert_is_permuted_source
from tests.test_planted_states_cpu import (RIM_EXPECTED, SINGLE_EXPECTED, SINGLE_TRANSFORMS, SPARSE_STATS, SPARSE_TRANSFORMS, assert_doubled,
                                           overlapping_destination)

pytestmark = pytest.mark.gpu

VOX, TRUNC = ps.VOX, ps.TRUNC


def planted(states):
    """A volume holding the states; its dump is what tests/planted_states.as_dump says, bit for bit."""
    vol = volume(VOX, TRUNC)
    if len(states[0]):
        ps.plant(vol, states)
    assert_bitwise(vol.dump(), ps.as_dump(states))
    return vol


def merge_and_check(dst, src, T, name, on_a_boundary=None, bitwise=True):
    """One merge held to the restatement on the volumes' own dumps.  -> (dump after, MergeStats)"""
    before, src_dump = dst.dump(), src.dump()
    st = dst.integrate_volume(src, T)
    after = dst.dump()
    assert_bitwise(src.dump(), src_dump)
    equal, stats = assert_matches_restatement(after, before, src_dump, T, name, on_a_boundary=on_a_boundary)
    assert st.as_tuple() == stats, (name, st.as_tuple(), stats)
    assert st.units_claimed == len(after[0]) - len(before[0])
    claimed = ~np.isin(after[0].astype(np.int64) @ [1 << 44, 1 << 22, 1], before[0].astype(np.int64).reshape(-1, 3) @ [1 << 44, 1 << 22, 1])
    assert (after[2][claimed].max(axis=1) > 0).all() if claimed.any() else True, (name, "an all-zero unit was left behind")
    if bitwise:
        assert equal, (name, "the dumps differ off the restatement in some bit")
    assert_consistent(dst)
    return after, st


@pytest.fixture(scope="module")
def sparse_states():
    return ps.sparse_source()


# a ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filled", [False, True], ids=["empty", "overlapping"])
@pytest.mark.parametrize("name", [n for n in SPARSE_TRANSFORMS if n != "far"])
def test_sparse_source_under_worst_case_rotations(sparse_states, name, filled):
    """k_merge_candidates with n[a] == 3 and hv_merge_resolve's full 3 x 3 x 3 LDS table (rotations near the cube diagonal);
    candidates probed and not kept, units kept for a handful of voxels (a sparse source with an isolated unit); the nearest /
    trilinear decision with unobserved corners and absent units on every side (10 % unobserved voxels, 20 % missing units);
    g0 >> 4 on negative indices; and, into the overlapping destination, the w0 > 0 update on arbitrary tsdf0 / w0 / sums."""
    T = SPARSE_TRANSFORMS[name]
    src = planted(sparse_states)
    dst = volume(VOX, TRUNC)
    if filled:
        result_keys = mr.merge_reference(mr.empty_dump(), src.dump(), T, VOX)[0][0]
        dst = planted(overlapping_destination(result_keys))
    after, st = merge_and_check(dst, src, T, name)
    assert st.as_tuple()[2:] == SPARSE_STATS[name][2:] and st.voxels_trilinear > 40000 and st.voxels_nearest > 50000
    assert st.units_claimed == (SPARSE_STATS[name][1] // 2 if filled else SPARSE_STATS[name][1])  # (the destination held every second unit)


# b ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.EXACT_ROTATIONS))
def test_exact_rotations(sparse_states, name):
    """Rotations by 90 / 120 / 180 degrees with literal 0 / +-1 entries: every voxel sits on r = 0 / 1 (whole-voxel translation:
    the result is the permuted source) or on r = 0.5 (half-voxel translation: the restatement on EVERY voxel) - the r >= 0.5 tie
    of hv_merge_nearest and the rt (R^T) indexing of hv_merge_locate under axis permutations."""
    T = ps.EXACT_ROTATIONS[name]
    src = planted(sparse_states)
    dst = volume(VOX, TRUNC)
    if name.endswith("half"):
        merge_and_check(dst, src, T, name, on_a_boundary=True)
        return
    src_dump = src.dump()
    st = dst.integrate_volume(src, T)
    after = dst.dump()
    err = assert_is_permuted_source(after, src_dump, T, VOX, name)
    print(f"{name}: stats {st.as_tuple()}, tsdf err {err:.3g}")
    assert st.voxels_updated == int((src_dump[2] > 0).sum()) == st.voxels_trilinear + st.voxels_nearest
    assert st.units_claimed == len(after[0]) and st.units_source == 26
    assert_consistent(dst)


# c ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", list(SINGLE_TRANSFORMS))
@pytest.mark.parametrize("source", list(ps.SINGLE_VOXELS))
def test_single_voxel_sources(source, transform):
    """k_merge_probe's early exit and keep list when ONE voxel decides (units kept for a single voxel, candidates all but one of
    which are dropped), at the low corner, the high corner and a face of a unit; and the no-voxel case (the half-voxel shift puts
    the face voxel's image at r = 0.5 ties that no destination voxel wins): a filled destination stays bitwise, caches included."""
    T = SINGLE_TRANSFORMS[transform]
    src = planted(ps.single_voxel(*ps.SINGLE_VOXELS[source]))
    voxels, units = SINGLE_EXPECTED.get((source, transform), (1, 1))
    if voxels:
        after, st = merge_and_check(volume(VOX, TRUNC), src, T, f"{source} / {transform}", on_a_boundary=transform != "diagonal")
        assert st.as_tuple() == (1, units, voxels, 0, voxels) and len(after[0]) == units
    else:
        src_dump = src.dump()
        assert mr.merge_reference(mr.empty_dump(), src_dump, T, VOX)[1] == (1, 0, 0, 0, 0)
        dst = volume(VOX, TRUNC)
        assert dst.integrate_volume(src, T).as_tuple() == (1, 0, 0, 0, 0) and dst.num_blocks() == 0
        fuse(dst, *tiny_frames(0, 4))
        (st,) = merges_that_leave_untouched(dst, [lambda: dst.integrate_volume(src, T)])
        assert st.as_tuple() == (1, 0, 0, 0, 0)


# d ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.RIM_TRANSFORMS))
def test_rim_of_the_key_range(name):
    """hv_key_in_range: the drop of out-of-range candidates in k_merge_candidates and the guard in hv_tsdf_unit.  Units at
    +-2^20 and the unit (-2^20, 1, -2^20) that (2^20, 0, -2^20) would pack to: a corner fetch beyond the rim must find nothing,
    not the alias (the trilinear / nearest split of the stats shows it), and units shifted out of the range are dropped silently."""
    T = ps.RIM_TRANSFORMS[name]
    src = planted(ps.rim_source(alias=True))
    dst = volume(VOX, TRUNC)
    after, st = merge_and_check(dst, src, T, f"rim {name}", on_a_boundary=True)
    assert st.units_source == 4 and np.abs(after[0]).max() <= ps.B and after[0].min() >= -ps.B and after[0].max() < ps.B
    plain = planted(ps.rim_source(alias=False))
    alone, st_plain = merge_and_check(volume(VOX, TRUNC), plain, T, f"rim {name} without the alias", on_a_boundary=True)
    assert st_plain.as_tuple()[:2] == (3, RIM_EXPECTED[name])
    rows = [i for i, k in enumerate(after[0].tolist()) if tuple(k) in set(map(tuple, alone[0].tolist()))]
    assert_bitwise(tuple(x[rows] for x in after), alone)  # the alias unit fed no voxel that is not its own
    assert dst.dropped_points() == 0


# e ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filled", [False, True], ids=["empty", "overlapping"])
def test_far_from_the_origin(sparse_states, filled):
    """hv_merge_locate at |i| ~ 1e7 voxels (a translation of 250 km with GENERIC's rotation): d = (i + 0.5) voxel - t cancels
    seven digits, and the result must still be the restatement's bit for bit; unit indices ~ 6e5 in the key set and the table."""
    T = SPARSE_TRANSFORMS["far"]
    src = planted(sparse_states)
    dst = volume(VOX, TRUNC)
    if filled:
        dst = planted(overlapping_destination(mr.merge_reference(mr.empty_dump(), src.dump(), T, VOX)[0][0]))
    after, st = merge_and_check(dst, src, T, "far")
    assert np.abs(after[0]).max() > 400000 and st.as_tuple()[2:] == SPARSE_STATS["far"][2:]


@pytest.mark.parametrize("metres", [2.1e7, 1.0e8])
def test_translations_beyond_the_lattice(sparse_states, metres):
    """The |g| >= 1e9 clauses of k_merge_candidates and hv_merge_locate: nothing is a candidate, the stats are
    (units_source, 0, 0, 0, 0) and a filled destination is left exactly as it was, caches included."""
    T = np.eye(4)
    T[0, 3] = metres
    src = planted(sparse_states)
    dst = volume(VOX, TRUNC)
    fuse(dst, *tiny_frames(0, 4))
    (st,) = merges_that_leave_untouched(dst, [lambda: dst.integrate_volume(src, T)])
    assert st.as_tuple() == (26, 0, 0, 0, 0) == mr.merge_reference(dst.dump(), src.dump(), T, VOX)[1]


# f ---------------------------------------------------------------------------------------------------------------------------
def test_unsynchronised_call_order():
    """The call's own ordering (both batch pipelines drained, the source's pending work waited for): integrate_batch queued on
    src and on dst, then integrate_volume at once - bitwise the result of twins that synchronised first."""
    import torch

    s, frames = tiny_frames(0, 24)
    d, c, T = stack(frames)
    dev = cuda(d, c)
    results = []
    for synchronise in (False, True):
        src, dst = volume(VOX, TRUNC), volume(VOX, TRUNC)
        torch.cuda.synchronize()
        src.integrate_batch(dev[0][:16], dev[1][:16], intrinsic(s), np.ascontiguousarray(T[:16]))
        dst.integrate_batch(dev[0][8:], dev[1][8:], intrinsic(s), np.ascontiguousarray(T[8:]))
        if synchronise:
            src.synchronize()
            dst.synchronize()
            torch.cuda.synchronize()
        st = dst.integrate_volume(src, GENERIC)
        results.append((dst.dump(), st.as_tuple()))
    assert results[0][1] == results[1][1] and results[0][1][2] > 0
    assert_bitwise(results[0][0], results[1][0])


def test_destination_with_released_slots(sparse_states):
    """k_merge_claim into a table and a pool that prune() has edited: units released (all-zero units among the planted ones), their
    blocks handed out again by the claim."""
    T = SPARSE_TRANSFORMS["diag60"]
    src = planted(sparse_states)
    result_keys = mr.merge_reference(mr.empty_dump(), src.dump(), T, VOX)[0][0]
    keys, tsdf, weight, colour = overlapping_destination(result_keys)
    weight[1::3] = 0.0  # every third unit holds nothing
    dst = planted(ps.finish(keys, tsdf, weight, colour))
    n = dst.num_blocks()
    pruned = dst.prune()
    assert pruned.units_empty == len(keys[1::3]) > 10 and dst.num_blocks() == n - pruned.units_empty
    after, st = merge_and_check(dst, src, T, "diag60 into a pruned destination")
    assert st.units_claimed >= pruned.units_empty and dst.max_blocks() == 1 << 12


def test_compacted_source(sparse_states):
    """hv_merge_resolve / k_merge_candidates on a source whose pool prune() has compacted (a bounded prune: survivors moved into
    the holes, the table re-keyed): block_keys[unit] and the table must still name the same units."""
    T = SPARSE_TRANSFORMS["z45"]
    src = planted(sparse_states)
    n = src.num_blocks()
    pruned = src.prune(empty=False, bounds=((-0.60, -0.60, -0.30), (0.30, 0.30, 0.30)))
    assert 0 < pruned.units_outside < n and src.num_blocks() == pruned.units_after >= 8
    print("compacted source:", pruned.as_tuple())
    merge_and_check(volume(VOX, TRUNC), src, T, "z45 from a compacted source")


def test_merging_the_same_source_twice(sparse_states):
    """The update formula with tsdf0 = (float) tsdf_s and w0 = w_s: weights and colour sums exactly double, tsdf moves by at most
    one float32 rounding."""
    src = planted(sparse_states)
    dst = volume(VOX, TRUNC)
    once, st1 = merge_and_check(dst, src, GENERIC, "generic, first")
    twice, st2 = merge_and_check(dst, src, GENERIC, "generic, second")
    assert st2.units_claimed == 0 and st2.as_tuple()[2:] == st1.as_tuple()[2:]
    assert_doubled(once, twice)
