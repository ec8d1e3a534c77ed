"""The scripts of tests/lifetime_cases.py run through the restatements alone (oracle.PortTsdf, deintegrate_reference, prune_reference,
merge_reference, components_reference, pack_reference), every step from the previous step's reference dump - no GPU.

What is held here is what keeps tests/test_gpu_lifetime.py from passing vacuously: every step changes the map unless it is named
`nothing`, the prune of slots_move releases units from the middle of the key order and the fuse behind it claims a unit next to a
kept one, pool_grows crosses its pool of 64 blocks, every removal removes and keeps, every de-integration reaches the fresh and the
remaining branch, the surface changes between two ticks that extract, and the writer-follows-writer and warm-reader coverage the
module docstring of lifetime_cases states is computed from the lists.
"""
import functools
import itertools
import time

import numpy as np
import pytest

from tests import lifetime_cases as lc
from tests import planted_states as ps

NAMES = sorted(lc.SCRIPTS)
IDENTITY_OPS = ("repack", "mark_merged")


@functools.lru_cache(maxsize=None)
def run(name):
    """-> [(step, dump before, dump after, stats, extra)] of the script, and the seconds it took.  Shared: never written to."""
    script = lc.SCRIPTS[name]
    dump, out, t0 = lc.start_dump(script), [], time.time()
    for step in script.steps:
        after, stats, extra = lc.reference_step(dump, step)
        out.append((step, dump, after, stats, extra))
        dump = after
    return out, time.time() - t0


def key_set(keys):
    return {tuple(int(x) for x in k) for k in np.asarray(keys).reshape(-1, 3)}


@pytest.mark.parametrize("name", NAMES)
def test_every_step_changes_the_map_unless_it_is_named_nothing(name):
    records, seconds = run(name)
    units = [len(lc.start_dump(lc.SCRIPTS[name])[0])] + [len(after[0]) for _, _, after, _, _ in records]
    print(f"{name}: {len(records)} steps, units {units[0]} at the start, {max(units)} at most, restatements {seconds:.1f} s")
    assert max(units) <= 150  # the size guide
    assert (units[0], max(units)) == lc.UNITS[name]  # what the module docstring of lifetime_cases states
    for k, (step, before, after, stats, _) in enumerate(records):
        if step.nothing or step.op in IDENTITY_OPS:
            assert lc.same_bits(before, after), (name, k, step.op)
        else:
            assert not lc.same_bits(before, after), (name, k, step.op, "changes nothing")
    if name == "pipeline_no_ops":
        hollow = [stats for step, _, _, stats, _ in records if step.op == "merge"]
        assert hollow == [(0, 0, 0, 0, 0)]
    for step, _, _, stats, _ in records:
        if step.op == "prune" and step.nothing:
            assert stats[1] == stats[2] == 0


def test_script_lengths_and_pipeline_pattern():
    for name in lc.NAMED:
        assert 8 <= len(lc.SCRIPTS[name].steps) <= 14, name
    others = []
    for name in lc.PIPELINE:
        ops = [s.op for s in lc.SCRIPTS[name].steps]
        for k in range(2, len(ops) - 1):
            if ops[k] != "fuse_batch" or lc.SCRIPTS[name].steps[k].arg.count == 1:
                assert ops[k - 2] == ops[k - 1] == ops[k + 1] == "fuse_batch", (name, k)
                step = lc.SCRIPTS[name].steps[k]
                others.append((step.op, step.nothing))
    assert sorted(others) == sorted([("read_mesh", True), ("ray_cast", True), ("sample_points", True), ("remove_small", True),
                                     ("remove_small", False), ("merge", True), ("deintegrate_batch", False), ("fuse", False), ("prune", True)])
    cameras = [s.arg.camera for name in lc.PIPELINE for s in lc.SCRIPTS[name].steps if s.op == "fuse_batch"]
    assert "other" in cameras and cameras[0] == "tiny"
    seen = set()
    for name in ("gather_a", "gather_b"):  # mark_merged directly behind every writer, every writer op in one of the two
        gather = lc.SCRIPTS[name].steps
        assert all(gather[k + 1].op == "mark_merged" for k, s in enumerate(gather) if lc.writer_op(s))
        seen |= {lc.writer_op(s) for s in gather if lc.writer_op(s)}
    assert seen == set(lc.WRITER_OPS)


def test_slots_move_releases_from_the_middle_and_fuses_next_to_a_kept_unit():
    records, _ = run("slots_move")
    steps = [r[0].op for r in records]
    k = steps.index("prune")
    assert steps[k + 1] == "fuse_batch" and records[k][0].tick == ()
    _, before, after, stats, _ = records[k]
    released = np.array([tuple(key) not in key_set(after[0]) for key in before[0].tolist()])
    assert stats[2] == released.sum() >= 3 and np.flatnonzero(released).max() < len(released) - 1
    assert (np.flatnonzero(released) < len(released) - 1).sum() >= 3
    _, kept, fused, _, _ = records[k + 1]
    held, new = key_set(kept[0]), key_set(fused[0]) - key_set(kept[0])
    adjacent = [n for n in new if any(tuple(np.add(n, d)) in held for d in itertools.product((-1, 0, 1), repeat=3))]
    assert len(adjacent) >= 1
    index = {tuple(key): i for i, key in enumerate(fused[0].tolist())}
    written = [key for i, key in enumerate(kept[0].tolist()) if not np.array_equal(kept[2][i], fused[2][index[tuple(key)]])]
    assert len(written) >= 1
    print(f"slots_move: {int(released.sum())} units released, {len(new)} claimed ({len(adjacent)} next to a kept unit), {len(written)} held units written")


def test_pool_grows_crosses_its_pool_and_the_merge_claims():
    records, _ = run("pool_grows")
    script = lc.SCRIPTS["pool_grows"]
    assert script.max_blocks == 64
    crossing = [k for k, (_, before, after, _, _) in enumerate(records) if len(before[0]) <= 64 < len(after[0])]
    assert crossing, [len(r[2][0]) for r in records]
    k = crossing[0]
    ticks = [t for r in records[:k] for t in r[0].tick]
    assert "mesh" in ticks and ("points" in ticks or "normals" in ticks)  # unit masks, classification and point counts are warm
    merges = [stats for step, _, _, stats, _ in records if step.op == "merge"]
    assert merges and all(stats[1] >= 1 for stats in merges), merges
    assert "repack" in [r[0].op for r in records]


@pytest.mark.parametrize("name", NAMES)
def test_every_removal_removes_and_keeps_and_every_deintegration_reaches_both_branches(name):
    for k, (step, before, after, stats, extra) in enumerate(run(name)[0]):
        if step.op == "remove_small":
            if step.nothing:
                assert stats[1] == stats[3] == stats[4] == 0
            else:
                assert stats[1] >= 1 and stats[0] - stats[1] >= 1 and stats[4] >= 1, (name, k, stats)
        if step.op in ("deintegrate_batch", "reintegrate_batch"):
            n, _, _ = ps.sample_counts(before[0], lc.samples_for(step.arg))
            under, fresh, rest = ps.removal_classes(before[2], n)
            print(f"{name} step {k}: underflow {under.sum()}, fresh {fresh.sum()}, remaining {rest.sum()}, stats {stats}")
            assert fresh.sum() >= 100 and rest.sum() >= 100, (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_the_surface_changes_between_two_ticks_that_extract(name):
    last = None
    for k, (step, _, after, _, _) in enumerate(run(name)[0]):
        if not step.tick and step.op != "read_mesh":
            continue
        mark = lc.sign_changes(after)
        assert mark[0] > 0, (name, k, "no surface")
        assert mark != last, (name, k, mark)
        last = mark


def test_writer_pairs_and_warm_readers_are_covered():
    pairs = lc.pair_coverage()
    missing = [(a, b) for a in lc.WRITER_OPS for b in lc.WRITER_OPS if a != b and (a, b) not in pairs]
    assert not missing, missing
    assert all(mesh and points for mesh, points in lc.warm_coverage().values()), lc.warm_coverage()
    for name in lc.SCRIPTS:  # every script ends with a tick that reads everything
        assert set(lc.SCRIPTS[name].steps[-1].tick) == set(lc.ALL), name
