"""CPU: the planted inputs of tests/bin_cases.py against the CPU oracles - the conditions under which the GPU files
tests/test_gpu_voxel_grid_bins.py and tests/test_gpu_semantic_bins.py test what they say they test.

* the constants behind the ladders are the ones in hv_bins.h, hv_voxel_grid.hip and hv_semantic.hip;
* every call plants exactly the listed blocks with exactly the listed point counts (oracle.PortGrid, and the compiled reference's
  RefGrid / RefSemGrid2 where it is built);
* every call is order-sensitive: fed in reversed point order, each bin that CAN change does.  A float32 sum can change only in a voxel
  that takes three or more points (0 + a + b is commutative), a voting label or counter only in a voxel that takes two or more: the
  condition is asked of every bin with such a voxel (the `distinct` layout below bs^3 points has none - it is there for the sort, not
  for the fold order);
* the windowed placement really holds a full window, an empty window between two of a bin's points and a straddling run."""
import os
import re

import numpy as np
import pytest

import oracle
from oracle import host_prep as hp
from oracle.semantic import PortSemGrid2
from tests import bin_cases as bc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyslam_amd", "csrc")


def test_constants_are_the_sources():
    for name, constants in bc.CONSTANT_SOURCES.items():
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for c in constants:
            m = re.findall(r"static constexpr int %s = (\d+);" % c, text)
            assert len(m) == 1, (name, c)
            assert int(m[0]) == getattr(bc, c), (name, c)
    with open(os.path.join(CSRC, "hv_semantic.hip")) as f:
        m = re.findall(r"static int sem_wcap\(\) \{ return (\d+); \}", f.read())
    assert len(m) == 1 and int(m[0]) == bc.SEM_WCAP
    assert bc.VG_LADDER == [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 4095, 4096, 4097, 5000]
    assert bc.SEM_LADDER == [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1537]
    assert bc.HV_VGB_RANK <= bc.HV_BIN_K0  # the rank sort reads inline entries only


def point_calls():
    """(name, Call) of the point calls the GPU files make."""
    out = []
    for layout in bc.LAYOUTS:
        for placement in bc.PLACEMENTS:
            out.append((f"vg_ladder-{layout}-{placement}", bc.vg_ladder(layout, placement, "f32")))
            out.append((f"sem_ladder-{layout}-{placement}", bc.sem_ladder(layout, placement)))
    out.append(("vg_ladder-f64", bc.vg_ladder("random", "shuffled", "u8", np.float64)))
    out.append(("sem_ladder-f64", bc.sem_ladder("random", "shuffled", np.float64)))
    for bs in (4, 5, 16):
        for layout in ("ends", "random"):
            out.append((f"vg_ladder-bs{bs}-{layout}", bc.vg_ladder(layout, "shuffled", "u8", bs=bs)))
    for bs in (4, 5, 12, 16):
        out.append((f"sem_ladder-bs{bs}", bc.sem_ladder("random", "shuffled", bs=bs)))
    out.append(("vg_small_ladder", bc.vg_small_ladder()))
    out.append(("vg_full_ladder", bc.vg_full_ladder()))
    out += [(f"vg_two_small-{k}", c) for k, c in enumerate(bc.vg_two_small())]
    out += [(f"stale-{n}", c) for n, c in zip("ABCD", bc.stale_calls())]
    out += [(f"firsts-{k}", c) for k, c in enumerate(bc.firsts_calls())]
    out.append(("many_pages", bc.many_pages_call()))
    out += [(f"sem_big-bs{bs}-{n}", c) for bs in (8, 12) for n, c in bc.sem_big_calls(bs).items()]
    return out


POINT_CALLS = point_calls()
FRAMES = [(f"frame-{layout}-{placement}", bc.frame_call(bc.VOXEL, 8, bc.FRAME_LADDER, layout, placement, 50))
          for layout, placement in (("random", "shuffled"), ("one_voxel", "contiguous"), ("distinct", "round_robin"), ("ends", "shuffled"),
                                    ("two_alternating", "shuffled"))]


def frame_points(fr):
    pts, cols, valid = hp.frame_to_world_f32(fr.depth, fr.rgb, *fr.intrinsics, fr.T_cw, np.inf)
    assert int(valid.sum()) == fr.call.n
    return pts, cols


def as_point_call(fr):
    pts, cols = frame_points(fr)
    c = fr.call
    return bc.Call(c.voxel, c.bs, pts, cols, c.class_ids, c.instance_ids, c.depths, c.bin_of, c.local, c.keys, c.sizes, c.planted)


ALL_CALLS = POINT_CALLS + [(name, as_point_call(fr)) for name, fr in FRAMES]


def assert_planted(call, dump):
    keys, counts = dump[0], dump[2]
    want = call.voxel_counts()
    assert len(keys) == len(want) == len(call.keys)
    order = np.lexsort(call.keys.T[::-1])
    np.testing.assert_array_equal(keys, call.keys[order])
    np.testing.assert_array_equal(counts.sum(axis=1), call.sizes[order])
    np.testing.assert_array_equal(counts, np.stack([want[tuple(int(x) for x in k)] for k in keys]))


@pytest.mark.parametrize("name,call", ALL_CALLS, ids=[n for n, _ in ALL_CALLS])
def test_planted_sizes_and_keys(name, call):
    assert call.n <= (1 << 17) and np.bincount(call.bin_of, minlength=len(call.sizes)).tolist() == call.sizes.tolist()
    grids = [oracle.PortGrid(call.voxel, call.bs)]
    if oracle.ref_available():
        grids.append(oracle.RefGrid(call.voxel, call.bs))
    for g in grids:
        g.integrate(*call.grid_args())
        assert_planted(call, g.dump())
    if oracle.ref_available() and call.n <= 20000:
        from oracle.semantic import RefSemGrid2

        g = RefSemGrid2(0, call.voxel, call.bs)
        g.integrate(call.points, call.colors if call.colors is not None else np.zeros((call.n, 3), np.uint8), call.class_ids, call.instance_ids,
                    call.depths)
        keys, ints = g.dump()[:2]
        assert_planted(call, (keys, None, ints[..., 0]))


@pytest.mark.parametrize("name,call", ALL_CALLS, ids=[n for n, _ in ALL_CALLS])
def test_reversed_order_changes_every_bin_that_can_change(name, call):
    rev = call.reversed()
    a, b = oracle.PortGrid(call.voxel, call.bs), oracle.PortGrid(call.voxel, call.bs)
    a.integrate(*call.grid_args())
    b.integrate(*rev.grid_args())
    (ka, _, ca, sa), (kb, _, cb, sb) = a.dump(), b.dump()
    np.testing.assert_array_equal(ka, kb)
    np.testing.assert_array_equal(ca, cb)
    sums_differ = (sa.view(np.uint32) != sb.view(np.uint32)).any(axis=(1, 2))
    can = ca.max(axis=1) >= 3
    assert (sums_differ | ~can).all(), (name, ka[can & ~sums_differ], ca.sum(axis=1)[can & ~sums_differ])
    assert not sums_differ[ca.max(axis=1) <= 2].any()
    if call.n > 20000:
        return
    for kind in (0, 2):  # the voting payloads
        a, b = PortSemGrid2(kind, call.voxel, call.bs), PortSemGrid2(kind, call.voxel, call.bs)
        for g in (a, b):
            g.set_depth_threshold(10.0)
        a.integrate(*call.semantic_args())
        b.integrate(*rev.semantic_args())
        (ka, ia, _, _, fa), (kb, ib, _, _, fb) = a.dump(), b.dump()
        np.testing.assert_array_equal(ka, kb)
        labels_differ = (ia[..., 1:] != ib[..., 1:]).any(axis=(1, 2)) | (fa != fb).any(axis=1)
        can = ia[..., 0].max(axis=1) >= 2
        assert (labels_differ | ~can).all(), (name, kind, ka[can & ~labels_differ], ia[..., 0].sum(axis=1)[can & ~labels_differ])


def test_depths_fall_on_both_sides_of_the_thresholds():
    for name, call in POINT_CALLS:
        if (np.bincount(call.bin_of * call.bs ** 3 + call.local) >= 3).sum() >= 20:  # (a run's first two points are near)
            for thr in (5.0, 10.0):
                assert (call.depths < thr).any() and (call.depths > thr).any(), name
    for name, fr in FRAMES:
        d = fr.depth[fr.depth > 0]
        assert (d < 5.0).any() and (d > 5.0).any() and d.max() < 10.0


def test_contiguous_ladder_has_a_lane_group_across_the_inline_boundary():
    for call in (bc.vg_ladder("random", "contiguous"), bc.sem_ladder("random", "contiguous")):
        b = call.sizes.tolist().index(bc.HV_BIN_K0 + 1)
        at = np.nonzero(call.bin_of == b)[0]
        assert (np.diff(at) == 1).all() and at[0] % bc.WAVE == 6
        # lane groups of the bin in launch order: 58, 64, 64, 64, 64 ...: the fifth takes places 250 .. 313 (here: .. 256)
        assert (bc.WAVE - at[0] % bc.WAVE) + 3 * bc.WAVE == bc.HV_BIN_K0 - 6


def test_round_robin_neighbours_lie_in_different_blocks():
    call = bc.vg_ladder("random", "round_robin")
    same = call.bin_of[1:] == call.bin_of[:-1]
    assert same.sum() <= 1  # (the last point of the largest bin)


def test_windowed_placement_holds_full_empty_and_straddling_windows():
    call = bc.vg_full_ladder()
    assert call.n <= (1 << 17)
    big = [b for b in range(call.planted) if call.sizes[b] > bc.HV_VGB_WCAP]
    assert sorted(call.sizes[big].tolist()) == [1025, 4095, 4096, 4097, 5000]
    for cap in (bc.HV_VGB_WCAP, bc.HV_VGB_CAP):  # the wave form's windows, the workgroup form's
        facts = np.array([bc.window_facts(call, b, cap) for b in big if call.sizes[b] > cap])
        assert facts.all(axis=1).any(), (cap, facts)  # one bin shows all three ...
        assert facts.any(axis=0).all()
    # ... and every big bin has a run across a multiple of 512; some across multiples of 1024 and 4096
    assert all(bc.window_facts(call, b, 512)[2] for b in big)
    # the bins within the wave window and the filler blocks lie between the runs
    assert (call.sizes[call.planted:] <= 40).all() and len(call.sizes) > call.planted
    one = bc.sem_big_calls()["one_voxel_1537_windowed"]
    full, empty, straddle = bc.window_facts(one, 0, bc.SEM_WCAP)
    assert full and empty and straddle and one.sizes[0] == 3 * bc.SEM_WCAP + 1
    assert len(np.unique(one.local[one.bin_of == 0])) == 1


def test_big_semantic_bins_cover_one_range_and_all_ranges():
    calls = bc.sem_big_calls()
    one, every = calls["one_range_1025"], calls["all_ranges_1025"]
    r = np.unique(one.local[one.bin_of == 0] // 64)
    assert len(r) == 1 and (one.bin_of == 0).sum() == 2 * bc.SEM_WCAP + 1
    assert len(np.unique(every.local[every.bin_of == 0] // 64)) == 8 and (every.bin_of == 0).sum() == 2 * bc.SEM_WCAP + 1


def test_first_block_calls_fill_the_workgroups():
    a, b = bc.firsts_calls()
    assert a.n == 3 * bc.HV_BIN_THREADS == len(np.unique(a.keys, axis=0))
    assert b.n == bc.HV_BIN_THREADS + 1 == len(np.unique(b.keys, axis=0))
    old = {tuple(k) for k in a.keys.tolist()}
    assert sum(tuple(k) not in old for k in b.keys.tolist()) == 256
    pages = bc.many_pages_call()
    assert pages.n == 1 << 17 and (pages.sizes[:-1] == bc.HV_BIN_K0 + 1).all() and 0 < pages.sizes[-1] <= bc.HV_BIN_K0 + 1
