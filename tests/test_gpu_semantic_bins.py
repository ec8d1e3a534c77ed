"""GPU: the per-call point bins of the four semantic payloads (hv_bins.h, k_semb_bin / k_semb_fold_wave / k_semb_fold_tasks of
hv_semantic.hip) at planted bin sizes, orders and pages, against the compiled reference (oracle/_ref: RefSemGrid2) after every call.

What is planted (tests/bin_cases.py; tests/test_bin_cases_cpu.py holds the inputs to what they claim): one block per size of the ladder
1 2 63 64 65 127 128 129 255 256 257 511 512 513 1023 1024 1025 1537 - each side of the readlane ranking (64), the staged records of
the frame source (128), the inline entries (256), the wave's LDS window (512: counting sort below, 64-voxel range tasks above) and the
page boundaries - with a bin's points in one voxel, all different voxels, two alternating, at random, in the first and last voxel;
contiguous, round-robin or shuffled in the call, or in explicit point-index runs; through the point-array source and through the frame
source (integrate_rgbd: HvSemRecs); at block sizes 4 (one range), 5 (odd), 8, 12 (27 ranges, the largest offsets window that fits the
LDS) and 16 (the fold's LDS exceeds 64 KiB: the radix path has to give the same state).  Labels are drawn so that the voting counters
depend on the order of a voxel's points; depths fall on both sides of the depth thresholds.

The bars are the project's own (tests/test_gpu_semantic_ops.py::assert_state_equal): counts, position and colour sums exact for all four
payloads, the voting payloads (kinds 0 and 2) bit for bit, the log-probability payloads' confidences within 2e-6 and
(int)(confidence * count) within 1.

Measured on the MI355X when the file was written: 176 cases (44 per payload), all within the bars above, 10.5 s for the file (the slowest
case, the chained calls of the probabilistic payloads, 0.7 s).  Largest bin per call: 1537 in the ladder calls (7 496 points) and in the
one-voxel call (12 288 points), 1025 in the range calls and the frame source (5 955 valid pixels), 600 in the chained calls.
"""
import numpy as np
import pytest

import oracle
from oracle.semantic import RefSemGrid2
from tests import bin_cases as bc
from tests.semantic_helpers import frame_points
from tests.test_gpu_semantic_ops import ALL_KINDS, EXACT, assert_state_equal
from tests.test_gpu_semantic_ops import restore_reference_statics  # noqa: F401  (autouse: the reference's static thresholds)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not oracle.ref_available(), reason="compiled reference not available")]


def grids(kind, bs=8, max_blocks=1 << 8, max_points=1 << 14):
    """The GPU grid and the compiled reference's, thresholds as in tests/test_gpu_semantic2_payloads.py (voting 10, log-probability 5,
    decay 0.07)."""
    from pyslam_amd import volumetric_semantic as vs

    cls = (vs.VoxelBlockSemanticGrid, vs.VoxelBlockSemanticProbabilisticGrid, vs.VoxelBlockSemanticGrid2, vs.VoxelBlockSemanticProbabilisticGrid2)[kind]
    gpu, ref = cls(bc.VOXEL, bs, max_blocks=max_blocks, max_points=max_points), RefSemGrid2(kind, bc.VOXEL, bs)
    for g in (gpu, ref):
        g.set_depth_threshold(10.0 if kind in EXACT else 5.0)
        g.set_depth_decay_rate(0.07)
    return gpu, ref


def feed(gpu, ref, kind, call, use_inst=True, use_depth=True):
    for g in (gpu, ref):
        g.integrate(*call.semantic_args(use_inst, use_depth))
    assert gpu.dropped_points() == 0 and gpu.label_overflows() == 0
    assert_state_equal(gpu, ref, kind)


def check_ladder(kind, layout, placement, dtype=np.float32, bs=8, use_inst=True, use_depth=True):
    """The whole ladder, 1537 included, in one call, then another draw of it onto the labelled voxels."""
    gpu, ref = grids(kind, bs)
    for seed in (5, 6):
        feed(gpu, ref, kind, bc.sem_ladder(layout, placement, dtype, bs, seed), use_inst, use_depth)
    assert gpu.num_blocks() == len(bc.SEM_LADDER) + 1


@pytest.mark.parametrize("placement", bc.PLACEMENTS)
@pytest.mark.parametrize("layout", bc.LAYOUTS)
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_ladder_array_source(kind, layout, placement):
    check_ladder(kind, layout, placement)


@pytest.mark.parametrize("use_inst,use_depth", [(True, False), (False, True), (False, False)])
@pytest.mark.parametrize("layout,placement", [("random", "shuffled"), ("one_voxel", "contiguous")])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_ladder_without_instance_ids_or_depths(kind, layout, placement, use_inst, use_depth):
    check_ladder(kind, layout, placement, use_inst=use_inst, use_depth=use_depth)


@pytest.mark.parametrize("layout,placement", [("random", "shuffled"), ("two_alternating", "round_robin"), ("ends", "contiguous")])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_ladder_float64_points(kind, layout, placement):
    check_ladder(kind, layout, placement, np.float64)


@pytest.mark.parametrize("bs,layout", [(4, "random"), (5, "random"), (5, "ends"), (12, "random"), (12, "distinct"), (12, "ends"), (16, "random")])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_ladder_block_sizes(kind, bs, layout):
    """bs 4: 64 voxels, one range.  bs 5: 125 voxels.  bs 12: 1728 voxels in 27 ranges, the largest offsets window that still fits the LDS.
    bs 16: sem_bins_usable is false (the fold's LDS would exceed 64 KiB) - the radix path, the same state."""
    check_ladder(kind, layout, "shuffled", bs=bs)


@pytest.mark.parametrize("bs", [8, 12])
@pytest.mark.parametrize("name", ["one_voxel_1537_windowed", "one_range_1025", "all_ranges_1025"])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_big_bins(kind, name, bs):
    """Bins beyond the 512-entry window go to k_semb_fold_tasks as 64-voxel ranges.  1537 points in ONE voxel: its range overflows the
    window and is folded in point-index windows of 512 - one of them filled by that voxel alone, one empty, runs across their ends.
    1025 points in one range: the same overflow with 64 runs.  1025 points over all ranges: every range fits."""
    call = bc.sem_big_calls(bs)[name]
    gpu, ref = grids(kind, bs, max_blocks=1 << 9)
    feed(gpu, ref, kind, call)
    feed(gpu, ref, kind, call)


@pytest.mark.parametrize("layout,placement", [("random", "shuffled"), ("one_voxel", "contiguous"), ("distinct", "round_robin"), ("ends", "shuffled"),
                                              ("two_alternating", "shuffled")])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_frame_source_ladder(kind, layout, placement):
    """The ladder planted through integrate_rgbd with label images and use_depths (HvSemRecs): the staged-record fold at 127 / 128 / 129,
    the readlane ranking at 63 / 64 / 65.  Reference side: the host prep of the keyframe flow + integrate."""
    fr = bc.frame_call(bc.VOXEL, 8, bc.FRAME_LADDER, layout, placement, 50)
    gpu, ref = grids(kind)
    for _ in range(2):
        gpu.integrate_rgbd(fr.depth, fr.rgb, *fr.intrinsics, fr.T_cw, class_ids_image=fr.cls, object_ids_image=fr.inst, max_depth=20.0,
                           use_depths=True)
        pts, cols, cls, obj, depths = frame_points(fr.depth, fr.rgb, fr.T_cw, fr.cls, fr.inst, fr.intrinsics, 20.0)
        ref.integrate(pts.astype(np.float32), cols, cls, obj, depths)
        assert gpu.dropped_points() == 0 and gpu.label_overflows() == 0
        assert_state_equal(gpu, ref, kind)
    keys, ints = gpu.dump2()[:2]
    np.testing.assert_array_equal(keys, fr.call.keys)
    np.testing.assert_array_equal(ints[..., 0].sum(axis=1), 2 * fr.call.sizes)


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_chained_calls_stale_places_and_first_points(kind):
    """The sequences of tests/test_gpu_voxel_grid_bins.py on a semantic grid: stale inline places and pages under a new epoch and the other
    parity, a clear(), 512 first points of 512 new blocks in every bin-pass workgroup, one workgroup plus one thread - then the ladder
    onto labelled voxels."""
    gpu, ref = grids(kind, max_blocks=1 << 11)
    a, b, c, d = bc.stale_calls()
    for call in (a, b, c, a, d, b):
        feed(gpu, ref, kind, call)
    gpu.clear()
    ref.clear()
    assert gpu.num_blocks() == 0
    feed(gpu, ref, kind, a)
    first, second = bc.firsts_calls()
    feed(gpu, ref, kind, first)
    feed(gpu, ref, kind, second)
    feed(gpu, ref, kind, bc.sem_ladder("random", "shuffled"))
    feed(gpu, ref, kind, bc.sem_ladder("one_voxel", "round_robin", seed=7))


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_sort_path_gives_the_same_state(kind, monkeypatch):
    """HV_SEM_PATH=sort (the device-wide radix sort) on the ladder and the 1537-point voxel: identical dumps for the voting payloads,
    within the log-probability bar of the reference for the other two."""
    calls = [bc.sem_ladder("random", "shuffled"), bc.sem_big_calls()["one_voxel_1537_windowed"], bc.sem_ladder("two_alternating", "contiguous", seed=8)]
    dumps = {}
    for path in ("bins", "sort"):
        if path == "sort":
            monkeypatch.setenv("HV_SEM_PATH", "sort")
        gpu, ref = grids(kind, max_blocks=1 << 9)
        for call in calls:
            feed(gpu, ref, kind, call)
        dumps[path] = gpu.dump2()[:5]
    (kb, ib, pb, cb, fb), (ks, js, ps, cs, fs) = dumps["bins"], dumps["sort"]
    for a, b in ((kb, ks), (ib[..., :3], js[..., :3]), (pb, ps), (cb, cs)):  # keys; count, object id, class id; position and colour sums
        np.testing.assert_array_equal(a, b)
    if kind in EXACT:
        np.testing.assert_array_equal(ib[..., 3], js[..., 3])
        np.testing.assert_array_equal(fb, fs)
