"""GPU: the per-call point bins of the VOXEL_GRID integrate (hv_bins.h, k_vgb_bin / k_vgb_fold_wave / k_vgb_fold of hv_voxel_grid.hip)
at planted bin sizes, orders and pages, bitwise against the compiled reference (oracle/_ref) / its C restatement after EVERY call.

What is planted (tests/bin_cases.py; tests/test_bin_cases_cpu.py holds the inputs to what they claim): one block per size of the ladder
1 2 63 64 65 127 128 129 255 256 257 511 512 513 767 768 769 1023 1024 1025 (4095 4096 4097 5000) - each side of the staged fold
(128), the register rank sort (256 = the inline entries of a slot), the page boundaries (256 + 256 k), the wave's LDS window (1024) and
the workgroup's (4096) - with a bin's points in one voxel, in all different voxels, alternating between two, at random and in the first
and last voxel of the block; contiguous in the call (lane groups of 64 across the inline / page boundary), round-robin, shuffled, or in
explicit point-index runs that fill a window, leave one empty and straddle its ends.  Positions, colours and the order of a voxel's
points decide the float32 sums: a fold that drops, repeats or swaps ONE entry of one of these bins changes bits of the dump.

Why: the bit-exact claim of this mode rests on rebuilding point order from bins that were filled in atomic order, by code that changes
form at exactly these sizes; workload-shaped data reaches the forms but pins no bin to their edges.

Measured on the MI355X when the file was written: 93 cases, all equal to the compiled reference bit for bit, 5.4 s for the file (the slowest
case, the form sequence on both paths, 0.54 s).  Largest bin per call: 1025 in the ladder calls (8 263 points), 5000 in the form sequence's
second and third call (53 248 points, 1 393 blocks), 600 in the stale-places calls, 1 in the first-point calls, 257 in the call of
2^17 points.
"""
import numpy as np
import pytest

from oracle import host_prep as hp
from tests import bin_cases as bc
from tests.test_gpu_voxel_grid import assert_same_grid, make_oracle

pytestmark = pytest.mark.gpu


def grid(bs=8, max_blocks=1 << 9, max_points=1 << 14):
    from pyslam_amd.volumetric import VoxelBlockGrid

    return VoxelBlockGrid(bc.VOXEL, bs, max_blocks=max_blocks, max_points=max_points)


def feed(gpu, cpu, call):
    gpu.integrate(*call.grid_args())
    cpu.integrate(*call.grid_args())
    assert gpu.dropped_points() == 0
    assert_same_grid(gpu, cpu)


def check_ladder(layout, placement, color, dtype=np.float32, bs=8):
    """The ladder up to 1025 in one call, then once more (another draw) onto the voxels it filled: stale entries of equal length in
    every place, the other parity, sums that start from non-zero values."""
    gpu, cpu = grid(bs), make_oracle(bc.VOXEL, bs)
    for seed in (1, 2):
        feed(gpu, cpu, bc.vg_ladder(layout, placement, color, dtype, bs, seed))
    assert gpu.num_blocks() == len(bc.VG_LADDER_WAVE) + 1


@pytest.mark.parametrize("color", ["f32", "u8", "none"])
@pytest.mark.parametrize("placement", bc.PLACEMENTS)
@pytest.mark.parametrize("layout", bc.LAYOUTS)
def test_ladder(layout, placement, color):
    check_ladder(layout, placement, color)


@pytest.mark.parametrize("placement", bc.PLACEMENTS)
@pytest.mark.parametrize("layout", bc.LAYOUTS)
def test_ladder_float64_points(layout, placement):
    """(Against the compiled reference's double overload where it is built; the C restatement narrows first, which is the same here:
    no point is near a cell border.)"""
    check_ladder(layout, placement, "u8", np.float64)


@pytest.mark.parametrize("placement", bc.PLACEMENTS)
@pytest.mark.parametrize("bs,layout", [(4, "random"), (4, "ends"), (5, "random"), (5, "distinct"), (5, "ends"), (16, "ends"), (16, "random")])
def test_ladder_block_sizes(bs, layout, placement):
    """bs 4 (64 voxels: every ladder bin beyond 64 repeats voxels), bs 5 (odd), bs 16: local_bits = 12 = 32 - HV_VGB_IDX_BITS, the widest
    voxel index an entry can hold - with `ends`, local voxel 4095 carries the call's highest point indices."""
    check_ladder(layout, placement, "f32", bs=bs)


def form_sequence(color):
    full = bc.vg_full_ladder(color=color)
    return [bc.vg_small_ladder(color=color), full, full] + bc.vg_two_small(color=color)


def run_form_sequence(gpu, cpu, calls):
    dumps = []
    for call in calls:
        feed(gpu, cpu, call)
        dumps.append(gpu.dump())
    return dumps


@pytest.mark.parametrize("color", ["f32", "u8"])
def test_form_sequence_wave_workgroup_wave(color):
    """One grid, checked after each call.  Which fold kernel runs follows from the largest bin of the call BEFORE (status->pad, read by
    the host at the next call; not observable from Python), so by construction:
      1. the ladder up to 1024                                     wave form (k_vgb_fold_wave), every bin in one sort;
      2. the whole ladder, 1025 4095 4096 4097 5000 in explicit     still the wave form: those five bins in point-index windows of
         point-index runs                                          1024 (full, empty and straddled windows);
      3. the same call again                                        workgroup form (k_vgb_fold): up to 4096 in one sort, 4097 and 5000
                                                                   in windows of 4096, onto voxels that already hold counts;
      4. a small call                                              still the workgroup form (call 3 had big bins);
      5. another small call                                        back in the wave form."""
    calls = form_sequence(color)
    assert max(calls[0].sizes) == bc.HV_VGB_WCAP and max(calls[1].sizes) > bc.HV_VGB_CAP and max(calls[3].sizes) < bc.HV_VGB_WCAP
    gpu, cpu = grid(max_blocks=1 << 12, max_points=1 << 16), make_oracle(bc.VOXEL)
    run_form_sequence(gpu, cpu, calls)


def test_form_sequence_on_the_sort_path_dumps_identically(monkeypatch):
    calls = form_sequence("f32")
    bins = run_form_sequence(grid(max_blocks=1 << 12, max_points=1 << 16), make_oracle(bc.VOXEL), calls)
    monkeypatch.setenv("HV_VG_PATH", "sort")
    sort = run_form_sequence(grid(max_blocks=1 << 12, max_points=1 << 16), make_oracle(bc.VOXEL), calls)
    for a, b in zip(bins, sort):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


def test_growth_under_the_ladder():
    """The second call of the form sequence brings ~1400 new blocks into a pool of 1024: its claim pass does not fit, the pool grows
    inside the call, the bin pass runs again on bins that restart from cleared arrays (bins_clean = false) and a table that moved.
    Bitwise the oracle's result and that of a roomy pool."""
    calls = form_sequence("u8")
    small, roomy, cpu = grid(max_blocks=1024, max_points=1 << 16), grid(max_blocks=1 << 12, max_points=1 << 16), make_oracle(bc.VOXEL)
    assert len(calls[1].keys) > 1024
    for k, call in enumerate(calls):
        before = small.max_blocks()
        roomy.integrate(*call.grid_args())
        feed(small, cpu, call)
        assert (small.max_blocks() > before) == (k == 1) or k > 1, (k, before, small.max_blocks())  # (later calls may grow ahead)
        for a, b in zip(small.dump(), roomy.dump()):
            np.testing.assert_array_equal(a, b)


def test_stale_places_pages_and_parity():
    """A: 600 points in each of 12 blocks.  B: 10 points in the same blocks - their inline places and both pages still hold A's entries
    beyond nb - and 300 in 12 other blocks, whose page 0 is claimed under the new epoch with 44 entries; the parity flips.  C: nine other
    blocks.  D: 300 points in A's blocks (page 0 of each claimed again under a new epoch with 44 entries where A left 256, page 1 still
    A's) and 600 in B's others.  Then clear() and A again: the bins of a cleared grid."""
    gpu, cpu = grid(), make_oracle(bc.VOXEL)
    a, b, c, d = bc.stale_calls()
    for call in (a, b, c, a, d, b, a):
        feed(gpu, cpu, call)
    gpu.clear()
    cpu.clear()
    assert gpu.num_blocks() == 0
    feed(gpu, cpu, a)
    feed(gpu, cpu, b)


def test_512_first_points_per_workgroup():
    """1536 points in 1536 new blocks: each of the three bin-pass workgroups appends HV_BIN_THREADS slots to the touched lists and takes
    HV_BIN_THREADS pool indices - s_first / s_new_slot / s_new_key filled to their last entry.  Then 513 points in 513 blocks (256 of
    them new): one full workgroup plus one thread."""
    gpu, cpu = grid(max_blocks=1 << 12), make_oracle(bc.VOXEL)
    a, b = bc.firsts_calls()
    feed(gpu, cpu, a)
    assert gpu.num_blocks() == 3 * bc.HV_BIN_THREADS
    feed(gpu, cpu, b)
    assert gpu.num_blocks() == 3 * bc.HV_BIN_THREADS + 256
    feed(gpu, cpu, a)


def test_many_pages_at_max_points():
    """max_points = 2^17 points in one call (the n <= max_points edge of hv_bins_usable) in 510 blocks of 257 points and one of 2:
    every block owns a page that holds ONE entry - 510 of the page table's 2048 slots."""
    gpu, cpu = grid(max_blocks=1 << 10, max_points=1 << 17), make_oracle(bc.VOXEL)
    call = bc.many_pages_call(1 << 17)
    assert call.n == 1 << 17
    feed(gpu, cpu, call)
    feed(gpu, cpu, bc.vg_small_ladder(color="u8"))


@pytest.mark.parametrize("layout,placement", [("random", "shuffled"), ("one_voxel", "contiguous"), ("distinct", "round_robin"), ("ends", "shuffled"),
                                              ("two_alternating", "shuffled")])
def test_frame_source_ladder(layout, placement):
    """The ladder planted through integrate_rgbd (HV_REC_U8_DIV records, the unprojection fused into the bin pass): a long focal length
    puts every pixel into one voxel column, the depth alone picks block and voxel.  Reference side: the host prep + integrate."""
    fr = bc.frame_call(bc.VOXEL, 8, bc.FRAME_LADDER, layout, placement, 50)
    gpu, cpu = grid(), make_oracle(bc.VOXEL)
    for _ in range(2):
        gpu.integrate_rgbd(fr.depth, fr.rgb, *fr.intrinsics, fr.T_cw)
        pts, cols, _ = hp.frame_to_world_f32(fr.depth, fr.rgb, *fr.intrinsics, fr.T_cw, np.inf)
        cpu.integrate(pts, cols)
        assert gpu.dropped_points() == 0
        assert_same_grid(gpu, cpu)
    keys, _, counts, _ = gpu.dump()
    np.testing.assert_array_equal(keys, fr.call.keys)
    np.testing.assert_array_equal(counts.sum(axis=1), 2 * fr.call.sizes)
