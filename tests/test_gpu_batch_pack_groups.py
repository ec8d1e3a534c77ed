"""GPU: the frame-grouped pack role of the batch path (k_tsdf_prep_touch_batch; hv_pack_px4_frames) at the shapes and batch sizes
where grouping can go wrong.  A pack thread writes the records of the same 4 pixels of HV_PACK_FRAMES consecutive frames; the last
group of a batch may be ragged, an image that is no whole number of pixel quads takes the per-frame fallback, the bitwise sweep
form's 8-byte records do too.

Every case fuses the same frames twice: one integrate() per frame (the online path: its own pack, no batch records) and
integrate_batch; the full dumps are held equal with conftest.assert_dumps_match (keys, weights and colours identical; tsdf bitwise
under the bitwise sweep form, within FOLD_TSDF_TOL under the fold form).  The uint16 cases are also held against oracle.PortTsdf.

Image sizes: 64x48 = 3 whole 1024-pixel pack blocks; 80x60 = 4800 pixels, the last block partly filled (its last wave holds 48
lanes: records stored straight from the registers, every other wave hands them through LDS); 37x23 = 851 pixels, no multiple of 4:
the fallback.  A tile leaves waves with some lanes out, too.
"""
import functools
import os
import re

import numpy as np
import pytest

import oracle
from tests.conftest import ROOT, assert_dumps_match
from tests.test_gpu_tsdf import assert_same_volume
from tests.test_gpu_tsdf_edges import cuda, frames_of, intrinsic, odd_config, stack, volume

pytestmark = pytest.mark.gpu

VOXEL, TRUNC = 0.02, 0.08
SHAPES = [(64, 48), (80, 60), (37, 23)]
with open(os.path.join(ROOT, "pyslam_amd", "csrc", "hv_tsdf_device.h")) as _f:
    FG = int(re.search(r"^static constexpr int HV_PACK_FRAMES = (\d+);", _f.read(), re.M).group(1))  # frames per pack thread
N_MAX = 64 + 2


def depth_kw(u16):
    """-> (frame generator arguments, depth_scale)"""
    return (dict(depth_dtype="uint16", depth_map_factor=1000.0), 1000.0) if u16 else (dict(), 1.0)


def frames(W, H, n, u16=False):
    kw, _ = depth_kw(u16)
    s, fr = frames_of(odd_config(W, H), 0, N_MAX, **kw)
    return s, fr[:n]


def prepared(v, bgr, tile):
    if bgr:
        v.set_color_order(True)
    if tile:
        v.set_tile(*tile)
    return v


@functools.lru_cache(maxsize=None)
def online_dump(W, H, n, u16=False, bgr=False, tile=None):
    """The dump of the first n frames fused one integrate() per frame: computed once per argument set, never written to."""
    from pyslam_amd.volumetric import RGBDImage

    s, fr = frames(W, H, n, u16)
    scale = depth_kw(u16)[1]
    v = prepared(volume(VOXEL, TRUNC), bgr, tile)
    for d, c, T in fr:
        v.integrate(RGBDImage(c, d, scale, 4.0), intrinsic(s), T)
    dump = v.dump()
    assert len(dump[0]) > 0
    for a in dump:
        a.setflags(write=False)
    return dump


def batch_volume(W, H, calls, u16=False, bgr=False, tile=None):
    """A volume that fused frames [lo, hi) of every (lo, hi) of `calls` with one integrate_batch call each."""
    s, fr = frames(W, H, max(hi for _, hi in calls), u16)
    d, c, T = stack(fr)
    dd, cd = cuda(d, c)
    v = prepared(volume(VOXEL, TRUNC), bgr, tile)
    for lo, hi in calls:
        v.integrate_batch(dd[lo:hi], cd[lo:hi], intrinsic(s), T[lo:hi], depth_scale=depth_kw(u16)[1], depth_trunc=4.0)
    return v


@pytest.mark.parametrize("B", sorted({FG - 1, FG, FG + 1, 7}))
@pytest.mark.parametrize("W,H", SHAPES)
def test_group_sizes_match_the_online_path(W, H, B, sweep_form):
    """One frame short of a group, a whole group, a group and a ragged one, a prime."""
    assert_dumps_match(batch_volume(W, H, [(0, B)]).dump(), online_dump(W, H, B))


@pytest.mark.parametrize("W,H", SHAPES)
def test_uint16_depth_matches_the_online_path_and_the_oracle(W, H, sweep_form):
    B = 2 * FG + 1
    gpu = batch_volume(W, H, [(0, B)], u16=True)
    assert_dumps_match(gpu.dump(), online_dump(W, H, B, u16=True))
    s, fr = frames(W, H, B, u16=True)
    cpu = oracle.PortTsdf(VOXEL, TRUNC, threads=8)
    for d, c, T in fr:
        cpu.integrate(d, c, intrinsic(s).as_array(), T, 1000.0, 4.0)
    assert_same_volume(gpu, cpu, swept=True)


def test_float_depth_matches_the_oracle(sweep_form):
    W, H, B = 80, 60, FG + 1
    s, fr = frames(W, H, B)
    cpu = oracle.PortTsdf(VOXEL, TRUNC, threads=8)
    for d, c, T in fr:
        cpu.integrate(d, c, intrinsic(s).as_array(), T, 1.0, 4.0)
    assert_same_volume(batch_volume(W, H, [(0, B)]), cpu, swept=True)


@pytest.mark.parametrize("u16", [False, True])
def test_two_chunks_in_one_call_the_second_ragged(u16, sweep_form):
    """64 + 2 frames: a chunk of whole groups, then a chunk that is one ragged group (packed beside the first chunk's sweep)."""
    assert_dumps_match(batch_volume(80, 60, [(0, N_MAX)], u16=u16).dump(), online_dump(80, 60, N_MAX, u16=u16))


@pytest.mark.parametrize("W,H", SHAPES)
def test_bgr_colour_order(W, H, sweep_form):
    B = FG + 1
    got = batch_volume(W, H, [(0, B)], bgr=True).dump()
    assert_dumps_match(got, online_dump(W, H, B, bgr=True))
    rgb = online_dump(W, H, B)
    np.testing.assert_array_equal(got[3][..., 0], rgb[3][..., 2])  # the order really was swapped
    assert not np.array_equal(got[3][..., 0], rgb[3][..., 0])


@pytest.mark.parametrize("W,H,tile", [(64, 48, (20, 12, 44, 40)), (80, 60, (0, 0, 40, 60)), (80, 60, (44, 31, 80, 60))])
def test_tile_set_the_pack_skips_rows_and_columns(W, H, tile, sweep_form):
    """Widths divisible by 4: the pack role leaves out the quads outside the tile (+ 4 pixels); an inner tile, a left half, a corner."""
    B = FG + 1
    got = batch_volume(W, H, [(0, B)], tile=tile).dump()
    assert_dumps_match(got, online_dump(W, H, B, tile=tile))
    assert got[2].sum() < online_dump(W, H, B)[2].sum()  # the tile really cut observations away


@pytest.mark.parametrize("W,H", SHAPES)
def test_two_consecutive_calls_the_second_pack_beside_a_sweep(W, H, sweep_form):
    """The second call's touch + pack launch runs on the second stream while the first call is swept, into the other scratch set."""
    n0, n1 = FG + 1, 7
    assert_dumps_match(batch_volume(W, H, [(0, n0), (n0, n0 + n1)]).dump(), online_dump(W, H, n0 + n1))
