"""GPU: ScalableTSDFVolume.integrate_volume (include/hipvol.h, hv_tsdf_integrate_volume) held to the numpy restatement
(tests/merge_reference.py) on the volumes' own dumps, and everything downstream of a map - extraction, ray cast, tracking, prune,
growth - run on the merged volume.

Against the restatement the aim is bit-for-bit equality of the dumps (both sides follow the contract's float64 operation order).
A voxel is FRAGILE when some component of r lies within 1e-9 of 0, 0.5 or 1.  The generic transform excludes its fragile voxels from
the value comparison (their share is bounded, their weights must be the restatement's or a neighbouring source voxel's).  The identity
and the whole-voxel shift put every voxel on r = 0 / 1 by construction and are held to the shifted source instead (weights and colour
sums exact, tsdf within 2^-23: tests/test_merge_reference_cpu.py).  The half-voxel shift puts every voxel on r = 0.5 by construction,
so a share bound cannot apply to it: it is held to the restatement on EVERY voxel, fragile or not.

The overlap case's bars are the fused-field bars of tests/test_raycast_reference_cpu.py; measured on the CPU restatement at
640 x 480 (tests/test_merge_reference_cpu.py: joined maps against all three frames fused directly, poses 0, 1, 2, NOVEL):
    joined  hits 99.92 / 99.95 / 99.95 / 99.99 %, |dz| median 0.020 / 0.014 / 0.012 / 0.016 voxel, p99 0.55 / 0.51 / 0.64 / 0.55 voxel
    direct  hits 99.92 / 99.95 / 99.97 / 99.99 %, |dz| median 0.020 / 0.014 / 0.013 / 0.016 voxel, p99 0.49 / 0.49 / 0.62 / 0.53 voxel
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import merge_reference as mr
from tests import raycast_reference as rr
from tests import track_reference as tr
from tests import tsdf_closed_form as cf
from tests.conftest import canonical_mesh
from tests.test_gpu_tsdf_deintegrate import assert_bitwise
from tests.test_gpu_tsdf_edges import assert_meshes_match, cuda, intrinsic, stack, tiny_frames, volume
from tests.test_gpu_tsdf_raycast import assert_agrees
from tests.test_merge_reference_cpu import (CAST_POSES, GENERIC, OTHER, SHIFT, assert_is_shifted_source, check_closed_form_scores,
                                            rigid_inverse, scores_in_frame, translation)

pytestmark = pytest.mark.gpu

VOX, TRUNC = 0.02, 0.08
TRANSFORMS = {"identity": np.eye(4), "shift": translation(SHIFT, VOX), "half": translation((0.5, 0.5, 0.5), VOX), "generic": GENERIC}
ON_A_BOUNDARY = ("identity", "shift", "half")  # every voxel is fragile by construction


def fuse(vol, s, frames, frame_of_map=None):
    """frame_of_map = F: the map is held in the frame p_map = F p_world (poses T_cw F^-1)."""
    d, c, T = stack(frames)
    if frame_of_map is not None:
        T = T @ rigid_inverse(frame_of_map)
    vol.integrate_batch(*cuda(d, c), intrinsic(s), np.ascontiguousarray(T))


def source_for(T, frames_from=0, count=24, **kw):
    """A map of tiny frames held in the frame from which `T` carries it back into the world frame."""
    s, frames = tiny_frames(frames_from, count)
    src = volume(VOX, TRUNC, **kw)
    fuse(src, s, frames, frame_of_map=rigid_inverse(T))
    return s, frames, src


def sums_of(dump):
    return np.rint(np.asarray(dump[3], np.float64) * np.asarray(dump[2], np.float64)[..., None])


def neighbour_weights(src_dump, T, keys, rows, words):
    """weights of the source voxels g0 + {-1..2}^3 around the listed destination voxels -> [n, 64]"""
    grid = rr._Grid(src_dump)
    local = np.stack([words // 256, (words // 16) % 16, words % 16], axis=-1)
    g0, _, _ = mr.locate(T, np.asarray(keys, np.int64)[rows] * 16 + local, VOX)
    out = []
    for dx in range(-1, 3):
        for dy in range(-1, 3):
            for dz in range(-1, 3):
                row, word = grid.locate(g0[0] + dx, g0[1] + dy, g0[2] + dz)
                out.append(np.where(row >= 0, grid.weight[np.maximum(row, 0), word], 0))
    return np.stack(out, axis=-1)


def assert_matches_restatement(gpu, before, src_dump, T, name, on_a_boundary=None):
    """-> (True when the dumps are equal bit for bit, the restatement's stats).  on_a_boundary: every voxel is fragile by
    construction, so every voxel is compared and no share bound applies (default: `name` is one of ON_A_BOUNDARY)."""
    if on_a_boundary is None:
        on_a_boundary = name in ON_A_BOUNDARY
    ref, stats, detail = mr.merge_reference(before, src_dump, T, VOX, detail=True)
    np.testing.assert_array_equal(gpu[0], ref[0], err_msg=f"{name}: unit set")
    fragile = np.zeros(np.asarray(ref[2]).shape, bool)
    index = {tuple(k): i for i, k in enumerate(np.asarray(ref[0]).tolist())}
    for j, k in enumerate(detail["keys"].tolist()):
        if tuple(k) in index:
            fragile[index[tuple(k)]] = detail["fragile"][j]
    share = float(fragile.mean())
    exclude = fragile if not on_a_boundary else np.zeros_like(fragile)
    if not on_a_boundary:
        assert share <= 1e-4, (name, "fragile share", share)
        rows, words = np.nonzero(fragile)
        if len(rows):
            bidx = {tuple(k): i for i, k in enumerate(np.asarray(before[0]).tolist())}
            w0 = np.array([before[2][bidx[tuple(ref[0][r])], w] if tuple(ref[0][r]) in bidx else 0.0 for r, w in zip(rows, words)])
            got = gpu[2][rows, words] - w0
            allowed = neighbour_weights(src_dump, T, ref[0], rows, words)
            assert ((got[:, None] == allowed).any(axis=1) | (got == 0)).all(), (name, "a fragile voxel's weight is nobody's")
    ok = ~exclude
    assert np.array_equal(gpu[2][ok], ref[2][ok]), (name, "update decision / weight", int((gpu[2] != ref[2])[ok].sum()))
    d_sum = np.abs(sums_of(gpu) - sums_of(ref))[ok]
    d_tsdf = np.abs(gpu[1].astype(np.float64) - ref[1].astype(np.float64))[ok]
    bitwise = all(np.array_equal(a.view(np.uint8) if a.dtype == np.float32 else a, b.view(np.uint8) if b.dtype == np.float32 else b)
                  for a, b in zip(gpu, ref))
    print(f"{name}: {len(ref[0])} units, stats {stats}, fragile share {share:.3g}, max colour-sum diff {d_sum.max():.0f}, "
          f"max tsdf diff {d_tsdf.max():.3g}, bitwise {bitwise}")
    assert d_sum.max() <= 1 and d_tsdf.max() <= 2.0 ** -23, (name, float(d_sum.max()), float(d_tsdf.max()))
    return bitwise, stats


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filled", [False, True], ids=["empty", "filled"])
@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_matches_the_restatement(name, filled):
    from pyslam_amd.volumetric import MergeStats

    T = TRANSFORMS[name]
    s, frames, src = source_for(T)
    dst = volume(VOX, TRUNC)
    if filled:
        fuse(dst, *tiny_frames(16, 24))
    before, src_dump = dst.dump(), src.dump()
    st = dst.integrate_volume(src, T)
    after = dst.dump()
    bitwise, stats = assert_matches_restatement(after, before, src_dump, T, name)
    assert isinstance(st, MergeStats) and st.as_tuple() == stats
    assert st.voxels_updated == st.voxels_trilinear + st.voxels_nearest > 0 and st.units_claimed == len(after[0]) - len(before[0])
    assert bitwise, name  # reached on the MI355X: the kernel follows the contract's operation order
    if not filled and name in ("identity", "shift"):
        shift = np.rint(T[:3, 3] / VOX).astype(np.int64)
        assert_is_shifted_source(after, src_dump, shift, name)


# 2 ---------------------------------------------------------------------------------------------------------------------------
def assert_consistent(vol):
    n = vol.num_blocks()
    keys, dump_keys = vol.unit_keys(), vol.dump()[0]
    assert len(keys) == n == len(dump_keys)
    np.testing.assert_array_equal(keys[np.lexsort(keys.T[::-1])], dump_keys)
    return n


@pytest.mark.parametrize("filled", [False, True], ids=["empty", "filled"])
def test_state_after_the_call(filled):
    s, frames, src = source_for(GENERIC)
    src_before = src.dump()
    twins = [volume(VOX, TRUNC), volume(VOX, TRUNC)]
    for v in twins:
        if filled:
            fuse(v, *tiny_frames(16, 24))
    d0 = twins[0].dump()
    empty_before = {tuple(k) for k in d0[0][d0[2].max(axis=1) == 0].tolist()} if filled else set()
    stats = [v.integrate_volume(src, GENERIC) for v in twins]
    assert_bitwise(src.dump(), src_before)
    assert stats[0] == stats[1]
    assert_bitwise(twins[0].dump(), twins[1].dump())
    n = assert_consistent(twins[0])
    assert stats[0].units_source == int((src_before[2].max(axis=1) > 0).sum())
    d1 = twins[0].dump()
    empty_after = {tuple(k) for k in d1[0][d1[2].max(axis=1) == 0].tolist()}
    assert empty_after <= empty_before  # nothing the merge claimed is empty: only units that were empty before and took no voxel
    pruned = twins[0].prune()
    assert pruned.units_empty == len(empty_after) and pruned.units_after == n - len(empty_after)
    # a second merge of the same source doubles its share: the units are there already
    again = twins[1].integrate_volume(src, GENERIC)
    assert again.units_claimed == 0 and again.voxels_updated == stats[0].voxels_updated
    assert twins[1].num_blocks() == n


# 3 ---------------------------------------------------------------------------------------------------------------------------
def mesh_of(vol):
    m = vol.extract_triangle_mesh()
    return canonical_mesh(m.vertices, m.triangles, m.vertex_colors)


def test_downstream_extraction_and_ray_cast(monkeypatch):
    import oracle

    s, frames, src = source_for(GENERIC)
    dst = volume(VOX, TRUNC)
    fuse(dst, *tiny_frames(16, 24))
    before_mesh = mesh_of(dst)  # arms the incremental caches
    dst.extract_point_cloud()
    dst.mark_merged()
    st = dst.integrate_volume(src, GENERIC)
    dump = dst.dump()
    dirty = {tuple(k) for k in dst.dirty_keys().tolist()}
    assert 0 < len(dirty) <= len(dump[0]) and st.units_claimed <= len(dirty)
    after_mesh = mesh_of(dst)
    assert after_mesh[0].shape != before_mesh[0].shape or not np.array_equal(after_mesh[0], before_mesh[0])
    cloud = dst.extract_point_cloud()
    monkeypatch.setenv("HV_EXTRACT_INCREMENTAL", "0")
    for x, y in zip(after_mesh, mesh_of(dst)):
        np.testing.assert_array_equal(x, y)
    full_cloud = dst.extract_point_cloud()
    o1, o2 = np.lexsort(np.asarray(cloud.points).T[::-1]), np.lexsort(np.asarray(full_cloud.points).T[::-1])
    np.testing.assert_array_equal(np.asarray(cloud.points)[o1], np.asarray(full_cloud.points)[o2])
    np.testing.assert_array_equal(np.asarray(cloud.colors)[o1], np.asarray(full_cloud.colors)[o2])
    monkeypatch.delenv("HV_EXTRACT_INCREMENTAL")
    cpu = oracle.PortTsdf(VOX, TRUNC)
    cpu.load_units(dump[0], dump[1].reshape(-1, 16, 16, 16), dump[2].reshape(-1, 16, 16, 16), dump[3].reshape(-1, 16, 16, 16, 3))
    assert assert_meshes_match(dst, cpu) > 0
    K = intrinsic(s)
    for i in (2, 11, 30):
        T = tiny_frames(0, 48)[1][i][2]
        gpu = dst.ray_cast(K, T, 0.1, 4.0)
        ref = rr.ray_cast(dump, VOX, TRUNC, s.intrinsics, T, s.height, s.width, 0.1, 4.0)
        assert gpu["mask"].mean() > 0.3, (i, float(gpu["mask"].mean()))
        assert_agrees(gpu, ref, f"pose {i} on the merged map")


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_tracking_against_a_moved_map():
    """A bench-shaped map moved to another frame by one merge into an empty volume: a source frame tracks against it at the carried
    pose T_cw T^-1 inside the bound tests/test_gpu_tsdf_track.py holds the original map to (2e-3 m, 0.1 deg)."""
    from pyslam_amd.synthetic import SyntheticRGBD
    from pyslam_amd.volumetric import PinholeCameraIntrinsic, ScalableTSDFVolume

    s = SyntheticRGBD("synthetic_640x480_5mm")
    depth, rgb, T = s.batch(0, 64)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    src = ScalableTSDFVolume(0.005, 0.04, max_blocks=1 << 15)
    src.integrate_batch(torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda(), K, T, depth_scale=1.0, depth_trunc=4.0)
    moved = ScalableTSDFVolume(0.005, 0.04, max_blocks=1 << 10)  # grows
    st = moved.integrate_volume(src, GENERIC)
    print("bench map moved:", st, "units", moved.num_blocks(), "of", src.num_blocks(), "max_blocks", moved.max_blocks())
    assert moved.max_blocks() > 1 << 10 and st.units_claimed == moved.num_blocks()
    back = rigid_inverse(GENERIC)
    errs = []
    for i in (12, 40):
        T_true = T[i] @ back
        xi = np.concatenate([np.radians(1.0) * np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0), 0.02 * np.array([0.0, 1.0, -1.0]) / np.sqrt(2.0)])
        T0 = np.linalg.inv(np.linalg.inv(T_true) @ tr.exp_twist(xi))
        out = moved.track_frame_to_model(depth[i], K, T0)
        errs.append(tr.pose_error(out.transformation, T_true))
        assert out.success and out.fitness > 0.5, (i, out)
    errs = np.array(errs)
    print("tracking against the moved map: max %.3g m, %.3g deg" % tuple(errs.max(0)))
    assert (errs[:, 0] <= 2e-3).all() and (errs[:, 1] <= 0.1).all(), errs.max(0)


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_destination_with_overlap_on_the_closed_form_scene():
    from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume

    K = PinholeCameraIntrinsic(cf.W, cf.H, *cf.K)
    frames = cf.frames()
    direct, dst, src = (ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 14) for _ in range(3))
    for i, (depth, rgb, T) in enumerate(frames):
        img = RGBDImage(rgb, depth, 1.0, cf.DEPTH_TRUNC)
        direct.integrate(img, K, T)
        if i < 2:
            dst.integrate(img, K, T)
        else:
            src.integrate(img, K, T @ rigid_inverse(OTHER))  # held in the frame p = OTHER p_scene
    st = dst.integrate_volume(src, rigid_inverse(OTHER))
    dump, direct_dump = dst.dump(), direct.dump()
    print("joined on the GPU:", st)
    for n, T in enumerate(CAST_POSES):
        a = scores_in_frame(dst.ray_cast(K, T, 0.1, 3.0, weight_threshold=0.5), T, dump, np.eye(4))
        b = scores_in_frame(direct.ray_cast(K, T, 0.1, 3.0, weight_threshold=0.5), T, direct_dump, np.eye(4))
        print("pose %d joined %.2f%% %.3f/%.2f  direct %.2f%% %.3f/%.2f  hits %d / %d" %
              (n, 100 * a["hit_frac"], a["dz_median"], a["dz_p99"], 100 * b["hit_frac"], b["dz_median"], b["dz_p99"], a["hits"], b["hits"]))
        check_closed_form_scores(a)
        assert abs(a["hits"] - b["hits"]) <= 1e-3 * b["hits"], (a["hits"], b["hits"])


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_pool_growth_and_stats():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    s, frames, src = source_for(GENERIC, 0, 48)
    dst = ScalableTSDFVolume(VOX, TRUNC, max_blocks=64)
    before, n0, cap = dst.dump(), dst.num_blocks(), dst.max_blocks()
    assert n0 == 0 and cap == 64
    st = dst.integrate_volume(src, GENERIC)
    assert dst.max_blocks() > cap and dst.dropped_points() == 0
    assert st.voxels_updated == st.voxels_trilinear + st.voxels_nearest > 0
    assert st.units_claimed == dst.num_blocks() - n0 > cap
    assert_matches_restatement(dst.dump(), before, src.dump(), GENERIC, "generic")
    assert_consistent(dst)
    # the grown volume goes on fusing
    fuse(dst, *tiny_frames(62, 2))
    assert_consistent(dst)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_errors():
    from pyslam_amd import _lib as L
    from pyslam_amd._lib import HipVolError
    from pyslam_amd.volumetric import ScalableTSDFVolume, VoxelBlockGrid

    s, frames, src = source_for(np.eye(4), 0, 4)
    dst = volume(VOX, TRUNC)
    fuse(dst, *tiny_frames(2, 4))
    before, src_before = dst.dump(), src.dump()

    def refused(match, d, s_, T=np.eye(4)):
        with pytest.raises(HipVolError, match=match):
            d.integrate_volume(s_, T)

    grid = VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12)
    assert not hasattr(grid, "integrate_volume")
    refused("TSDF", dst, grid)
    with pytest.raises(HipVolError, match="TSDF"):
        type(dst).integrate_volume(grid, src)
    tiled = volume(VOX, TRUNC)
    tiled.set_tile(0, 0, s.width // 2, s.height)
    refused("tile", dst, tiled)
    refused("tile", tiled, src)
    owned = volume(VOX, TRUNC)
    owned.set_owner(0, 2)
    refused("owner", dst, owned)
    refused("owner", owned, src)
    refused("same volume", dst, dst)
    refused("voxel_length", dst, volume(0.01, TRUNC))
    refused("voxel_length", dst, volume(VOX, 0.06))
    bad = np.eye(4)
    bad[1, 3] = np.nan
    refused("not finite", dst, src, bad)
    bad = np.eye(4)
    bad[0, 1] = np.inf
    refused("not finite", dst, src, bad)
    refused("not rigid", dst, src, np.diag([1.0, 1.0, 1.001, 1.0]))
    refused("not rigid", dst, src, np.diag([1.0, 1.0, -1.0, 1.0]))
    bad = np.eye(4)
    bad[3, 2] = 1e-3
    refused("bottom row", dst, src, bad)
    bad = np.eye(4)
    bad[3, 3] = 2.0
    refused("bottom row", dst, src, bad)
    with pytest.raises(ValueError):
        dst.integrate_volume(src, np.eye(3))
    with pytest.raises(TypeError):
        dst.integrate_volume(None)
    with pytest.raises(HipVolError, match="null"):
        L.check(dst._lib.hv_tsdf_integrate_volume(dst._h, src._h, None, None))
    assert_bitwise(dst.dump(), before)
    assert_bitwise(src.dump(), src_before)
    # a rotation that is rigid to 1e-6 passes, and stats may be NULL
    T = np.ascontiguousarray(GENERIC)
    L.check(dst._lib.hv_tsdf_integrate_volume(dst._h, src._h, L.ptr(T), None))
    assert_bitwise(dst.dump(), mr.merge_reference(before, src_before, T, VOX)[0])


# 8 ---------------------------------------------------------------------------------------------------------------------------
def merges_that_leave_untouched(dst, merges):
    """`dst`, a filled volume, through `merges` (callables -> MergeStats) that update no voxel: the mesh cached before them is
    still served without an extraction kernel (launches == 0), the dump is bitwise the same and no unit is dirty.  -> their stats."""
    from pyslam_amd import _lib as L

    dst.mark_merged()
    before = dst.dump()
    mesh = dst.extract_triangle_mesh()
    # the C ABI's two steps: the size query does the device work and caches the result ...
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    L.check(dst._lib.hv_tsdf_extract_mesh(dst._h, None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt)))
    dst.profile_enable(True)
    dst.profile_read()
    stats = [merge() for merge in merges]
    # ... and the fetch after the merges is served from it: no extraction kernel runs (the profile brackets those; the merge's own
    # candidate pass, which does run for a source that holds units, is not bracketed)
    verts, cols, tris = np.zeros((nv.value, 3)), np.zeros((nv.value, 3)), np.zeros((nt.value, 3), np.int32)
    L.check(dst._lib.hv_tsdf_extract_mesh(dst._h, L.ptr(verts), L.ptr(cols), nv.value, L.ptr(tris), nt.value, ctypes.byref(nv), ctypes.byref(nt)))
    launches = dst.profile_read()[1]
    dst.profile_enable(False)
    assert launches == 0, launches
    np.testing.assert_array_equal(verts, mesh.vertices)
    np.testing.assert_array_equal(tris, mesh.triangles)
    assert_bitwise(dst.dump(), before)
    assert len(dst.dirty_keys()) == 0
    return stats


def test_empty_source_leaves_the_destination_untouched():
    s, frames = tiny_frames(0, 8)
    dst = volume(VOX, TRUNC)
    fuse(dst, s, frames)
    never = volume(VOX, TRUNC)  # never fused
    hollow = volume(VOX, TRUNC)  # units, but no observed voxel: fused and de-integrated
    d, c, T = stack(frames[:2])
    hollow.integrate_batch(*cuda(d, c), intrinsic(s), T)
    hollow.deintegrate_batch(*cuda(d, c), intrinsic(s), T)
    assert hollow.num_blocks() > 0
    for st in merges_that_leave_untouched(dst, [lambda src=src: dst.integrate_volume(src, GENERIC) for src in (never, hollow)]):
        assert st.as_tuple() == (0, 0, 0, 0, 0)
    # the other way round: a map merged into a never-used volume
    st = never.integrate_volume(dst, np.eye(4))
    assert st.units_claimed == never.num_blocks() > 0
