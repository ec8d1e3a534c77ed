"""GPU: ScalableTSDFVolume.prune (include/hipvol.h, hv_tsdf_prune) held to the numpy restatement (tests/prune_reference.py) bit
for bit on the volume's own dump, and everything that ran before - fusion, de-integration, extraction, ray cast, tracking, growth,
reset, sharding - run again on the pruned volume.

The oracle never releases a unit, so wherever a pruned volume is held to oracle.PortTsdf both dumps first lose their all-zero units
(prune_reference(dump, True)); then the key sets must be equal and weights, colours and tsdf are compared as assert_oracle_match
does (weights and colour sums exact, tsdf within 1e-4).  No bar of its own: every comparison is bitwise or an existing test's.
"""
import numpy as np
import pytest

from tests import raycast_reference as rr
from tests import track_reference as tr
from tests.conftest import canonical_mesh
from tests.prune_reference import prune_reference
from tests.test_gpu_tsdf_deintegrate import assert_bitwise, assert_oracle_match
from tests.test_gpu_tsdf_edges import cuda, intrinsic, oracle_of, stack, tiny_frames, volume
from tests.test_gpu_tsdf_raycast import assert_agrees

pytestmark = pytest.mark.gpu

VOX, TRUNC = 0.02, 0.08
UNIT = VOX * 16


def rgbd(d, c):
    from pyslam_amd.volumetric import RGBDImage

    return RGBDImage.create_from_color_and_depth(c, d, 1.0, 4.0, False)


def fuse(vol, s, frames):
    d, c, T = stack(frames)
    vol.integrate_batch(*cuda(d, c), intrinsic(s), T)


def unfuse(vol, s, frames):
    d, c, T = stack(frames)
    return vol.deintegrate_batch(*cuda(d, c), intrinsic(s), T)


def fused(frames_from=0, count=48, **kw):
    s, frames = tiny_frames(frames_from, count)
    vol = volume(VOX, TRUNC, **kw)
    fuse(vol, s, frames)
    return s, frames, vol


class _Dumped:
    def __init__(self, dump):
        self._dump = dump

    def dump(self):
        return self._dump


def assert_oracle_match_pruned(gpu_dump, cpu, label):
    """The rule for a volume that has been pruned: both sides without their all-zero units, equal key sets, then assert_oracle_match."""
    g = prune_reference(gpu_dump, True)[0]
    o = prune_reference(cpu.dump(), True)[0]
    np.testing.assert_array_equal(g[0], o[0])
    assert_oracle_match(g, _Dumped(o), label)


def assert_consistent(vol, n):
    assert vol.num_blocks() == n
    keys = vol.unit_keys()
    dump_keys = vol.dump()[0]
    assert len(keys) == n == len(dump_keys)
    np.testing.assert_array_equal(keys[np.lexsort(keys.T[::-1])], dump_keys)


def sorted_cloud(pc):
    p, c = np.asarray(pc.points), np.asarray(pc.colors)
    o = np.lexsort(p.T[::-1])
    return p[o], c[o]


def assert_same_surfaces(a, b):
    ma, mb = a.extract_triangle_mesh(), b.extract_triangle_mesh()
    for x, y in zip(canonical_mesh(ma.vertices, ma.triangles, ma.vertex_colors), canonical_mesh(mb.vertices, mb.triangles, mb.vertex_colors)):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(sorted_cloud(a.extract_point_cloud()), sorted_cloud(b.extract_point_cloud())):
        np.testing.assert_array_equal(x, y)
    return len(ma.triangles)


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_lossless_on_a_fused_map():
    from pyslam_amd.volumetric import PruneStats

    s, frames, vol = fused()
    before = vol.dump()
    cap = vol.max_blocks()
    ref, stats = prune_reference(before, True)
    print("fused 0..47: reference stats", stats)
    assert stats[2] > 0 and stats[3] > 0  # (19 of 451 on the oracle: tests/test_prune_reference_cpu.py)
    st = vol.prune()
    assert isinstance(st, PruneStats) and st.as_tuple() == stats and st == PruneStats(*stats)
    assert_bitwise(vol.dump(), ref)
    assert_consistent(vol, stats[3])
    assert vol.max_blocks() == cap
    again = vol.prune()
    assert again.as_tuple() == (stats[3], 0, 0, stats[3])
    assert_bitwise(vol.dump(), ref)
    assert_consistent(vol, stats[3])
    assert vol.prune(empty=False).as_tuple() == (stats[3], 0, 0, stats[3])
    assert_oracle_match_pruned(vol.dump(), oracle_of(s, frames, VOX, TRUNC), "pruned map of 0..47")


# 2 ---------------------------------------------------------------------------------------------------------------------------
def deintegrated_and_pruned():
    s, frames, vol = fused()
    unfuse(vol, s, frames[24:])
    before = vol.dump()
    st = vol.prune()
    return s, frames, vol, before, st


def test_after_a_deintegration():
    s, frames, vol, before, st = deintegrated_and_pruned()
    ref, stats = prune_reference(before, True)
    print("fused 0..47, removed 24..47: reference stats", stats)
    assert stats[2] > 19  # the removal emptied units (85 of 451 on the oracle)
    assert st.as_tuple() == stats
    after = vol.dump()
    assert_bitwise(after, ref)
    assert_consistent(vol, stats[3])
    assert_oracle_match_pruned(after, oracle_of(s, frames[:24], VOX, TRUNC), "pruned map of 0..23")


# 3 ---------------------------------------------------------------------------------------------------------------------------
def _refused(online):
    s, frames = tiny_frames(0, 48)
    vol, twin = volume(VOX, TRUNC), volume(VOX, TRUNC)
    for v in (vol, twin):
        fuse(v, s, frames)
        unfuse(v, s, frames[24:])
    st = vol.prune()
    assert st.units_empty > 0
    for v in (vol, twin):
        if online:
            for d, c, T in frames[24:]:
                v.integrate(rgbd(d, c), intrinsic(s), T)
        else:
            fuse(v, s, frames[24:])
    a, b = prune_reference(vol.dump(), True)[0], prune_reference(twin.dump(), True)[0]
    assert_bitwise(a, b)
    assert vol.num_blocks() <= twin.num_blocks()
    assert_oracle_match_pruned(vol.dump(), oracle_of(s, frames, VOX, TRUNC), "pruned, fused again")


def test_released_slots_are_clean_and_reusable(sweep_form):
    _refused(online=False)


def test_released_slots_are_clean_and_reusable_online():
    _refused(online=True)


# 4 ---------------------------------------------------------------------------------------------------------------------------
def split_box(dump):
    """A box in metres from the dump's key range that cuts the map in two along x, and its unit range."""
    from pyslam_amd.volumetric import unit_range_of_bounds

    keys = dump[0]
    lo, hi = keys.min(0).astype(np.int64), keys.max(0).astype(np.int64)
    cut = int(np.median(keys[:, 0]))
    hi_cut = np.array([cut, hi[1], hi[2]])
    bounds = (lo * UNIT + 0.25 * UNIT, hi_cut * UNIT + 0.5 * UNIT)
    ulo, uhi = unit_range_of_bounds(bounds, VOX, 16)
    assert ulo.tolist() == lo.tolist() and uhi.tolist() == hi_cut.tolist()
    return bounds, ulo, uhi


@pytest.mark.parametrize("empty", [False, True])
def test_bounds_match_the_restatement(empty):
    s, frames, vol = fused()
    before = vol.dump()
    bounds, ulo, uhi = split_box(before)
    ref, stats = prune_reference(before, empty, ulo, uhi)
    observed = before[2].max(axis=1) > 0
    outside = np.any((before[0] < ulo) | (before[0] > uhi), axis=1)
    print("bounds", bounds, "reference stats", stats)
    assert (observed & outside).sum() > 0 and (observed & ~outside).sum() > 0  # the box releases AND keeps units with weight
    assert stats[1] > 0 and stats[3] > 0 and (stats[2] > 0) == empty
    st = vol.prune(empty=empty, bounds=bounds)
    assert st.as_tuple() == stats
    assert_bitwise(vol.dump(), ref)
    assert_consistent(vol, stats[3])


def test_bounds_that_hold_everything_and_nothing():
    s, frames, vol = fused()
    before = vol.dump()
    n = len(before[0])
    lo, hi = before[0].min(0) * UNIT, (before[0].max(0) + 1) * UNIT
    assert vol.prune(empty=False, bounds=(lo - 1.0, hi + 1.0)).as_tuple() == (n, 0, 0, n)
    assert_bitwise(vol.dump(), before)
    far = (hi + 10.0, hi + 11.0)
    assert vol.prune(empty=False, bounds=far).as_tuple() == (n, n, 0, 0)
    assert vol.num_blocks() == 0 and len(vol.dump()[0]) == 0 and len(vol.unit_keys()) == 0
    fuse(vol, s, frames[30:40])
    assert_oracle_match(vol.dump(), oracle_of(s, frames[30:40], VOX, TRUNC), "fused after everything was released")
    assert vol.num_blocks() == oracle_of(s, frames[30:40], VOX, TRUNC).num_units()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_everything_released():
    s, frames, vol = fused(0, 10)
    n = vol.num_blocks()
    unfuse(vol, s, frames)
    st = vol.prune()
    assert st.as_tuple() == (n, 0, n, 0)
    assert vol.num_blocks() == 0 and len(vol.dump()[0]) == 0
    assert vol.extract_triangle_mesh().triangles.shape[0] == 0
    assert len(vol.extract_point_cloud().points) == 0
    assert not vol.ray_cast(intrinsic(s), frames[3][2], render_attributes=("mask",))["mask"].any()
    fuse(vol, s, frames)
    cpu = oracle_of(s, frames, VOX, TRUNC)
    assert vol.num_blocks() == cpu.num_units()
    assert_oracle_match(vol.dump(), cpu, "fused again after everything was released")


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_extraction_follows_a_prune(monkeypatch):
    s, frames = tiny_frames(0, 49)
    vol, twin = volume(VOX, TRUNC), volume(VOX, TRUNC)
    for v in (vol, twin):
        fuse(v, s, frames[:48])
        v.extract_triangle_mesh()  # arms the incremental caches
        v.extract_point_cloud()
        unfuse(v, s, frames[24:48])
    assert vol.prune().units_empty > 0
    assert assert_same_surfaces(vol, twin) > 0
    d, c, T = frames[48]
    for v in (vol, twin):
        v.integrate(rgbd(d, c), intrinsic(s), T)
    assert assert_same_surfaces(vol, twin) > 0
    inc = vol.extract_triangle_mesh(), sorted_cloud(vol.extract_point_cloud())
    monkeypatch.setenv("HV_EXTRACT_INCREMENTAL", "0")
    full = vol.extract_triangle_mesh(), sorted_cloud(vol.extract_point_cloud())
    for x, y in zip(canonical_mesh(inc[0].vertices, inc[0].triangles, inc[0].vertex_colors),
                    canonical_mesh(full[0].vertices, full[0].triangles, full[0].vertex_colors)):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(inc[1], full[1]):
        np.testing.assert_array_equal(x, y)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_ray_cast_and_tracking_on_a_pruned_map():
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    s, frames, vol, _, st = deintegrated_and_pruned()
    assert st.units_empty > 0
    K = intrinsic(s)
    dump = vol.dump()
    for i in (2, 11, 20):
        T = frames[i][2]
        gpu = vol.ray_cast(K, T, 0.1, 4.0)
        ref = rr.ray_cast(dump, VOX, TRUNC, s.intrinsics, T, s.height, s.width, 0.1, 4.0)
        assert gpu["mask"].mean() > 0.3, (i, float(gpu["mask"].mean()))
        assert_agrees(gpu, ref, f"pose {i} after prune")

    i = 12
    depth, _, T_true = frames[i]
    xi = np.concatenate([np.radians(1.0) * np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0), 0.02 * np.array([0.0, 1.0, -1.0]) / np.sqrt(2.0)])
    T0 = np.linalg.inv(np.linalg.inv(T_true) @ tr.exp_twist(xi))
    iterations = (10, 5, 4)
    out = vol.track_frame_to_model(depth, K, T0, depth_max=4.0, iterations=iterations, trace=True)

    def model(level, Kl, h, w):
        Kp = PinholeCameraIntrinsic(w, h, *Kl)
        m = vol.ray_cast(Kp, T0, 0.1, 4.0, 3.0, render_attributes=("depth", "normal", "mask"))
        # the level's model is the public cast, and that agrees with the numpy cast of the post-prune dump
        ref = rr.ray_cast(dump, VOX, TRUNC, Kl, T0, h, w, 0.1, 4.0, 3.0)
        full = vol.ray_cast(Kp, T0, 0.1, 4.0, 3.0)
        assert_agrees(full, ref, f"track model level {level}")
        return m["depth"], m["normal"], m["mask"]

    rep = tr.check_call(out, depth, s.intrinsics, T0, model, iterations, depth_max=4.0)
    err = tr.pose_error(out.transformation, T_true)
    print("tracking on the pruned map: rows %d, max xi rel %.3g, success %s, fitness %.3f, pose error %.3g m %.3g deg"
          % (rep["rows"], rep["xi_rel"], out.success, out.fitness, err[0], err[1]))
    assert out.success


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_stamps_follow_their_units():
    s, frames = tiny_frames(0, 48)
    vol = volume(VOX, TRUNC)
    fuse(vol, s, frames[:16])
    vol.mark_merged()
    fuse(vol, s, frames[16:])
    unfuse(vol, s, frames[24:])
    dirty = {tuple(k) for k in vol.dirty_keys()}
    held = {tuple(k) for k in vol.dump()[0]}
    assert 0 < len(dirty) < len(held)
    st = vol.prune()
    kept = {tuple(k) for k in vol.dump()[0]}
    released = held - kept
    assert len(released) == st.units_empty > 0 and released & dirty and (held - dirty) & kept
    after = vol.dirty_keys()
    assert {tuple(k) for k in after} == dirty - released and len(after) == len(dirty - released)
    assert len(vol.touched_keys()) == 0
    d, c, T = frames[5]
    vol.integrate(rgbd(d, c), intrinsic(s), T)
    cpu = oracle_of(s, [frames[5]], VOX, TRUNC)
    np.testing.assert_array_equal(vol.touched_keys(), cpu.touched_keys())


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_growth_and_reset_after_a_prune():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    s, frames = tiny_frames(0, 160)
    vol = ScalableTSDFVolume(VOX, TRUNC, max_blocks=512)
    assert vol.prune().as_tuple() == (0, 0, 0, 0)  # an empty volume
    fuse(vol, s, frames[:16])
    unfuse(vol, s, frames[8:16])
    cap = vol.max_blocks()
    st = vol.prune()
    assert st.units_empty > 0 and vol.max_blocks() == cap
    for lo in range(16, 160, 8):  # the camera moves on: the pool has to grow (reserve_blocks / auto-growth inside the calls)
        fuse(vol, s, frames[lo:lo + 8])
    assert vol.max_blocks() > cap and vol.dropped_points() == 0
    keep = frames[:8] + frames[16:]
    assert_oracle_match_pruned(vol.dump(), oracle_of(s, keep, VOX, TRUNC), "pruned small pool, grown")
    vol.reserve_blocks(vol.max_blocks() * 2)
    n = vol.num_blocks()
    st = vol.prune()
    assert st.units_before == n and st.units_after == vol.num_blocks()
    assert_oracle_match_pruned(vol.dump(), oracle_of(s, keep, VOX, TRUNC), "reserved, pruned again")
    vol.reset()
    assert vol.num_blocks() == 0
    assert vol.prune().as_tuple() == (0, 0, 0, 0)  # a freshly reset volume
    fuse(vol, s, frames[40:48])
    cpu = oracle_of(s, frames[40:48], VOX, TRUNC)
    assert vol.num_blocks() == cpu.num_units()
    assert_oracle_match(vol.dump(), cpu, "fused after prune and reset")


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_owner_sharded_ranks_prune_their_own_units():
    s, frames = tiny_frames(0, 48)
    single = volume(VOX, TRUNC)
    ranks = [volume(VOX, TRUNC) for _ in range(2)]
    for r, v in enumerate(ranks):
        v.set_owner(r, 2)
    for v in [single] + ranks:
        fuse(v, s, frames)
        unfuse(v, s, frames[24:])
    bounds, _, _ = split_box(single.dump())
    for kw in (dict(), dict(bounds=bounds)):
        st = [v.prune(**kw) for v in [single] + ranks]
        assert st[0].units_after < st[0].units_before
        assert tuple(a + b for a, b in zip(st[1].as_tuple(), st[2].as_tuple())) == st[0].as_tuple()
        dumps = [v.dump() for v in ranks]
        union = [np.concatenate([dp[k] for dp in dumps]) for k in range(4)]
        order = np.lexsort(union[0].T[::-1])
        assert_bitwise(tuple(u[order] for u in union), single.dump())


def test_errors():
    from pyslam_amd._lib import HipVolError
    from pyslam_amd.volumetric import VoxelBlockGrid

    s, frames, vol = fused(0, 4)
    before = vol.dump()
    tiled = volume(VOX, TRUNC)
    tiled.set_tile(0, 0, s.width // 2, s.height)
    with pytest.raises(HipVolError, match="tile"):
        tiled.prune()
    grid = VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12)
    assert not hasattr(grid, "prune")
    with pytest.raises(HipVolError, match="TSDF"):
        type(vol).prune(grid)
    # the C ABI: one of unit_lo / unit_hi alone and an empty range are refused; stats may be NULL
    import ctypes

    from pyslam_amd import _lib as L

    lo, hi = (ctypes.c_int32 * 3)(0, 0, 0), (ctypes.c_int32 * 3)(5, -1, 5)
    with pytest.raises(HipVolError, match="go together"):
        L.check(vol._lib.hv_tsdf_prune(vol._h, 1, lo, None, None))
    with pytest.raises(HipVolError, match="empty unit range"):
        L.check(vol._lib.hv_tsdf_prune(vol._h, 1, lo, hi, None))
    assert_bitwise(vol.dump(), before)
    other = fused(0, 4)[2]
    L.check(other._lib.hv_tsdf_prune(other._h, 1, None, None, None))
    assert_bitwise(other.dump(), prune_reference(before, True)[0])
    # bad bounds are refused before the library
    for bad in (((0.0, 0.0, 1.0), (1.0, 1.0, 0.0)), ((0.0, 0.0, 0.0), (1.0, np.nan, 1.0)), ((0.0, 0.0, 0.0), (np.inf, 1.0, 1.0)),
                ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0e9)), ((0.0, 0.0), (1.0, 1.0))):
        with pytest.raises(ValueError):
            vol.prune(bounds=bad)
    assert_bitwise(vol.dump(), before)
