"""GPU: TSDF de-integration and re-integration (hv_deintegrate.hip) on planted voxel states (tests/planted_states.py) and under the
volume's rectify maps and colour order - the branches a map fused from the frames that are then removed never reaches.

Planted states: all three branches of the update rule (w0 < n, w0 == n, w0 > n) inside single 16-byte quads, weights between a
voxel's count in the first 64-frame chunk and its count over the whole call, colour sums the removed frames never contributed to,
units of the touch sets that are absent.  Every case is held bit for bit to the numpy restatement (tests/deintegrate_reference.py)
run on the planted volume's OWN dump, stats included, and re-asserts the class counts of tests/test_planted_states_cpu.py from what
the restatement saw, so that no case passes without reaching its branch.

Prep: frames handed to deintegrate* / reintegrate_batch go through set_rectify_maps and set_color_order(bgr=True) exactly as integrate
took them; the oracle is fed frames remapped on the host (oracle/host_prep.py) with the channels swapped, by the rules of
tests/test_gpu_tsdf_deintegrate.py::assert_oracle_match.  No tolerance of its own.

Measured on the MI355X when the file was written: every planted case equals the restatement bit for bit, stats included.  Before
the colour sums were clamped (include/hipvol.h, `update`) the foreign-colour case left dump() colours in [0, 4.29497e9]: the
uint32 sums wrapped.  With the kernel changed on a scratch copy: `w0 == n` treated like `w0 > n` fails every case of sections 1-7
and of the prep section; 32-frame chunks in the host loop fail the 64-frame batch and the 70-frame case; hv_tsdf_reintegrate_batch
leaving the maps on for its integrate half fails the 70-frame re-integration and the maps-survive case.  Nothing here takes
longer than 3 s.
"""
import ctypes

import numpy as np
import pytest

import oracle
from oracle import host_prep as hp
from tests import planted_states as ps
from tests.conftest import canonical_mesh
from tests.deintegrate_reference import deintegrate_reference
from tests.test_gpu_tsdf_deintegrate import assert_bitwise, assert_oracle_match, rgbd
from tests.test_gpu_tsdf_edges import cuda, frames_of, intrinsic, odd_config, stack, volume

pytestmark = pytest.mark.gpu

VOX, TRUNC = ps.VOX, ps.TRUNC


def planted(states, stride=4, max_blocks=None):
    """A volume holding the states; its dump is what tests/planted_states.as_dump says, bit for bit."""
    from pyslam_amd.volumetric import ScalableTSDFVolume

    vol = (volume(VOX, TRUNC, depth_sampling_stride=stride) if max_blocks is None else
           ScalableTSDFVolume(VOX, TRUNC, depth_sampling_stride=stride, max_blocks=max_blocks))
    ps.plant(vol, states)
    assert_bitwise(vol.dump(), ps.as_dump(states))
    return vol


def remove(vol, s, frames, scale):
    """One frame through deintegrate (host arrays), several through deintegrate_batch (device tensors)."""
    K = intrinsic(s)
    if len(frames) == 1:
        d, c, T = frames[0]
        return vol.deintegrate(rgbd(d, c, scale), K, T)
    d, c, T = stack(frames)
    return vol.deintegrate_batch(*cuda(d, c), K, T, depth_scale=scale)


def assert_reaches_every_branch(before, samples, stats):
    """The conditions of tests/test_planted_states_cpu.py, from the planted volume's dump and what the restatement counted (first
    chunk of the call).  -> (n, bytes, (underflow, fresh, remaining))"""
    first = samples[:ps.CHUNK]
    n, csum, missing = ps.sample_counts(before[0], first)
    under, fresh, rest = ps.removal_classes(before[2], n)
    quads = ps.quads_with_all_classes(under, fresh, rest)
    print(f"underflow {under.sum()}, fresh {fresh.sum()}, remaining {rest.sum()}, quads with all three {quads}, stats {stats}")
    assert min(under.sum(), fresh.sum(), rest.sum()) >= 200 and quads >= 50
    assert stats[1] >= 1 and stats[1] >= missing >= 1
    if len(samples) <= ps.CHUNK:
        assert stats == (sum(len(f.keys) for f in samples), missing, int(n[fresh | rest].sum()), int(under.sum()))
    return n, csum, (under, fresh, rest)


def removed_and_checked(name):
    """Plant REMOVALS[name], remove its frames, hold dump and stats to the restatement.  -> (volume, dump before, dump after, n, bytes)"""
    s, frames, samples, states, scale, stride = ps.removal_case(name)
    vol = planted(states, stride)
    before = vol.dump()
    ref, stats = deintegrate_reference(before, samples)
    n, csum, _ = assert_reaches_every_branch(before, samples, stats)
    st = remove(vol, s, frames, scale)
    after = vol.dump()
    print(f"{name}: colours after the removal in [{after[3].min():.6g}, {after[3].max():.6g}], stats {st.as_tuple()}")
    assert_bitwise(after, ref)
    assert st.as_tuple() == stats, (st.as_tuple(), stats)
    return vol, before, after, n, csum


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["single", "single odd"])
def test_single_frame_takes_all_three_branches_inside_one_quad(name):
    """160 x 120 at stride 4 and 97 x 61 at stride 1 with uint16 depth, consistent colours."""
    vol, before, after, n, csum = removed_and_checked(name)
    # a twin that was planted and never de-integrated differs only where the rule updates: n >= 1 and w0 >= n
    s, frames, samples, states, scale, stride = ps.removal_case(name)
    twin = planted(states, stride).dump()
    under, fresh, rest = ps.removal_classes(twin[2], n)
    np.testing.assert_array_equal(twin[0], after[0])
    changed = (twin[1].view(np.uint32) != after[1].view(np.uint32)) | (twin[2] != after[2]) | (twin[3] != after[3]).any(-1)
    np.testing.assert_array_equal(changed, fresh | rest)  # (the weight of every updated voxel moved: n >= 1)
    assert ps.clamp_ends(before, n, csum) == (0, 0)
    assert after[3].min() >= 0.0 and after[3].max() <= 255.0


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["batch5", "batch64"])
def test_batches_with_mixed_counts_per_voxel(name):
    """5 frames, and 64: the full width of the frame mask."""
    vol, before, after, n, csum = removed_and_checked(name)
    assert len(np.unique(n)) >= min(len(ps.removal_case(name)[1]), 20)  # counts from 0 up to (nearly) every frame of the batch
    assert before[2].max() > 7


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_seventy_frames_decide_per_chunk_of_64():
    """Weights strictly between a voxel's count in the first chunk and its count over the call: the first chunk's observations
    leave and the second chunk underflows.  One decision per call would remove nothing there."""
    s, frames, samples, states, scale, stride = ps.removal_case("chunk70")
    assert len(frames) == 70
    vol = planted(states, stride)
    before = vol.dump()
    ref, stats = deintegrate_reference(before, samples)
    per_call, stats_call = deintegrate_reference(before, samples, max_frames=70)
    differ = int((ref[2] != per_call[2]).sum())
    print(f"per chunk {stats}, per call {stats_call}, {differ} voxels differ")
    assert differ >= 200 and stats[3] != stats_call[3] and stats[2] != stats_call[2]
    assert_reaches_every_branch(before, samples, stats)
    st = remove(vol, s, frames, scale)
    assert st.voxels_underflow == stats[3] != stats_call[3]
    assert st.as_tuple() == stats
    assert_bitwise(vol.dump(), ref)


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_foreign_colours_stay_in_range():
    """Frames that were never fused into the voxels they are removed from: sum - bytes < 0 and sum - bytes > 255 w both occur, the
    sums are clamped as the contract states, and nothing downstream sees a colour outside 0..255."""
    vol, before, after, n, csum = removed_and_checked("foreign")
    low, high = ps.clamp_ends(before, n, csum)
    print(f"clamp: {low} voxels below 0, {high} above 255 w; colour range after [{after[3].min()}, {after[3].max()}]")
    assert low >= 100 and high >= 100
    assert after[3].min() >= 0.0 and after[3].max() <= 255.0
    mesh, cloud = vol.extract_triangle_mesh(), vol.extract_point_cloud()
    assert len(mesh.triangles) > 0 and len(cloud.points) > 0
    for colours in (np.asarray(mesh.vertex_colors), np.asarray(cloud.colors)):
        assert colours.min() >= 0.0 and colours.max() <= 1.0, (float(colours.min()), float(colours.max()))


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_extraction_caches_follow_a_planted_removal(monkeypatch):
    """tests/test_gpu_tsdf_deintegrate.py::test_extraction_caches_follow_a_deintegration on the three-branch state (a fifth of its
    units: arbitrary tsdf values put a surface into almost every cell), both extractions run before the removal."""
    s, frames, samples, _, scale, stride = ps.removal_case("single")
    states = ps.deintegration_target(samples, 15, drop=0.8)
    vol = planted(states, stride)
    vol.extract_triangle_mesh()
    vol.extract_point_cloud()
    before = vol.dump()
    ref, stats = deintegrate_reference(before, samples)
    assert_reaches_every_branch(before, samples, stats)
    st = remove(vol, s, frames, scale)
    assert st.as_tuple() == stats
    m1, p1 = vol.extract_triangle_mesh(), vol.extract_point_cloud()
    monkeypatch.setenv("HV_EXTRACT_INCREMENTAL", "0")
    m2, p2 = vol.extract_triangle_mesh(), vol.extract_point_cloud()
    assert len(m1.triangles) > 0 and len(p1.points) > 0
    for a, b in zip(canonical_mesh(m1.vertices, m1.triangles, m1.vertex_colors), canonical_mesh(m2.vertices, m2.triangles, m2.vertex_colors)):
        np.testing.assert_array_equal(a, b)
    o1, o2 = np.lexsort(np.asarray(p1.points).T), np.lexsort(np.asarray(p2.points).T)
    np.testing.assert_array_equal(np.asarray(p1.points)[o1], np.asarray(p2.points)[o2])
    np.testing.assert_array_equal(np.asarray(p1.colors)[o1], np.asarray(p2.colors)[o2])
    assert_bitwise(vol.dump(), ref)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_owner_sharded_ranks_add_up_to_the_single_volume():
    from pyslam_amd.distributed import block_owner

    s, frames, samples, states, scale, stride = ps.removal_case("batch5")
    single = planted(states, stride)
    owner = np.asarray(block_owner(states[0], 2))
    assert 0 < (owner == 0).sum() < len(owner)
    ranks = []
    for r in range(2):
        v = volume(VOX, TRUNC, depth_sampling_stride=stride)
        v.set_owner(r, 2)
        mine = tuple(x[owner == r] for x in states)
        ps.plant(v, mine)
        assert_bitwise(v.dump(), ps.as_dump(mine))
        ranks.append(v)
    before = single.dump()
    ref, stats = deintegrate_reference(before, samples)
    assert_reaches_every_branch(before, samples, stats)
    st = [remove(v, s, frames, scale) for v in [single] + ranks]
    assert st[0].as_tuple() == stats
    assert tuple(a + b for a, b in zip(st[1].as_tuple(), st[2].as_tuple())) == stats
    assert min(st[1].voxels_removed, st[2].voxels_removed, st[1].voxels_underflow, st[2].voxels_underflow, st[1].units_missing,
               st[2].units_missing) > 0
    dumps = [v.dump() for v in ranks]
    union = [np.concatenate([dp[k] for dp in dumps]) for k in range(4)]
    order = np.lexsort(union[0].T[::-1])
    assert_bitwise(tuple(u[order] for u in union), single.dump())
    assert_bitwise(single.dump(), ref)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def drifted(T, seed=3):
    """A few centimetres and a degree or so of drift per pose (tests/test_gpu_tsdf_deintegrate.py's)."""
    rng = np.random.default_rng(seed)
    out = np.array(T, np.float64, copy=True)
    for k in range(len(out)):
        a = rng.normal(0, 0.01, 3)
        Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        out[k, :3, :3] = Rz @ out[k, :3, :3]
        out[k, :3, 3] += rng.normal(0, 0.02, 3)
    return out


def test_reintegration_on_a_planted_target_claims_the_missing_units_and_grows(sweep_form):
    """reintegrate_batch = deintegrate_batch then integrate_batch, bit for bit, on a target that holds a seventh of the frames'
    touch sets in a pool far smaller than them: the removal skips the absent units, the integrate half claims them (and those of
    the new poses) and the pool grows inside the call."""
    s, frames, samples, _, scale, stride = ps.removal_case("batch5")
    states = ps.deintegration_target(samples, 17, drop=0.85)  # a seventh of the touch sets: the integrate half claims the rest
    K = intrinsic(s)
    d, c, T = stack(frames)
    T_new = drifted(T, seed=11)
    vol, twin = planted(states, stride, max_blocks=len(states[0]) + 4), planted(states, stride, max_blocks=len(states[0]) + 4)
    cap = vol.max_blocks()  # (planting may have doubled it: still far below what the frames touch)
    assert cap < 4 * len(states[0]) < len(ps.removal_case("batch5")[3][0])
    before = vol.dump()
    ref, stats = deintegrate_reference(before, samples)
    assert_reaches_every_branch(before, samples, stats)
    st = vol.reintegrate_batch(*cuda(d, c), K, T, T_new)
    st2 = twin.deintegrate_batch(*cuda(d, c), K, T)
    assert_bitwise(twin.dump(), ref)
    twin.integrate_batch(*cuda(d, c), K, T_new)
    assert st == st2 and st.as_tuple() == stats
    out = vol.dump()
    assert_bitwise(out, twin.dump())
    assert vol.max_blocks() > cap and vol.dropped_points() == 0
    held = {tuple(int(x) for x in k) for k in out[0]}
    absent = {tuple(int(x) for x in k) for f in samples for k in f.keys} - {tuple(int(x) for x in k) for k in before[0]}
    assert len(absent & held) > cap and len(held) > cap


# ---- prep: rectify maps, BGR order, uint16 depth --------------------------------------------------------------------------------
ODD = odd_config(97, 61)
CAMERAS = {"tiny": ("tiny_160x120_2cm", "float32", 1.0, 4), "odd": (ODD, "uint16", 5000.0, 1)}


def rectified_case(camera, start, count):
    """Frames of `camera` as a BGR sensor with TUM1's lens would hand them over (the pixels need not be rendered through the lens:
    both sides remap the same images), the rectify maps, the rectified intrinsics."""
    from pyslam_amd import prep
    from pyslam_amd.synthetic import CONFIGS
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    cfg, dtype, scale, stride = CAMERAS[camera]
    s, frames = frames_of(cfg, start, count, depth_dtype=dtype)
    fx, fy, cx, cy = s.intrinsics
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    dist = np.array(CONFIGS["tum1_640x480_5mm"]["dist"])
    new_K = prep.get_optimal_new_camera_matrix(K, dist, (s.width, s.height), 0.7, (s.width, s.height))[0]
    mx, my = prep.init_undistort_rectify_map(K, dist, new_K, (s.width, s.height))
    assert np.abs(mx - np.arange(s.width)[None]).max() > 1.0  # the maps move pixels
    intr = (float(new_K[0, 0]), float(new_K[1, 1]), float(new_K[0, 2]), float(new_K[1, 2]))
    bgr = [(dd, np.ascontiguousarray(cc[..., ::-1]), TT) for dd, cc, TT in frames]
    return s, bgr, mx, my, intr, PinholeCameraIntrinsic(s.width, s.height, *intr), scale, stride


def rectifying_volume(mx, my, stride):
    vol = volume(VOX, TRUNC, depth_sampling_stride=stride)
    vol.set_rectify_maps(mx, my)
    vol.set_color_order(bgr=True)
    return vol


def oracle_rectified(frames, mx, my, intr, scale, stride, poses=None):
    """The oracle fed what the reference's host prep makes of the BGR frames: remapped (depth nearest, colour bilinear), R and B swapped."""
    cpu = oracle.PortTsdf(VOX, TRUNC, depth_sampling_stride=stride, threads=8)
    K = np.array(intr, np.float64)
    for i, (d, c, T) in enumerate(frames):
        cpu.integrate(hp.remap_nearest(d, mx, my), hp.remap_linear_u8(np.ascontiguousarray(c[..., ::-1]), mx, my), K,
                      T if poses is None else poses[i], scale, 4.0)
    return cpu


@pytest.mark.parametrize("camera,where,path", [("tiny", "host", "online"), ("tiny", "device", "batch"), ("tiny", "host", "batch"),
                                               ("tiny", "device", "online"), ("odd", "host", "online"), ("odd", "host", "batch")])
def test_removal_under_maps_and_bgr_leaves_the_oracle_of_the_rest(camera, where, path):
    """Integrate 12, de-integrate every third: the frames go through the maps and the colour order on the way out as on the way in."""
    s, frames, mx, my, intr, K, scale, stride = rectified_case(camera, 10, 12)
    vol = rectifying_volume(mx, my, stride)
    d, c, T = stack(frames)
    put = (lambda *a: cuda(*a)) if where == "device" else (lambda *a: a)
    if path == "online":
        for dd, cc, TT in frames:
            vol.integrate(rgbd(*put(dd, cc), scale), K, TT)
    else:
        vol.integrate_batch(*put(d, c), K, T, depth_scale=scale)
    gone = list(range(0, 12, 3))
    st = vol.deintegrate_batch(*put(d[gone], c[gone]), K, T[gone], depth_scale=scale)
    assert st.units_missing == 0 and st.voxels_underflow == 0 and st.voxels_removed > 0
    keep = [f for i, f in enumerate(frames) if i not in gone]
    assert_oracle_match(vol.dump(), oracle_rectified(keep, mx, my, intr, scale, stride), f"{camera} {where} {path}: every third removed")
    # one more, through the single-frame call
    dd, cc, TT = keep[0]
    st = vol.deintegrate(rgbd(*put(dd, cc), scale), K, TT)
    assert st.units_missing == 0 and st.voxels_underflow == 0 and st.voxels_removed > 0
    assert_oracle_match(vol.dump(), oracle_rectified(keep[1:], mx, my, intr, scale, stride), f"{camera} {where} {path}: one more removed")


def test_reintegrating_seventy_frames_under_maps():
    """hv_tsdf_reintegrate_batch rectifies all F frames once and runs the integrate half with the maps switched off: two chunks on
    the way out, two sweeps on the way in."""
    s, frames, mx, my, intr, K, scale, stride = rectified_case("tiny", 0, 70)
    d, c, T = stack(frames)
    drift = drifted(T)
    vol, twin = rectifying_volume(mx, my, stride), rectifying_volume(mx, my, stride)
    for v in (vol, twin):
        v.integrate_batch(*cuda(d, c), K, drift)
    st = vol.reintegrate_batch(*cuda(d, c), K, drift, T)
    st2 = twin.deintegrate_batch(*cuda(d, c), K, drift)
    twin.integrate_batch(*cuda(d, c), K, T)
    assert st == st2 and st.voxels_underflow == 0 and st.units_missing == 0 and st.voxels_removed > 0
    out = vol.dump()
    assert_bitwise(out, twin.dump())
    assert_oracle_match(out, oracle_rectified(frames, mx, my, intr, scale, stride), "70 frames re-integrated under maps")


def test_maps_survive_a_reintegration_and_a_refused_one():
    from pyslam_amd import _lib as L
    from pyslam_amd._lib import HipVolError

    s, frames, mx, my, intr, K, scale, stride = rectified_case("odd", 4, 8)
    d, c, T = stack(frames[:6])
    drift = drifted(T, seed=5)
    vol = rectifying_volume(mx, my, stride)
    vol.integrate_batch(d, c, K, drift, depth_scale=scale)
    st = vol.reintegrate_batch(d, c, K, drift, T, depth_scale=scale)
    assert st.voxels_underflow == 0 and st.units_missing == 0
    dd, cc, TT = frames[6]
    vol.integrate(rgbd(dd, cc, scale), K, TT)
    assert_oracle_match(vol.dump(), oracle_rectified(frames[:7], mx, my, intr, scale, stride), "a frame fused after a re-integration")
    # refused calls: a T_new of the wrong length (the Python layer), no T_new at all (the library)
    before = vol.dump()
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        vol.reintegrate_batch(d, c, K, T, T[:3], depth_scale=scale)
    T16 = np.ascontiguousarray(T.reshape(6, 16))
    ia = K.as_array()
    stats = L.HvDeintegrateStats()
    with pytest.raises(HipVolError, match="Unsupported image format"):
        L.check(vol._lib.hv_tsdf_reintegrate_batch(vol._h, L.ptr(d), L.HV_DEPTH_U16, L.ptr(c), 6, s.height, s.width, L.ptr(ia), L.ptr(T16), None,
                                                   float(scale), 4.0, L.HV_HOST, ctypes.byref(stats)))
    assert_bitwise(vol.dump(), before)
    dd, cc, TT = frames[7]
    vol.integrate(rgbd(dd, cc, scale), K, TT)
    assert_oracle_match(vol.dump(), oracle_rectified(frames, mx, my, intr, scale, stride), "a frame fused after a refused re-integration")
