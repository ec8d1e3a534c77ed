"""GPU: TSDF de-integration and re-integration (include/hipvol.h, hv_tsdf_deintegrate) held to the numpy restatement
(tests/deintegrate_reference.py) bit for bit, and to the oracle fed only the frames that remain."""
import numpy as np
import pytest

from tests.conftest import canonical_mesh
from tests.deintegrate_reference import deintegrate_reference, frame_samples
from tests.test_gpu_tsdf_edges import cuda, frames_of, intrinsic, odd_config, oracle_of, stack, tiny_frames, volume

pytestmark = pytest.mark.gpu

VOX, TRUNC = 0.02, 0.08
ODD = odd_config(97, 61)


def rgbd(d, c, depth_scale=1.0, depth_trunc=4.0):
    from pyslam_amd.volumetric import RGBDImage

    return RGBDImage.create_from_color_and_depth(c, d, depth_scale, depth_trunc, False)


def samples_of(s, frames, depth_scale=1.0, stride=4):
    K = intrinsic(s).as_array()
    return [frame_samples(VOX, TRUNC, d, c, K, T, depth_scale, 4.0, stride) for d, c, T in frames]


def assert_bitwise(a, b):
    for x, y, name in zip(a, b, ("keys", "tsdf", "weight", "colour")):
        assert x.shape == y.shape, name
        assert np.array_equal(x.view(np.uint8) if x.dtype == np.float32 else x, y.view(np.uint8) if y.dtype == np.float32 else y), name


def assert_oracle_match(gpu_dump, cpu, label):
    """Keys the oracle holds are equal to the GPU's; weights and colour sums there are exact, tsdf within 1e-4; every other GPU
    unit is in the fresh state."""
    kg, tg, wg, cg = gpu_dump
    kc, tc, wc, cc = cpu.dump()
    index = {tuple(k): i for i, k in enumerate(kg)}
    sel = np.array([index[tuple(k)] for k in kc], np.int64)  # KeyError: the oracle holds a unit the GPU does not
    np.testing.assert_array_equal(wg[sel], wc)
    # colour: the integer sums are exact (the oracle keeps Open3D's double running mean, which can differ from sum / weight in
    # the last bit)
    np.testing.assert_array_equal(np.rint(cg[sel] * wg[sel][..., None]), np.rint(cc * wc[..., None]))
    np.testing.assert_allclose(cg[sel], cc, rtol=1e-12, atol=0)
    err = float(np.abs(tg[sel] - tc).max()) if len(sel) else 0.0
    print(f"{label}: max |tsdf - oracle| = {err:.3g} over {len(sel)} units")
    assert err <= 1e-4
    rest = np.setdiff1d(np.arange(len(kg)), sel)
    assert np.all(wg[rest] == 0) and np.all(tg[rest] == 0) and np.all(cg[rest] == 0)


@pytest.mark.parametrize("cfg,depth_dtype,stride", [("tiny_160x120_2cm", "float32", 1), ("tiny_160x120_2cm", "float32", 4),
                                                    ("tiny_160x120_2cm", "uint16", 4), ("odd", "uint16", 1)])
def test_single_frame_matches_the_restatement_bitwise(cfg, depth_dtype, stride):
    s, frames = frames_of(ODD if cfg == "odd" else cfg, 0, 6, depth_dtype=depth_dtype)
    scale = 5000.0 if depth_dtype == "uint16" else 1.0
    K = intrinsic(s)
    vol = volume(VOX, TRUNC, depth_sampling_stride=stride)
    for d, c, T in frames:
        vol.integrate(rgbd(d, c, scale), K, T)
    before = vol.dump()
    d, c, T = frames[2]
    st = vol.deintegrate(rgbd(d, c, scale), K, T)
    smp = samples_of(s, [frames[2]], scale, stride)
    ref, stats = deintegrate_reference(before, smp)
    assert_bitwise(vol.dump(), ref)
    assert st.as_tuple() == stats
    assert st.units_listed == sum(len(x.keys) for x in smp) and st.units_missing == 0 and st.voxels_removed > 0


@pytest.mark.parametrize("F", [1, 5, 64, 65, 130])
def test_batch_matches_the_restatement_bitwise(F):
    s, frames = tiny_frames(0, F + 6)
    K = intrinsic(s)
    vol = volume(VOX, TRUNC)
    vol.integrate_batch(*cuda(*stack(frames)[:2]), K, stack(frames)[2])
    before = vol.dump()
    d, c, T = stack(frames[:F])
    st = vol.deintegrate_batch(*cuda(d, c), K, T)
    ref, stats = deintegrate_reference(before, samples_of(s, frames[:F]))
    assert_bitwise(vol.dump(), ref)
    assert st.as_tuple() == stats
    assert st.voxels_removed > 0


def test_removing_a_subset_leaves_the_oracle_of_the_rest():
    s, frames = tiny_frames(10, 24)
    K = intrinsic(s)
    vol = volume(VOX, TRUNC)
    d, c, T = stack(frames)
    vol.integrate_batch(*cuda(d, c), K, T)
    gone = list(range(0, 24, 3))
    st = vol.deintegrate_batch(*cuda(d[gone], c[gone]), K, T[gone])
    assert st.voxels_underflow == 0 and st.units_missing == 0
    keep = [f for i, f in enumerate(frames) if i not in gone]
    assert_oracle_match(vol.dump(), oracle_of(s, keep, VOX, TRUNC), "every third frame removed")


def test_removing_everything_empties_the_map():
    s, frames = tiny_frames(0, 10)
    K = intrinsic(s)
    vol = volume(VOX, TRUNC)
    d, c, T = stack(frames)
    vol.integrate_batch(*cuda(d, c), K, T)
    n = vol.num_blocks()
    st = vol.deintegrate_batch(*cuda(d, c), K, T)
    assert st.voxels_underflow == 0 and st.voxels_removed > 0
    keys, t, w, col = vol.dump()
    assert vol.num_blocks() == n == len(keys)
    assert np.all(t == 0) and np.all(w == 0) and np.all(col == 0)
    assert vol.extract_triangle_mesh().triangles.shape[0] == 0
    assert len(vol.extract_point_cloud().points) == 0
    assert not vol.ray_cast(K, T[3], render_attributes=("mask",))["mask"].any()


def test_reintegrate_moves_frames_to_their_true_poses(sweep_form):
    s, frames = tiny_frames(20, 40)
    K = intrinsic(s)
    d, c, T = stack(frames)
    rng = np.random.default_rng(3)
    drift = T.copy()
    for k in range(len(drift)):  # a few centimetres and a degree or so of drift per frame
        a = rng.normal(0, 0.01, 3)
        Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        drift[k, :3, :3] = Rz @ drift[k, :3, :3]
        drift[k, :3, 3] += rng.normal(0, 0.02, 3)
    vol, twin = volume(VOX, TRUNC), volume(VOX, TRUNC)
    for v in (vol, twin):
        v.integrate_batch(*cuda(d, c), K, drift)
    st = vol.reintegrate_batch(*cuda(d, c), K, drift, T)
    st2 = twin.deintegrate_batch(*cuda(d, c), K, drift)
    twin.integrate_batch(*cuda(d, c), K, T)
    assert st == st2 and st.voxels_underflow == 0
    out = vol.dump()
    assert_bitwise(out, twin.dump())
    assert_oracle_match(out, oracle_of(s, frames, VOX, TRUNC), f"re-integrated ({sweep_form})")


def test_extraction_caches_follow_a_deintegration(monkeypatch):
    s, frames = tiny_frames(0, 16)
    K = intrinsic(s)
    d, c, T = stack(frames)
    vol = volume(VOX, TRUNC)
    vol.integrate_batch(*cuda(d, c), K, T)
    vol.extract_triangle_mesh()
    vol.extract_point_cloud()
    vol.deintegrate_batch(*cuda(d[4:12], c[4:12]), K, T[4:12])
    m1, p1 = vol.extract_triangle_mesh(), vol.extract_point_cloud()
    monkeypatch.setenv("HV_EXTRACT_INCREMENTAL", "0")
    m2, p2 = vol.extract_triangle_mesh(), vol.extract_point_cloud()
    for a, b in zip(canonical_mesh(m1.vertices, m1.triangles, m1.vertex_colors), canonical_mesh(m2.vertices, m2.triangles, m2.vertex_colors)):
        np.testing.assert_array_equal(a, b)
    o1, o2 = np.lexsort(np.asarray(p1.points).T), np.lexsort(np.asarray(p2.points).T)
    np.testing.assert_array_equal(np.asarray(p1.points)[o1], np.asarray(p2.points)[o2])
    np.testing.assert_array_equal(np.asarray(p1.colors)[o1], np.asarray(p2.colors)[o2])


def test_owner_sharded_ranks_sum_to_the_single_volume():
    s, frames = tiny_frames(30, 20)
    K = intrinsic(s)
    d, c, T = stack(frames)
    single = volume(VOX, TRUNC)
    ranks = [volume(VOX, TRUNC) for _ in range(2)]
    for r, v in enumerate(ranks):
        v.set_owner(r, 2)
    for v in [single] + ranks:
        v.integrate_batch(*cuda(d, c), K, T)
    st = [v.deintegrate_batch(*cuda(d[::2], c[::2]), K, T[::2]) for v in [single] + ranks]
    assert st[1].units_listed + st[2].units_listed == st[0].units_listed
    assert st[1].voxels_removed + st[2].voxels_removed == st[0].voxels_removed
    dumps = [v.dump() for v in ranks]
    union = [np.concatenate([dp[k] for dp in dumps]) for k in range(4)]
    order = np.lexsort(union[0].T[::-1])
    assert_bitwise(tuple(u[order] for u in union), single.dump())


def test_edge_cases_and_errors():
    from pyslam_amd._lib import HipVolError

    s, frames = tiny_frames(0, 4)
    K = intrinsic(s)
    d, c, T = stack(frames)
    vol = volume(VOX, TRUNC)
    st = vol.deintegrate_batch(*cuda(d, c), K, T)  # empty volume: nothing to take out
    assert st.units_listed > 0 and st.units_missing == st.units_listed and st.voxels_removed == 0 and vol.num_blocks() == 0
    vol.integrate_batch(*cuda(d, c), K, T)
    vol.reset()
    st = vol.deintegrate(rgbd(d[0], c[0]), K, T[0])
    assert st.units_missing == st.units_listed > 0 and vol.num_blocks() == 0
    # twice: the second call finds voxels only that frame observed empty
    vol.integrate_batch(*cuda(d, c), K, T)
    vol.deintegrate(rgbd(d[1], c[1]), K, T[1])
    before = vol.dump()
    st = vol.deintegrate(rgbd(d[1], c[1]), K, T[1])
    assert st.voxels_underflow > 0
    after = vol.dump()
    assert np.all(after[2] <= before[2])
    # zero frames: a no-op
    st = vol.deintegrate_batch(d[:0], c[:0], K, T[:0])
    assert st.as_tuple() == (0, 0, 0, 0)
    st = vol.reintegrate_batch(d[:0], c[:0], K, T[:0], T[:0])
    assert st.as_tuple() == (0, 0, 0, 0)
    assert_bitwise(vol.dump(), after)
    # bad operands are refused before the library
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        vol.deintegrate_batch(d, c.astype(np.float32), K, T)
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        vol.deintegrate_batch(d, c, K, T[:2])
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        vol.reintegrate_batch(d, c, K, T, T[:3])
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        vol.deintegrate(rgbd(d[0][:, :-1], c[0]), K, T[0])
    # tile-sharded volumes are refused
    tiled = volume(VOX, TRUNC)
    tiled.set_tile(0, 0, s.width // 2, s.height)
    with pytest.raises(HipVolError, match="tile"):
        tiled.deintegrate(rgbd(d[0], c[0]), K, T[0])
    assert_bitwise(vol.dump(), after)


def test_host_frames_and_the_oracle_agree_with_device_frames():
    s, frames = tiny_frames(40, 8)
    K = intrinsic(s)
    d, c, T = stack(frames)
    a, b = volume(VOX, TRUNC), volume(VOX, TRUNC)
    for v in (a, b):
        v.integrate_batch(*cuda(d, c), K, T)
    sa = a.deintegrate_batch(d[2:6], c[2:6], K, T[2:6])
    sb = b.deintegrate_batch(*cuda(d[2:6], c[2:6]), K, T[2:6])
    assert sa == sb
    assert_bitwise(a.dump(), b.dump())
    assert_oracle_match(a.dump(), oracle_of(s, frames[:2] + frames[6:], VOX, TRUNC), "host frames")
