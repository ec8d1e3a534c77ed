"""GPU: packed TSDF maps (include/hipvol.h "Packed maps"; hv_pack.hip) - pack / unpack / save / load of ScalableTSDFVolume.

Bars: equalities only.  vol.pack() is, byte for byte, tests/pack_reference.py's pack_reference of the volume's own dump() and
export_numerators(unit_keys()); a map unpacked into a fresh volume dumps, exports, packs and behaves (ray_cast, extraction,
integrate, deintegrate, prune) exactly like the one that was packed; pack only reads; every refusal leaves the volume as it was.
Every corrupt buffer here is one the host validator rejects: no test hands the kernels a buffer that did not pass it.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import pack_reference as PR
from tests import planted_states as PS
from tests.conftest import canonical_mesh, sort_rows

pytestmark = pytest.mark.gpu

VOX, TRUNC = PS.VOX, PS.TRUNC
BOUNDARY_WORDS = (0, 31, 32, 63, 64, 255, 256, 4095)  # mask-word, wave and workgroup-iteration boundaries of the kernels
MANY = 2500


def fresh(max_blocks=1 << 12, voxel=VOX, trunc=TRUNC):
    from pyslam_amd.volumetric import ScalableTSDFVolume

    return ScalableTSDFVolume(voxel, trunc, max_blocks=max_blocks)


def dump_index(word):
    """The library's voxel word z * 256 + x * 16 + y -> the dump-order index x * 256 + y * 16 + z (PS.library_word's inverse)."""
    z, x, y = word >> 8, (word >> 4) & 15, word & 15
    return (x * 16 + y) * 16 + z


def one_voxel_payload(units, weight=3.0):
    """A numerators payload [units, 4096, 5] (word order): unit j is all-zero when j % 3 == 0, else holds one voxel at word
    (j * 37) % 4096 - 37 is coprime to 4096, so the words walk through every mask word."""
    payload = np.zeros((units, PR.NV, 5), np.float32)
    for j in range(units):
        if j % 3:
            k = (j * 37) % PR.NV
            payload[j, k] = (0.25 * weight * (1 if j % 2 else -1), weight, (j % 256) * weight, ((j * 7) % 256) * weight, 200.0 * weight)
    return payload


def plant_chunks(vol, units, chunk=250):
    """`units` units on a line of keys (negative and positive indices), planted in chunks from ONE payload."""
    payload = one_voxel_payload(chunk)
    for lo in range(0, units, chunk):
        n = min(chunk, units - lo)
        j = np.arange(lo, lo + n, dtype=np.int64)
        keys = np.stack([j - units // 2, (j * 5) % 7 - 3, 2 - j % 4], axis=1).astype(np.int32)
        vol.import_numerators(keys, payload[:n])
    return vol


def _finish_single(unit, i, tsdf, weight, colour, max_weight=7):
    t, w, c = np.zeros((1, PR.NV), np.float32), np.zeros((1, PR.NV), np.float32), np.zeros((1, PR.NV, 3))
    t[0, i], w[0, i], c[0, i] = tsdf, weight, colour
    return PS.finish([unit], t, w, c, max_weight=max_weight)


def _weightless_colour(vol):
    payload = np.zeros((2, PR.NV, 5), np.float32)
    payload[0, 1234] = (0, 0, 5, 0, 0)     # weight 0, a colour sum: stored
    payload[1, 77] = (0.5 * 2, 2, 20, 40, 60)
    vol.import_numerators(np.array([[2, -1, 0], [-3, 4, 1]], np.int32), payload)
    return vol


CASES = {
    "sparse source": lambda v: PS.plant(v, PS.sparse_source()),
    "boundary words": lambda v: PS.plant(v, PS.one_voxel_units(words=tuple(dump_index(k) for k in BOUNDARY_WORDS))[0]),
    "full unit": lambda v: PS.plant(v, PS.random_units([(1, -2, 3)], seed=11, unobserved=0.0)),
    "empty units": lambda v: PS.plant(v, PS.empty_units([(0, 0, 0), (-5, 2, 9), (7, 7, -7)])),
    "weightless colour": _weightless_colour,
    "negative zero": lambda v: PS.plant(v, _finish_single((0, -1, 2), 555, -0.0, 4, (1, 2, 3))),
    "weight 65000": lambda v: PS.plant(v, _finish_single((3, 3, 3), 4095, 0.75, 65000, (255, 255, 255), max_weight=PS.MAX_WEIGHT)),
    "many units": lambda v: plant_chunks(v, MANY),
}


def reference_bytes(vol):
    return PR.pack_reference(*PR.state_of_volume(vol), voxel_length=vol.voxel_length, sdf_trunc=vol.sdf_trunc)


def sorted_numerators(vol):
    keys = vol.unit_keys()
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return keys[order], vol.export_numerators(keys)[order]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (volume, the reference's bytes, its dump, its key-sorted numerators): planted once, shared, never written to."""
    vol = CASES[name](fresh())
    return vol, reference_bytes(vol), vol.dump(), sorted_numerators(vol)


def assert_dumps_bitwise(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[3], b[3])


# ---- bytes -------------------------------------------------------------------------------------------------------------------
def test_the_planted_cases_hold_what_they_are_named_for():
    state = PR.state_of_volume(case("weightless colour")[0])
    assert ((state[2] == 0) & (state[3] != 0).any(-1)).sum() == 1
    _, t, w, _ = PR.state_of_volume(case("negative zero")[0])
    assert ((t == 0x80000000) & (w > 0)).sum() == 1
    assert PR.state_of_volume(case("weight 65000")[0])[2].max() == 65000
    _, t, w, s = PR.state_of_volume(case("boundary words")[0])
    stored = (t != 0) | (w != 0) | (s != 0).any(-1)
    assert sorted(np.nonzero(stored)[1].tolist()) == sorted(BOUNDARY_WORDS) and (stored.sum(1) == 1).all()
    assert PR.header_reference(case("full unit")[1])["voxels"] == PR.NV
    h = PR.header_reference(case("empty units")[1])
    assert (h["units"], h["voxels"]) == (3, 0)
    h = PR.header_reference(case("many units")[1])
    assert h["units"] == MANY and 0 < h["voxels"] < MANY


@pytest.mark.parametrize("name", sorted(CASES))
def test_pack_equals_the_reference_byte_for_byte(name):
    vol, ref, _, _ = case(name)
    host = vol.pack()
    assert host.dtype == np.uint8 and host.ndim == 1
    assert host.tobytes() == ref
    dev = vol.pack(device=True)
    assert dev.is_cuda and dev.cpu().numpy().tobytes() == ref
    PR.check_reference(ref)


# ---- round trip --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["numpy", "cuda"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_unpack_into_a_fresh_volume_restores_the_map_bit_for_bit(name, source):
    import torch

    from pyslam_amd.volumetric import PackStats

    vol, ref, dump, (nkeys, numerators) = case(name)
    buf = np.frombuffer(ref, np.uint8)
    back = fresh()
    stats = back.unpack(torch.from_numpy(buf.copy()).cuda() if source == "cuda" else buf)
    h = PR.header_reference(ref)
    assert stats == PackStats(h["units"], h["voxels"], h["bytes"])
    assert back.num_blocks() == vol.num_blocks() == h["units"]
    np.testing.assert_array_equal(back.dirty_keys(), dump[0])
    assert len(back.touched_keys()) == 0
    assert_dumps_bitwise(back.dump(), dump)
    bkeys, bnum = sorted_numerators(back)
    np.testing.assert_array_equal(bkeys, nkeys)
    np.testing.assert_array_equal(bnum.view(np.uint32), numerators.view(np.uint32))
    assert back.pack().tobytes() == ref


def test_unpack_takes_bytes_and_cpu_tensors():
    import torch

    vol, ref, dump, _ = case("boundary words")
    for buf in (ref, bytearray(ref), torch.frombuffer(bytearray(ref), dtype=torch.uint8)):
        back = fresh()
        back.unpack(buf)
        assert_dumps_bitwise(back.dump(), dump)


# ---- a loaded map behaves like the original ----------------------------------------------------------------------------------
def fused_pair(tmp_path, frames=6):
    """Six tiny frames fused into a volume, saved, loaded: -> (camera, frames, intrinsic, original, loaded)."""
    from pyslam_amd.volumetric import RGBDImage, ScalableTSDFVolume
    from tests.test_gpu_tsdf_edges import intrinsic, tiny_frames

    s, fr = tiny_frames(0, 8)
    K = intrinsic(s)
    vol = fresh()
    for d, c, T in fr[:frames]:
        vol.integrate(RGBDImage(c, d, 1.0, 4.0), K, T)
    path = tmp_path / "map.hvtsdf"
    stats = vol.save(path)
    assert stats.units == vol.num_blocks() and stats.bytes == path.stat().st_size
    assert [p.name for p in tmp_path.iterdir()] == ["map.hvtsdf"]  # the temporary file is gone
    loaded = ScalableTSDFVolume.load(path)
    assert loaded.voxel_length == vol.voxel_length and loaded.sdf_trunc == vol.sdf_trunc
    assert loaded.max_blocks() >= max(1024, 2 * stats.units)
    return s, fr, K, vol, loaded


def test_loaded_map_casts_and_extracts_like_the_original(tmp_path):
    s, fr, K, vol, loaded = fused_pair(tmp_path)
    assert_dumps_bitwise(loaded.dump(), vol.dump())
    a = vol.ray_cast(K, fr[2][2], depth_min=0.1, depth_max=4.0, weight_threshold=0.5)
    b = loaded.ray_cast(K, fr[2][2], depth_min=0.1, depth_max=4.0, weight_threshold=0.5)
    assert a["mask"].any()
    for name in vol.RAY_CAST_ATTRIBUTES:
        np.testing.assert_array_equal(a[name].view(np.uint8), b[name].view(np.uint8), err_msg=name)
    ma, mb = vol.extract_triangle_mesh(), loaded.extract_triangle_mesh()
    assert len(ma.triangles) > 0
    for x, y in zip(canonical_mesh(ma.vertices, ma.triangles, ma.vertex_colors), canonical_mesh(mb.vertices, mb.triangles, mb.vertex_colors)):
        np.testing.assert_array_equal(x, y)
    pa, pb = vol.extract_point_cloud(), loaded.extract_point_cloud()
    assert len(pa.points) > 0
    for x, y in zip(sort_rows(np.hstack([pa.points, pa.colors])), sort_rows(np.hstack([pb.points, pb.colors]))):
        np.testing.assert_array_equal(x, y)


def test_loaded_map_fuses_a_further_frame_like_the_original(tmp_path):
    from pyslam_amd.volumetric import RGBDImage

    s, fr, K, vol, loaded = fused_pair(tmp_path)
    d, c, T = fr[6]
    for v in (vol, loaded):
        v.integrate(RGBDImage(c, d, 1.0, 4.0), K, T)
    np.testing.assert_array_equal(loaded.touched_keys(), vol.touched_keys())
    assert_dumps_bitwise(loaded.dump(), vol.dump())


def test_loaded_map_gives_a_frame_back_like_the_original(tmp_path):
    from pyslam_amd.volumetric import RGBDImage

    s, fr, K, vol, loaded = fused_pair(tmp_path)
    d, c, T = fr[3]
    sa = vol.deintegrate(RGBDImage(c, d, 1.0, 4.0), K, T)
    sb = loaded.deintegrate(RGBDImage(c, d, 1.0, 4.0), K, T)
    assert sa == sb and sa.voxels_removed > 0
    assert_dumps_bitwise(loaded.dump(), vol.dump())


def test_loaded_map_prunes_like_the_original(tmp_path):
    s, fr, K, vol, loaded = fused_pair(tmp_path)
    sa, sb = vol.prune(), loaded.prune()
    assert sa == sb and sa.units_before == sa.units_after + sa.units_empty
    assert_dumps_bitwise(loaded.dump(), vol.dump())


# ---- pack only reads ---------------------------------------------------------------------------------------------------------
def test_pack_leaves_the_volume_and_its_extractions_as_they_were(tmp_path):
    from pyslam_amd.volumetric import RGBDImage
    from tests.test_gpu_tsdf_edges import intrinsic, tiny_frames

    s, fr = tiny_frames(0, 3)
    K = intrinsic(s)
    vol = fresh()
    for d, c, T in fr:
        vol.integrate(RGBDImage(c, d, 1.0, 4.0), K, T)

    def observe():
        m = vol.extract_triangle_mesh()
        return vol.dump(), vol.dirty_keys(), vol.touched_keys(), (m.vertices.copy(), m.triangles.copy(), m.vertex_colors.copy())

    before = observe()
    assert len(before[2]) > 0 and len(before[3][1]) > 0
    first = vol.pack().tobytes()
    mid = vol.extract_triangle_mesh()  # (right behind the pack: what a cached extraction result would be served from)
    for x, y in zip((mid.vertices, mid.triangles, mid.vertex_colors), before[3]):
        np.testing.assert_array_equal(x, y)
    assert vol.pack(device=True).cpu().numpy().tobytes() == first
    assert vol.pack().tobytes() == first
    after = observe()
    assert_dumps_bitwise(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    np.testing.assert_array_equal(after[2], before[2])
    for x, y in zip(after[3], before[3]):
        np.testing.assert_array_equal(x, y)
    assert first == reference_bytes(vol)


# ---- growth ------------------------------------------------------------------------------------------------------------------
def test_unpack_grows_a_pool_that_is_too_small_or_leaves_the_volume_empty(monkeypatch):
    from pyslam_amd._lib import HipVolError

    src = plant_chunks(fresh(), 300)
    buf = src.pack()
    grown = fresh(max_blocks=64)
    grown.unpack(buf)
    assert grown.num_blocks() == 300 and grown.max_blocks() >= 300
    assert_dumps_bitwise(grown.dump(), src.dump())
    assert grown.pack().tobytes() == buf.tobytes()
    fixed = fresh(max_blocks=64)
    monkeypatch.setenv("HV_AUTO_GROW", "0")
    with pytest.raises(HipVolError, match="block pool exhausted"):
        fixed.unpack(buf)
    assert fixed.num_blocks() == 0 and fixed.max_blocks() == 64 and len(fixed.dump()[0]) == 0
    monkeypatch.delenv("HV_AUTO_GROW")
    fixed.unpack(buf)  # the refused volume is as good as new
    assert fixed.pack().tobytes() == buf.tobytes()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_unpack_refuses_a_volume_that_holds_units():
    from pyslam_amd._lib import HipVolError

    _, ref, _, _ = case("boundary words")
    held = PS.plant(fresh(), PS.empty_units([(9, 9, 9)]))  # even one all-zero unit
    before = held.dump()
    with pytest.raises(HipVolError, match="integrate_volume"):
        held.unpack(ref)
    assert held.num_blocks() == 1
    assert_dumps_bitwise(held.dump(), before)


@pytest.mark.parametrize("voxel,trunc", [(np.nextafter(VOX, 1.0), TRUNC), (VOX, np.nextafter(TRUNC, 0.0)), (0.01, 0.04)])
def test_unpack_refuses_another_voxel_length_or_truncation(voxel, trunc):
    from pyslam_amd._lib import HipVolError

    _, ref, _, _ = case("boundary words")
    other = fresh(voxel=float(voxel), trunc=float(trunc))
    with pytest.raises(HipVolError, match="bitwise equal"):
        other.unpack(ref)
    assert other.num_blocks() == 0


def test_voxel_grid_volumes_are_refused():
    from pyslam_amd import _lib as L
    from pyslam_amd.volumetric import VoxelBlockGrid

    _, ref, _, _ = case("boundary words")
    grid = VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12)
    lib = L.load()
    buf = np.frombuffer(ref, np.uint8)
    info = L.HvPackInfo()
    assert lib.hv_tsdf_unpack(grid._h, L.ptr(buf), buf.size, L.HV_HOST, ctypes.byref(info)) == -4  # HV_ERR_MODE
    assert b"TSDF mode" in lib.hv_last_error()
    assert lib.hv_tsdf_pack_size(grid._h, ctypes.byref(info)) == -4
    out = np.zeros(1 << 16, np.uint8)
    assert lib.hv_tsdf_pack(grid._h, L.ptr(out), out.size, L.HV_HOST, ctypes.byref(info)) == -4
    assert grid.num_blocks() == 0 and not out.any()


@pytest.mark.parametrize("sharding", ["tile", "owner"])
def test_sharded_volumes_are_refused(sharding):
    from pyslam_amd._lib import HipVolError

    _, ref, _, _ = case("boundary words")
    shard = lambda v: v.set_tile(0, 0, 80, 60) if sharding == "tile" else v.set_owner(0, 2)
    empty = fresh()
    shard(empty)
    with pytest.raises(HipVolError, match=f"{sharding}-sharded"):
        empty.unpack(ref)
    assert empty.num_blocks() == 0
    held = PS.plant(fresh(), PS.one_voxel_units(words=(0, 100))[0])
    before = held.dump()
    shard(held)
    for device in (False, True):
        with pytest.raises(HipVolError, match=f"{sharding}-sharded"):
            held.pack(device=device)
    assert_dumps_bitwise(held.dump(), before)
    # the settings are the volume's, not the map's: whole again, it packs
    held.set_tile(0, 0, 0, 0) if sharding == "tile" else held.set_owner(0, 1)
    assert held.pack().tobytes() == reference_bytes(held)


@functools.lru_cache(maxsize=None)
def corrupt():
    return PR.corrupt_buffers(case("sparse source")[1])


@functools.lru_cache(maxsize=None)
def refusing_volume():
    return fresh()


CORRUPT = ("wrong magic", "version 2", "one byte cut off", "one byte appended", "offset off 64", "two keys swapped", "duplicated key",
           "key out of range", "offsets[U] != N", "mask bit flipped", "decreasing offset")


def test_the_corrupt_list_is_complete():
    assert sorted(corrupt()) == sorted(CORRUPT)


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("name", CORRUPT)
def test_corrupt_buffers_end_as_exceptions_before_any_kernel(name, source):
    import torch

    from pyslam_amd._lib import HipVolError
    from pyslam_amd.volumetric import ScalableTSDFVolume

    bad, rule = corrupt()[name]
    with pytest.raises(ValueError):  # the host validator rejects it: the precondition of handing it to unpack at all
        ScalableTSDFVolume.packed_info(bad)
    vol = refusing_volume()
    buf = np.frombuffer(bad, np.uint8)
    with pytest.raises(HipVolError) as err:
        vol.unpack(torch.from_numpy(buf.copy()).cuda() if source == "device" else buf)
    assert PR.RULE_WORDS[rule] in str(err.value), str(err.value)
    assert vol.num_blocks() == 0 and len(vol.dump()[0]) == 0 and len(vol.dirty_keys()) == 0


def test_load_of_a_truncated_file_raises(tmp_path):
    from pyslam_amd.volumetric import ScalableTSDFVolume

    _, ref, _, _ = case("boundary words")
    (tmp_path / "cut.hvtsdf").write_bytes(ref[:-64])
    with pytest.raises(ValueError, match="total_bytes"):
        ScalableTSDFVolume.load(tmp_path / "cut.hvtsdf")


def test_pack_into_a_buffer_that_is_too_small_reports_the_size_and_writes_nothing():
    import torch

    from pyslam_amd import _lib as L

    vol, ref, _, _ = case("sparse source")
    lib = L.load()
    for out in (np.full(len(ref) - 1, 0xAB, np.uint8), torch.full((len(ref) - 1,), 0xAB, dtype=torch.uint8, device="cuda")):
        info = L.HvPackInfo()
        torch.cuda.synchronize()
        assert lib.hv_tsdf_pack(vol._h, L.ptr(out), len(ref) - 1, L.location(out), ctypes.byref(info)) == -3  # HV_ERR_CAPACITY
        h = PR.header_reference(ref)
        assert (info.units, info.voxels, info.bytes) == (h["units"], h["voxels"], len(ref))
        assert bool((out == 0xAB).all())
    size = L.HvPackInfo()
    assert lib.hv_tsdf_pack_size(vol._h, ctypes.byref(size)) == 0 and size.bytes == len(ref)


# ---- the empty volume --------------------------------------------------------------------------------------------------------
def test_an_empty_volume_packs_unpacks_saves_and_loads(tmp_path):
    from pyslam_amd.volumetric import PackStats, ScalableTSDFVolume

    vol = fresh()
    buf = vol.pack()
    empty = tuple(np.zeros((0,) + shape, dt) for shape, dt in (((3,), np.int32), ((PR.NV,), np.uint32), ((PR.NV,), np.uint32), ((PR.NV, 3), np.uint32)))
    assert buf.tobytes() == PR.pack_reference(*empty, voxel_length=VOX, sdf_trunc=TRUNC)
    assert vol.pack(device=True).cpu().numpy().tobytes() == buf.tobytes()
    info = ScalableTSDFVolume.packed_info(buf)
    assert (info["units"], info["voxels"], info["bytes"]) == (0, 0, len(buf))
    back = fresh()
    assert back.unpack(buf) == PackStats(0, 0, len(buf))
    assert back.num_blocks() == 0 and len(back.dirty_keys()) == 0
    assert vol.save(tmp_path / "empty.hvtsdf") == PackStats(0, 0, len(buf))
    loaded = ScalableTSDFVolume.load(tmp_path / "empty.hvtsdf")
    assert loaded.num_blocks() == 0 and loaded.max_blocks() == 1024 and loaded.pack().tobytes() == buf.tobytes()
