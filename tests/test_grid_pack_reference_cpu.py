"""CPU: the library's validator of packed grids (hv_grid_packed_check behind _BlockGrid.packed_info, no GPU) against the numpy
restatement of the format in tests/grid_pack_reference.py, which is written from the comment in include/hipvol.h."""
import numpy as np
import pytest

from pyslam_amd.volumetric import VoxelBlockGrid
from pyslam_amd.volumetric_semantic import VoxelBlockSemanticGrid
from tests import grid_pack_reference as R


def planted(mode, bs, long_maps):
    """Three blocks (negative and positive keys, given out of key order), block (-2, 0, 1) storing voxels 0 and nvox - 1."""
    nv, rw = bs ** 3, R.RECORD_BYTES[mode] // 4
    keys = np.array([[3, -1, 2], [-2, 0, 1], [0, 0, 0]], np.int32)
    words = np.zeros((3, nv, rw), np.uint32)
    extra = {}

    def put(b, k, n_pairs, **kw):
        pairs = [(10 + i, i % 3, -0.125 * (i + 1)) for i in range(n_pairs)] if mode == 2 else [(10 + i, i % 2, -0.25 * (i + 1)) for i in range(n_pairs)]
        w, more = R.record(mode, pairs=pairs if mode in R.MAP_MODES else (), **kw)
        words[b, k] = w
        if more:
            extra[(b, k)] = more

    put(1, 0, 17 if long_maps else 2, count=3, pos=(0.5, 0.25, 0.125), col=(1.0, 2.0, 3.0), obj=4, cls=2, counter=2, cls_counter=1, best=(0, 1))
    put(1, nv - 1, 1, count=1, pos=(-0.5, 0.0, 0.0), col=(9.0, 8.0, 7.0), obj=-1, cls=0, counter=1, cls_counter=1)
    put(0, min(5, nv - 1), 26 if long_maps else 6, count=2, pos=(1.0, 1.0, 1.0), obj=7, cls=1, counter=1, cls_counter=2)
    return keys, words, extra


CASES = [(mode, bs, long_maps) for mode in R.MODES for bs in (3, 4) for long_maps in ((False, True) if mode in R.MAP_MODES else (False,))]


@pytest.mark.parametrize("mode,bs,long_maps", CASES)
def test_validator_accepts_the_reference_buffers_and_returns_its_header(mode, bs, long_maps):
    keys, words, extra = planted(mode, bs, long_maps)
    buf = R.pack_reference(mode, bs, keys, words, extra, voxel_size=0.0625, next_object_id=9, depth_threshold=5.0, depth_decay_rate=0.25)
    ref = R.check_reference(buf)
    got = VoxelBlockGrid.packed_info(buf)
    assert got == {name: ref[name] for name in R.HEADER_FIELDS}
    assert got["blocks"] == 3 and got["voxels"] == 3 and (got["extra_pairs"] > 0) == long_maps
    assert len(buf) % 64 == 0 and got["bytes"] == len(buf)
    back = R.unpack_reference(buf)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    assert np.array_equal(back["keys"], keys[order]) and np.array_equal(back["words"], words[order])


def test_an_empty_grid_is_a_valid_buffer():
    for mode in R.MODES:
        buf = R.pack_reference(mode, 8, np.zeros((0, 3), np.int32), np.zeros((0, 512, R.RECORD_BYTES[mode] // 4), np.uint32))
        got = VoxelBlockSemanticGrid.packed_info(buf)
        assert (got["blocks"], got["voxels"], got["extra_pairs"], got["chain_nodes"]) == (0, 0, 0, 0) and got["mode"] == mode


@pytest.mark.parametrize("mode,bs,long_maps", CASES)
def test_validator_rejects_every_corrupt_buffer_with_the_rule_the_reference_names(mode, bs, long_maps):
    buf = R.pack_reference(mode, bs, *planted(mode, bs, long_maps))
    cases = R.corrupt_buffers(buf)
    assert ("high bit set" in cases) == (bs == 3) and ("extras sum off" in cases) == long_maps
    for name, (bad, rule) in cases.items():
        with pytest.raises(ValueError) as ref:
            R.check_reference(bad)
        assert str(ref.value) == rule, name
        with pytest.raises(ValueError) as lib:
            VoxelBlockGrid.packed_info(bad)
        assert R.RULE_WORDS[rule] in str(lib.value), (name, str(lib.value))
        assert str(lib.value).startswith("hv_grid_packed_check: "), name


def test_operand_kinds_and_files_agree(tmp_path):
    buf = R.pack_reference(2, 4, *planted(2, 4, True))
    want = VoxelBlockGrid.packed_info(buf)
    path = tmp_path / "grid.hvg"
    path.write_bytes(buf)
    for operand in (bytearray(buf), memoryview(buf), np.frombuffer(buf, np.uint8), path, str(path)):
        assert VoxelBlockGrid.packed_info(operand) == want
    cut = tmp_path / "cut.hvg"
    cut.write_bytes(buf[:-64])
    with pytest.raises(ValueError, match="total_bytes"):
        VoxelBlockGrid.packed_info(cut)
    cut.write_bytes(buf[:100])
    with pytest.raises(ValueError, match="fewer than"):
        VoxelBlockGrid.packed_info(cut)
    with pytest.raises(ValueError, match="1-D uint8"):
        VoxelBlockGrid.packed_info(np.zeros(4, np.float32))
