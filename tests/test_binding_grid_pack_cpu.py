"""What pack / unpack / save / load / packed_info of the block grids send over the C ABI, against the recording stand-in for the library
(tests/recording_lib.py; no GPU), on a VoxelBlockGrid and a semantic grid."""
import ctypes
import os

import numpy as np
import pytest

from pyslam_amd import _lib as L
from pyslam_amd import volumetric as V
from pyslam_amd import volumetric_semantic as S
from tests import grid_pack_reference as R
from tests.recording_lib import HANDLE, addr, ref, volume

GRIDS = [V.VoxelBlockGrid, S.VoxelBlockSemanticProbabilisticGrid]


def grid(cls):
    return volume(cls, voxel_size=0.0625, block_size=8)


def calls(vol):
    got, vol._lib.calls = vol._lib.calls, []
    for _, args in got:
        assert addr(args[0]) == HANDLE
    return got


@pytest.mark.parametrize("cls", GRIDS)
def test_pack_asks_for_the_size_then_packs_into_its_result(cls):
    vol = grid(cls)
    vol._lib.script("hv_grid_pack_size")
    out = vol.pack()
    (n0, a0), (n1, a1) = calls(vol)
    assert (n0, n1) == ("hv_grid_pack_size", "hv_grid_pack")
    assert type(ref(a0[1])) is L.HvGridPackInfo and type(ref(a1[4])) is L.HvGridPackInfo
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.ndim == 1
    assert addr(a1[1]) == addr(out) and a1[2] == out.size and a1[3] == L.HV_HOST


@pytest.mark.parametrize("cls", GRIDS)
def test_unpack_hands_over_the_operand_and_returns_the_info(cls):
    vol = grid(cls)
    buf = np.arange(16, dtype=np.uint8)
    st = vol.unpack(buf)
    ((name, args),) = calls(vol)
    assert name == "hv_grid_unpack" and addr(args[1]) == addr(buf) and args[2] == 16 and type(args[2]) is int and args[3] == L.HV_HOST
    assert type(ref(args[4])) is L.HvGridPackInfo
    assert isinstance(st, V.GridPackStats) and st.as_tuple() == (0, 0, 0, 0) and V.GridPackStats.__slots__ == ("blocks", "voxels", "extra_pairs", "bytes")
    vol.unpack(bytes(buf))
    ((name, args),) = calls(vol)
    assert name == "hv_grid_unpack" and args[2] == 16 and args[3] == L.HV_HOST and addr(args[1])
    torch = pytest.importorskip("torch")
    t = torch.from_numpy(buf)
    vol.unpack(t)
    ((name, args),) = calls(vol)
    assert addr(args[1]) == t.data_ptr() and args[2] == 16
    for bad in (np.zeros(4, np.float32), np.zeros((4, 4), np.uint8)):
        with pytest.raises(ValueError, match="a packed map is a 1-D uint8 buffer, got"):
            vol.unpack(bad)
        assert vol._lib.calls == []


@pytest.mark.parametrize("cls", GRIDS)
def test_save_packs_on_the_host_and_leaves_only_the_final_file(cls, tmp_path):
    vol = grid(cls)
    path = tmp_path / "map.hvg"
    path.write_bytes(b"an older map")
    st = vol.save(path)
    got = calls(vol)
    assert [n for n, _ in got] == ["hv_grid_pack_size", "hv_grid_pack"] and got[1][1][3] == L.HV_HOST
    assert isinstance(st, V.GridPackStats)
    assert os.listdir(tmp_path) == ["map.hvg"] and path.read_bytes() == b""  # (the stand-in reports a size of 0)

    def failing(*args):
        raise OSError("disk full")

    vol2 = grid(cls)
    real = os.replace
    os.replace = failing
    try:
        with pytest.raises(OSError, match="disk full"):
            vol2.save(path)
    finally:
        os.replace = real
    assert os.listdir(tmp_path) == ["map.hvg"]


def test_the_five_methods_are_the_grids_own_and_name_the_grid_abi():
    for cls in (V.VoxelBlockGrid, V.VoxelGrid, S.VoxelBlockSemanticGrid, S.VoxelBlockSemanticProbabilisticGrid, S.VoxelBlockSemanticGrid2,
                S.VoxelBlockSemanticProbabilisticGrid2, S.VoxelSemanticGrid, S.VoxelSemanticGridProbabilistic, S.VoxelSemanticGrid2,
                S.VoxelSemanticGridProbabilistic2):
        assert cls._PACKED[0] == "hv_grid_" and cls._MODE in R.MODES
        for name in ("pack", "unpack", "save", "load", "packed_info"):
            assert callable(getattr(cls, name))
    assert V.ScalableTSDFVolume._PACKED[0] == "hv_tsdf_"
    for name in ("hv_grid_pack_size", "hv_grid_pack", "hv_grid_unpack", "hv_grid_packed_check"):
        assert name in L.SIGNATURES
    assert ctypes.sizeof(L.HvGridPackInfo) == 32 and ctypes.sizeof(L.HvGridPackedHeader) == 80


def test_load_sizes_the_pool_for_the_blocks_and_for_the_chains():
    hdr = dict(blocks=10, chain_nodes=0)
    G = S.VoxelBlockSemanticProbabilisticGrid
    assert G._load_blocks(hdr) == 1024 and G._load_blocks(dict(hdr, blocks=3000)) == 6000 and G._load_blocks(hdr, 77) == 77
    # the node pool of a grid holds max(65536, 4 * max_blocks) nodes: chains within it change nothing, chains beyond it raise the pool
    assert G._load_blocks(dict(hdr, chain_nodes=65536)) == 1024 and G._load_blocks(dict(hdr, chain_nodes=65536), 77) == 77
    assert G._load_blocks(dict(hdr, chain_nodes=65537)) == 16385 and G._load_blocks(dict(hdr, chain_nodes=65537), 77) == 16385
    assert G._load_blocks(dict(blocks=40000, chain_nodes=320000)) == 80000 and G._load_blocks(dict(blocks=40000, chain_nodes=320001)) == 80001


def test_load_of_an_alias_refuses_another_block_size(tmp_path):
    path = tmp_path / "bs4.hvg"
    path.write_bytes(R.pack_reference(1, 4, np.zeros((0, 3), np.int32), np.zeros((0, 64, 16), np.uint32)))
    with pytest.raises(ValueError, match="block_size 4 cannot be loaded as VoxelSemanticGrid"):
        S.VoxelSemanticGrid.load(path)


def test_a_failing_map_task_reports_and_does_not_touch_the_volume(tmp_path):
    from pyslam_amd.dense.volumetric_integrator_base import (VolumetricIntegrationMapTaskType, VolumetricIntegrationTask,
                                                             VolumetricIntegratorBase)

    class Volume:
        calls = []
        _read_packed = staticmethod(V._Volume._read_packed)
        packed_info = staticmethod(V.VoxelBlockGrid.packed_info)

        def __getattr__(self, name):
            return lambda *a, **k: self.calls.append(name)

    front = VolumetricIntegratorBase.__new__(VolumetricIntegratorBase)
    front.volume = Volume()
    (tmp_path / "dense_map.hvmap").write_bytes(b"not a map")
    for path in (tmp_path / "nowhere" / "dense_map.hvmap", tmp_path / "dense_map.hvmap"):
        out = front._map_task(VolumetricIntegrationTask(task_type=VolumetricIntegrationMapTaskType.LOAD_MAP, load_save_path=str(path)))
        assert out.task_type is VolumetricIntegrationMapTaskType.LOAD_MAP and out.error and Volume.calls == []
    flag = lambda v: __import__("types").SimpleNamespace(value=v)
    done, cond = flag(0), __import__("threading").Condition()
    front._publish(out, None, None, flag(1), done, cond)
    assert done.value == front.kMapRequestFailed == 2


def test_load_refuses_a_file_of_another_mode_before_it_creates_anything(tmp_path):
    buf = R.pack_reference(1, 8, np.zeros((0, 3), np.int32), np.zeros((0, 512, 16), np.uint32))
    path = tmp_path / "voting.hvg"
    path.write_bytes(buf)
    with pytest.raises(ValueError, match="cannot be loaded as VoxelBlockGrid"):
        V.VoxelBlockGrid.load(path)
    with pytest.raises(ValueError, match="cannot be loaded as VoxelBlockSemanticGrid2"):
        S.VoxelBlockSemanticGrid2.load(path)
