"""GPU: save_map / load_map of the dense front.  An integrator's own task handler (volume_integration, the code its worker process
runs) is driven in-process on plain queues: a few keyframes, SAVE_MAP, a NEW integrator, LOAD_MAP, the remaining keyframes - and the
result equals that of an integrator that never stopped, bit for bit."""
import os
import queue
import threading
import types

import numpy as np
import pytest

from tests import dense_helpers as dh
from tests.conftest import sort_rows
from tests.test_gpu_dense import _params

pytestmark = pytest.mark.gpu


class InProcess:
    """An integrator initialised in this process, with the queues and flags VolumetricIntegratorBase.run hands volume_integration."""

    def __init__(self, cls, cam, **kw):
        from pyslam_amd.dense.volumetric_integrator_types import DatasetEnvironmentType, SensorType

        self.integ = cls.__new__(cls)
        self.integ.init(cam, DatasetEnvironmentType.INDOOR, SensorType.RGBD, {}, dict(kw))
        self.cam = cam
        self.q_in, self.q_out, self.q_management = queue.Queue(), queue.Queue(), queue.Queue()
        self.flag = lambda v: types.SimpleNamespace(value=v)
        self.running, self.saved, self.loaded, self.elapsed = self.flag(1), self.flag(0), self.flag(0), self.flag(0.0)

    def run(self, task):
        self.saved.value = 0
        self.q_in.put(task)
        self.integ.volume_integration(self.q_in, self.q_out, threading.Condition(), self.q_management, None, self.running, self.loaded,
                                      threading.Condition(), self.saved, threading.Condition(), self.elapsed)

    def keyframe(self, stream, i, semantic=False):
        from pyslam_amd.dense.volumetric_integrator_base import VolumetricIntegrationTask, VolumetricIntegrationTaskType

        kf = dh.FakeKeyFrame(i, stream, self.cam, semantic=semantic)
        self.run(VolumetricIntegrationTask(kf, kf.img, None, kf.depth_img, kf.semantic_img, task_type=VolumetricIntegrationTaskType.INTEGRATE))

    def map_task(self, which, path, acknowledged=1):
        from pyslam_amd.dense.volumetric_integrator_base import VolumetricIntegrationMapTaskType, VolumetricIntegrationTask

        self.run(VolumetricIntegrationTask(task_type=VolumetricIntegrationMapTaskType[which],
                                           load_save_path=os.path.join(str(path), self.integ.kPackedMapFile)))
        assert self.saved.value == acknowledged  # like SAVE: 1 done; kMapRequestFailed: the caller's save_map / load_map raises


def stop_and_go(cls, stream, cam, tmp_path, frames, cut, semantic=False, **kw):
    """-> (volume of the integrator that never stopped, volume of the one that loaded the first one's map after `cut` keyframes)."""
    whole, first = InProcess(cls, cam, **kw), InProcess(cls, cam, **kw)
    for i in frames:
        whole.keyframe(stream, i, semantic)
    for i in frames[:cut]:
        first.keyframe(stream, i, semantic)
    first.map_task("SAVE_MAP", tmp_path)
    assert sorted(os.listdir(tmp_path)) == ["dense_map.hvmap"]
    second = InProcess(cls, cam, **kw)
    second.keyframe(stream, frames[-1], semantic)  # (content that load_map has to replace)
    second.map_task("LOAD_MAP", tmp_path)
    for i in frames[cut:]:
        second.keyframe(stream, i, semantic)
    return whole.integ.volume, second.integ.volume


def test_voxel_grid_front_continues_from_a_saved_map(tmp_path):
    from pyslam_amd.dense.volumetric_integrator_voxel_grid import VolumetricIntegratorVoxelGrid
    from pyslam_amd.synthetic import SyntheticRGBD

    _params(0.02, 0.08)
    s = SyntheticRGBD("tiny_160x120_2cm")
    a, b = stop_and_go(VolumetricIntegratorVoxelGrid, s, dh.FakeCamera(s), tmp_path, [0, 1, 2, 3], 2)
    for x, y in zip(a.dump(), b.dump()):
        assert x.tobytes() == y.tobytes() and len(x) > 0
    va, vb = a.get_voxels(1), b.get_voxels(1)
    for x, y in zip(sort_rows(va.points, va.colors), sort_rows(vb.points, vb.colors)):
        np.testing.assert_array_equal(x, y)


def test_a_failing_map_task_is_acknowledged_and_leaves_the_map_as_it_was(tmp_path):
    """A missing, a truncated and a foreign file are refused before the volume is touched; a valid map the volume refuses (another
    voxel size) is undone.  Each time the request is acknowledged as failed, and a later load of a good map works."""
    from pyslam_amd.dense.volumetric_integrator_voxel_grid import VolumetricIntegratorVoxelGrid
    from pyslam_amd.synthetic import SyntheticRGBD
    from pyslam_amd.volumetric import ScalableTSDFVolume, VoxelBlockGrid

    _params(0.02, 0.08)
    s = SyntheticRGBD("tiny_160x120_2cm")
    front = InProcess(VolumetricIntegratorVoxelGrid, dh.FakeCamera(s))
    failed = front.integ.kMapRequestFailed
    for i in (0, 1):
        front.keyframe(s, i)
    held = [x.tobytes() for x in front.integ.volume.dump()]
    unchanged = lambda: [x.tobytes() for x in front.integ.volume.dump()] == held
    front.map_task("LOAD_MAP", tmp_path / "nowhere", acknowledged=failed)
    assert unchanged()
    good = tmp_path / "good"
    front.map_task("SAVE_MAP", good)
    whole = (good / "dense_map.hvmap").read_bytes()
    for name, content in (("truncated", whole[: len(whole) // 2]), ("foreign", ScalableTSDFVolume(0.02, 0.08, max_blocks=64).pack().tobytes())):
        os.makedirs(tmp_path / name)
        (tmp_path / name / "dense_map.hvmap").write_bytes(content)
        front.map_task("LOAD_MAP", tmp_path / name, acknowledged=failed)
        assert unchanged()
    other = VoxelBlockGrid(0.04, 8, max_blocks=64, max_points=1 << 12)
    other.integrate(np.array([[0.1, 0.2, 0.3]], np.float32), np.array([[0.5, 0.5, 0.5]], np.float32))
    os.makedirs(tmp_path / "coarser")
    other.save(tmp_path / "coarser" / "dense_map.hvmap")
    front.map_task("LOAD_MAP", tmp_path / "coarser", acknowledged=failed)
    assert unchanged()
    front.keyframe(s, 2)
    assert not unchanged()
    front.map_task("LOAD_MAP", good)
    assert unchanged()


@pytest.mark.parametrize("probabilistic", [False, True])
def test_semantic_front_continues_from_a_saved_map(tmp_path, probabilistic):
    from pyslam_amd.dense.parameters import Parameters
    from pyslam_amd.dense.volumetric_integrator_voxel_semantic_grid import VolumetricIntegratorVoxelSemanticGrid
    from pyslam_amd.synthetic import SyntheticRGBD
    from pyslam_amd.volumetric_semantic import get_next_object_id_peek, set_next_object_id
    from tests.semantic_helpers import CFG

    P = _params(0.02, 0.08)
    old = P.kVolumetricSemanticIntegrationUseInstanceIds
    P.kVolumetricSemanticIntegrationUseInstanceIds = True
    try:
        s = SyntheticRGBD(CFG, noise=True)
        cam = dh.FakeCamera(s)
        frames, cut = [0, 6, 12, 18], 2
        kw = dict(use_semantic_probabilistic=probabilistic)
        # the object ids come from one process-wide counter: the uninterrupted run first, then the interrupted one from the same start
        set_next_object_id(1)
        whole = InProcess(VolumetricIntegratorVoxelSemanticGrid, cam, **kw)
        for i in frames:
            whole.keyframe(s, i, True)
        end = get_next_object_id_peek()
        set_next_object_id(1)
        first = InProcess(VolumetricIntegratorVoxelSemanticGrid, cam, **kw)
        for i in frames[:cut]:
            first.keyframe(s, i, True)
        first.map_task("SAVE_MAP", tmp_path)
        set_next_object_id(1)  # (a new process: load_map brings the counter back)
        second = InProcess(VolumetricIntegratorVoxelSemanticGrid, cam, **kw)
        second.map_task("LOAD_MAP", tmp_path)
        for i in frames[cut:]:
            second.keyframe(s, i, True)
        assert get_next_object_id_peek() == end
        a, b = whole.integ.volume, second.integ.volume
        for x, y in zip(list(a.dump2(max_labels=254)) + list(a.dump_marginals()), list(b.dump2(max_labels=254)) + list(b.dump_marginals())):
            assert x.tobytes() == y.tobytes()
        sa, sb = a.get_object_segments(1, 0.0), b.get_object_segments(1, 0.0)
        # (a segment's class id is that of the first of its voxels in POOL order - object 0 spans classes - and the pool order is
        # not part of a map: the segments are compared by object id and voxels)
        rows = lambda pts: np.asarray(pts)[np.lexsort(np.asarray(pts).T[::-1])].tobytes()  # whole rows, sorted by (x, y, z)
        key = lambda g: sorted((o.object_id, len(o.points), rows(o.points)) for o in g.object_vector)
        assert key(sa) == key(sb) and len(sa.object_vector) >= 1
    finally:
        P.kVolumetricSemanticIntegrationUseInstanceIds = old


def test_tsdf_front_continues_from_a_saved_map(tmp_path):
    from pyslam_amd.dense.volumetric_integrator_tsdf import VolumetricIntegratorTsdf
    from pyslam_amd.synthetic import SyntheticRGBD

    _params(0.02, 0.08)
    s = SyntheticRGBD("tiny_160x120_2cm")
    a, b = stop_and_go(VolumetricIntegratorTsdf, s, dh.FakeCamera(s), tmp_path, [0, 1, 2, 3], 2)
    for x, y in zip(a.dump(), b.dump()):
        assert x.tobytes() == y.tobytes() and len(x) > 0
    assert a.pack().tobytes() == b.pack().tobytes()
