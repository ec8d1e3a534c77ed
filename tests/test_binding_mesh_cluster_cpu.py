"""What extract_simplified_mesh sends over the C ABI, pinned against the recording stand-in for the library (tests/recording_lib.py;
no GPU), in the manner of tests/test_binding_calls_cpu.py, whose list of exercised public methods these tests extend (its
test_binding_covers_every_public_method counts them); and the dense front's choice between the full and the simplified mesh."""
import types

import numpy as np
import pytest

from pyslam_amd import volumetric as V
from tests.test_binding_calls_cpu import I64, P, REF, covers, expect, refused, shaped, tsdf

QUERY = (None, None, 0, None, 0, None, 0, REF(I64), REF(I64), REF(I64))


@pytest.mark.parametrize("vertex_map", [False, True])
@pytest.mark.parametrize("dtype, suffix", [(None, ""), (np.float64, ""), (np.float32, "_f32")])
@covers("extract_simplified_mesh")
def test_simplified_mesh_is_a_query_and_a_fill(dtype, suffix, vertex_map):
    name = "hv_tsdf_extract_mesh_clustered" + suffix
    dt = np.float32 if suffix else np.float64
    vol = tsdf()
    vol._lib.script(name, 5, 7, 11)
    m = vol.extract_simplified_mesh(cell=8, dtype=dtype, vertex_map=vertex_map)
    got = expect(vol, (name, 8) + QUERY,
                 (name, 8, P(m.vertices), P(m.vertex_colors), 5, P(m.triangles), 7, P(m.vertex_cluster) if vertex_map else None,
                  11 if vertex_map else 0, REF(I64), REF(I64), REF(I64)))
    assert all(type(args[1]) is int for _, args in got)
    assert type(m) is V.TriangleMesh and hasattr(m, "vertex_cluster") == vertex_map
    shaped(m.vertices, (5, 3), dt), shaped(m.vertex_colors, (5, 3), dt), shaped(m.triangles, (7, 3), np.int32)
    if vertex_map:
        shaped(m.vertex_cluster, (11,), np.int32)
    assert m.vertex_normals.shape == (0, 3)


@covers("extract_simplified_mesh")
def test_simplified_mesh_defaults_and_zero_counts():
    vol = tsdf()
    vol._lib.script("hv_tsdf_extract_mesh_clustered", 3, 1, 9)
    m = vol.extract_simplified_mesh()  # cell 4, host, float64, no map
    expect(vol, ("hv_tsdf_extract_mesh_clustered", 4) + QUERY,
           ("hv_tsdf_extract_mesh_clustered", 4, P(m.vertices), P(m.vertex_colors), 3, P(m.triangles), 1, None, 0, REF(I64), REF(I64), REF(I64)))
    for cell in V.ScalableTSDFVolume.SIMPLIFIED_MESH_CELLS + (np.int32(2), np.int64(16)):
        vol._lib.script("hv_tsdf_extract_mesh_clustered", 0, 0, 0)
        m = vol.extract_simplified_mesh(cell=cell, vertex_map=True)  # nothing to fetch: a single call
        (_, args), = expect(vol, ("hv_tsdf_extract_mesh_clustered", int(cell)) + QUERY)
        assert type(args[1]) is int
        shaped(m.vertices, (0, 3), np.float64), shaped(m.vertex_colors, (0, 3), np.float64), shaped(m.triangles, (0, 3), np.int32)
        shaped(m.vertex_cluster, (0,), np.int32)
    vol._lib.script("hv_tsdf_extract_mesh_clustered", 3, 0, 3)  # (vertices without triangles: the fetch runs)
    m = vol.extract_simplified_mesh(cell=16, vertex_map=True)
    assert vol._lib.names() == ["hv_tsdf_extract_mesh_clustered"] * 2
    vol._lib.calls = []
    shaped(m.vertices, (3, 3), np.float64), shaped(m.triangles, (0, 3), np.int32), shaped(m.vertex_cluster, (3,), np.int32)


@covers("extract_simplified_mesh")
def test_simplified_mesh_refusals_come_before_any_call():
    vol = tsdf()
    for cell in (0, 1, 3, 32, 4.0, 4.5, "4", None, True, -4):
        refused(vol, ValueError, "extract_simplified_mesh: cell must be one of (2, 4, 8, 16) voxels", vol.extract_simplified_mesh, cell=cell)
    refused(vol, TypeError, "extraction dtype must be float64 (Open3D's) or float32, got int32", vol.extract_simplified_mesh, dtype=np.int32)
    refused(vol, TypeError, "extraction dtype must be float64 (Open3D's) or float32, got int32", vol.extract_simplified_mesh, 8, False, np.int32, True)


def test_triangle_mesh_keeps_its_positional_form():
    v, t, c = np.zeros((2, 3)), np.zeros((1, 3), np.int32), np.ones((2, 3))
    m = V.TriangleMesh(v, t, c)
    assert m.vertices is v and m.triangles is t and m.vertex_colors is c and not hasattr(m, "vertex_cluster")
    vc = np.zeros(5, np.int32)
    assert V.TriangleMesh(v, t, c, vertex_cluster=vc).vertex_cluster is vc


# ---- dense front: which mesh an output tick extracts ---------------------------------------------------------------------------
MARK = 777.0


class MarkingVolume:
    """The volume stand-in of tests/dense_helpers.py (the front's worker process builds it: nothing of it can be inspected from
    here) whose simplified mesh says how it was asked for: one vertex (cell, 1 if dtype is float32 else 0, MARK)."""

    def __init__(self, voxel_length, sdf_trunc):
        from tests.dense_helpers import OracleTsdfVolume

        self.inner = OracleTsdfVolume(voxel_length, sdf_trunc)

    def integrate(self, image, intrinsic, extrinsic):
        self.inner.integrate(image, intrinsic, extrinsic)

    def reset(self):
        self.inner.reset()

    def extract_triangle_mesh(self, **kw):
        assert set(kw) <= {"dtype"}
        return self.inner.extract_triangle_mesh()

    def extract_simplified_mesh(self, cell, **kw):
        assert set(kw) <= {"dtype"}
        vertex = np.array([[float(cell), 1.0 if kw.get("dtype") is np.float32 else 0.0, MARK]])
        return types.SimpleNamespace(vertices=vertex, triangles=np.zeros((0, 3), np.int32), vertex_colors=np.zeros((1, 3)),
                                     vertex_normals=np.zeros((0, 3)))

    def extract_point_cloud(self):
        return self.inner.extract_point_cloud()


def marking_factory(voxel_length, sdf_trunc, device, max_blocks, max_points):
    return MarkingVolume(voxel_length, sdf_trunc)


@pytest.mark.parametrize("cell, in_dtype", [(0, False), (4, False), (8, True)])
def test_dense_front_output_tick_and_save(cell, in_dtype, tmp_path, monkeypatch):
    """Parameter 0: today's full mesh; 2 / 4 / 8 / 16: extract_simplified_mesh(cell=...) with the same dtype keyword; SAVE always
    writes the full mesh."""
    from pyslam_amd.dense import VolumetricIntegrationTaskType, VolumetricIntegratorType, volumetric_integrator_factory
    from pyslam_amd.dense.parameters import Parameters
    from pyslam_amd.dense.ply_io import read_ply
    from pyslam_amd.dense.volumetric_integrator_types import DatasetEnvironmentType, SensorType
    from pyslam_amd.synthetic import SyntheticRGBD
    from tests import dense_helpers as dh
    from tests.test_dense_front_cpu import wait_until

    assert Parameters.kVolumetricIntegrationTsdfOutputMeshCell == 0  # the default is today's behaviour
    for name, value in (("kVolumetricIntegrationVoxelLength", 0.04), ("kVolumetricIntegrationTSdfTrunc", 0.12),
                        ("kVolumetricIntegrationOutputTimeInterval", 0.0), ("kVolumetricIntegrationMinNumLBATimes", 1),
                        ("kVolumetricIntegrationTsdfOutputMeshCell", cell),
                        ("kVolumetricIntegrationTsdfOutputInDenseMappingDtype", in_dtype)):
        monkeypatch.setattr(Parameters, name, value)
    s = SyntheticRGBD("tiny_160x120_2cm", noise=False)
    cam = dh.FakeCamera(s)
    integ = volumetric_integrator_factory(VolumetricIntegratorType.TSDF, cam, DatasetEnvironmentType.INDOOR, SensorType.RGBD,
                                          volume_factory=marking_factory)
    try:
        assert wait_until(integ.is_ready), "worker did not start"
        kf = dh.FakeKeyFrame(0, s, cam)
        integ.add_keyframe(kf, kf.img, None, kf.depth_img)
        got = []
        assert wait_until(lambda: (got.append(integ.pop_output(timeout=0.2)) or True) and got[-1] is not None)
        integ.add_update_output_task()
        assert wait_until(lambda: (got.append(integ.pop_output(timeout=0.2)) or True) and got[-1] is not None
                          and got[-1].task_type == VolumetricIntegrationTaskType.UPDATE_OUTPUT)
        meshes = [o.mesh for o in got if o is not None]
        assert len(meshes) >= 2
        for mesh in meshes:
            if cell == 0:
                assert len(mesh.vertices) > 100 and len(mesh.triangles) > 100
            else:
                assert mesh.vertices.tolist() == [[float(cell), 1.0 if in_dtype else 0.0, MARK]] and mesh.triangles.shape == (0, 3)
        integ.save(str(tmp_path))
        pts, _, faces = read_ply(str(tmp_path / "dense_map.ply"))
        assert len(pts) > 100 and faces is not None and len(faces) > 100  # the full mesh, whatever the ticks hand out
    finally:
        integ.quit()
