"""What lookup_points and label_mesh send over the C ABI, pinned against the recording stand-in for the library
(tests/recording_lib.py; no GPU), in the manner of tests/test_binding_calls_cpu.py, whose list of exercised public methods these
tests extend (its test_binding_covers_every_public_method counts them); and the labelled PLY files."""
import numpy as np
import pytest

from pyslam_amd import _lib as L
from pyslam_amd import volumetric as V
from pyslam_amd import volumetric_semantic as S
from pyslam_amd.dense import ply_io
from tests.recording_lib import ref, volume
from tests.test_binding_calls_cpu import P, REF, covers, expect, refused, shaped


@pytest.fixture(params=["numpy", "torch"])
def host(request):
    if request.param == "numpy":
        return lambda a: a
    torch = pytest.importorskip("torch")
    return torch.from_numpy


@pytest.mark.parametrize("f64", [False, True])
@covers("lookup_points")
def test_lookup_points_on_both_grid_families(host, f64):
    pts = np.zeros((5, 3), np.float64 if f64 else np.float32)
    p = host(pts)
    dt = L.HV_F64 if f64 else L.HV_F32
    plain = volume(V.VoxelBlockGrid, voxel_size=0.25, block_size=8)
    r = plain.lookup_points(p)
    (_, args), = expect(plain, ("hv_lookup_points", P(p), dt, 5, REF(L.HvLookupParams), P(r.status), P(r.count), P(r.position), P(r.color), None, None,
                                None, None, L.HV_HOST))
    prm = ref(args[4])
    assert (prm.min_count, prm.min_confidence, prm.radius) == (1, 0.0, 0)
    assert type(r) is V.VoxelLookup and r.class_id is None and r.object_id is None and r.confidence is None and r.stats is None
    shaped(r.status, (5,), np.uint8), shaped(r.count, (5,), np.int32), shaped(r.position, (5, 3), np.float64), shaped(r.color, (5, 3), np.float32)
    sem = volume(S.VoxelBlockSemanticGrid, voxel_size=0.25, block_size=8)
    r = sem.lookup_points(p, 2, 0.5, radius=2, stats=True, device=False)
    (_, args), = expect(sem, ("hv_lookup_points", P(p), dt, 5, REF(L.HvLookupParams), P(r.status), P(r.count), P(r.position), P(r.color),
                              P(r.class_id), P(r.object_id), P(r.confidence), REF(L.HvLookupStats), L.HV_HOST))
    prm = ref(args[4])
    assert (prm.min_count, prm.min_confidence, prm.radius) == (2, 0.5, 2)
    shaped(r.class_id, (5,), np.int32), shaped(r.object_id, (5,), np.int32), shaped(r.confidence, (5,), np.float32)
    assert type(r.stats) is V.LookupStats and r.stats.as_tuple() == (0, 0, 0, 0, 0)
    # an empty list is one call with n = 0
    r = sem.lookup_points(p[:0])
    expect(sem, ("hv_lookup_points", ("skip",), dt, 0, REF(L.HvLookupParams), ("skip",), ("skip",), ("skip",), ("skip",), ("skip",), ("skip",), ("skip",),
                 None, L.HV_HOST))
    assert len(r.status) == 0 and r.position.shape == (0, 3)


@covers("lookup_points")
def test_lookup_points_refuses_other_points():
    for vol in (volume(V.VoxelBlockGrid, voxel_size=0.25, block_size=8), volume(S.VoxelBlockSemanticGrid, voxel_size=0.25, block_size=8)):
        refused(vol, ValueError, "lookup_points: points must be float32 or float64", vol.lookup_points, np.zeros((4, 3), np.int32))
        refused(vol, ValueError, "lookup_points: points must be float32 or float64", vol.lookup_points, np.zeros((4, 3), np.float16))
        refused(vol, ValueError, "lookup_points: points must have shape [n, 3]", vol.lookup_points, np.zeros((4, 2), np.float32))
        refused(vol, ValueError, "lookup_points: points must have shape [n, 3]", vol.lookup_points, np.zeros(3, np.float64))
        refused(vol, ValueError, "lookup_points: points must have shape [n, 3]", vol.lookup_points, np.zeros((2, 2, 3), np.float64))
    torch = pytest.importorskip("torch")
    refused(vol, ValueError, "lookup_points: points must be float32 or float64", vol.lookup_points, torch.zeros((4, 3), dtype=torch.int64))


@covers("label_mesh")
def test_label_mesh_takes_meshes_clouds_and_images(host):
    sem = volume(S.VoxelBlockSemanticGrid, voxel_size=0.25, block_size=8)
    verts = np.zeros((7, 3), np.float64)
    mesh = V.TriangleMesh(host(verts), np.zeros((2, 3), np.int32), host(np.zeros((7, 3), np.float64)))
    g = sem.label_mesh(mesh)
    (_, args), = expect(sem, ("hv_lookup_points", P(verts), L.HV_F64, 7, REF(L.HvLookupParams), ("p", "any"), ("p", "any"), ("p", "any"), ("p", "any"),
                              P(g.class_ids), P(g.object_ids), P(g.confidences), None, L.HV_HOST))
    assert ref(args[4]).radius == 1 and ref(args[4]).min_count == 1
    assert type(g) is S.GeometryLabels
    shaped(g.class_ids, (7,), np.int32), shaped(g.object_ids, (7,), np.int32), shaped(g.confidences, (7,), np.float32), shaped(g.status, (7,), np.uint8)
    assert mesh.vertices is not None and tuple(mesh.vertices.shape) == (7, 3)  # the geometry is as it was
    cloud = V.PointCloud(host(np.zeros((3, 3), np.float32)), None)
    g = sem.label_mesh(cloud, min_count=2, min_confidence=0.25, radius=0)
    (_, args), = expect(sem, ("hv_lookup_points", P(cloud.points), L.HV_F32, 3, REF(L.HvLookupParams), ("p", "any"), ("p", "any"), ("p", "any"),
                              ("p", "any"), P(g.class_ids), P(g.object_ids), P(g.confidences), None, L.HV_HOST))
    assert (ref(args[4]).min_count, ref(args[4]).min_confidence, ref(args[4]).radius) == (2, 0.25, 0)
    image = host(np.zeros((4, 6, 3), np.float32))  # a ray-cast vertex image keeps its leading shape
    g = sem.label_mesh(image)
    expect(sem, ("hv_lookup_points", P(image), L.HV_F32, 24, REF(L.HvLookupParams), ("p", "any"), ("p", "any"), ("p", "any"), ("p", "any"),
                 ("p", "any"), ("p", "any"), ("p", "any"), None, L.HV_HOST))
    assert tuple(g.class_ids.shape) == (4, 6) and tuple(g.status.shape) == (4, 6) and g.confidences.dtype == np.float32
    refused(sem, ValueError, "label_mesh: points must have shape [..., 3]", sem.label_mesh, np.zeros((4, 2), np.float32))


def test_module_namespace_offers_the_lookup_names():
    import pyslam_amd.volumetric_module as volumetric

    assert (volumetric.LOOKUP_MISSING, volumetric.LOOKUP_OWN, volumetric.LOOKUP_NEAR, volumetric.LOOKUP_INVALID) == (0, 1, 2, 3)
    assert volumetric.VoxelLookup is V.VoxelLookup and volumetric.GeometryLabels is S.GeometryLabels and volumetric.LookupStats is V.LookupStats
    assert (L.HV_LOOKUP_MISSING, L.HV_LOOKUP_OWN, L.HV_LOOKUP_NEAR, L.HV_LOOKUP_INVALID) == (0, 1, 2, 3)


def test_ply_labels_round_trip_and_plain_files_stay_as_they_were(tmp_path):
    rng = np.random.default_rng(0)
    v, t, c = rng.random((6, 3)), np.array([[0, 1, 2], [3, 4, 5]], np.int32), rng.random((6, 3))
    cls, obj = np.arange(6, dtype=np.int32) - 1, np.arange(6, dtype=np.int32) * 7
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    ply_io.write_ply_mesh(a, v, t, c, class_ids=cls, object_ids=obj)
    pts, cols, faces = ply_io.read_ply(a)
    np.testing.assert_array_equal(pts, v), np.testing.assert_array_equal(faces, t)
    np.testing.assert_array_equal(cols, np.clip(np.rint(c * 255.0), 0, 255).astype(np.uint8))
    got = ply_io.read_ply_labels(a)
    np.testing.assert_array_equal(got[0], cls), np.testing.assert_array_equal(got[1], obj)
    header = open(a, "rb").read().split(b"end_header")[0].decode()
    assert "property int class_id\nproperty int object_id\nelement face 2" in header
    # without labels: the bytes of the writer as it was before labels existed
    ply_io.write_ply_mesh(b, v, t, c)
    want = ("ply\nformat binary_little_endian 1.0\ncomment Created by pyslam_amd\nelement vertex 6\nproperty double x\nproperty double y\n"
            "property double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 2\n"
            "property list uchar uint vertex_indices\nend_header\n").encode()
    vrec = np.zeros(6, dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    c8 = np.clip(np.rint(c * 255.0), 0, 255).astype(np.uint8)
    vrec["r"], vrec["g"], vrec["b"] = c8[:, 0], c8[:, 1], c8[:, 2]
    frec = np.zeros(2, dtype=[("n", "u1"), ("a", "<u4"), ("b", "<u4"), ("c", "<u4")])
    frec["n"], frec["a"], frec["b"], frec["c"] = 3, t[:, 0], t[:, 1], t[:, 2]
    assert open(b, "rb").read() == want + vrec.tobytes() + frec.tobytes()
    assert ply_io.read_ply_labels(b) == (None, None)
    # point clouds: labels behind normals and colours; one of the two may be left out
    ply_io.write_ply_points(a, v, c, v, object_ids=obj)
    np.testing.assert_array_equal(ply_io.read_ply(a)[0], v), np.testing.assert_array_equal(ply_io.read_ply_normals(a), v)
    got = ply_io.read_ply_labels(a)
    assert got[0] is None
    np.testing.assert_array_equal(got[1], obj)
    ply_io.write_ply_points(b, v, c)
    ply_io.write_ply_points(a, v, c, None, None, None)
    assert open(a, "rb").read() == open(b, "rb").read()
    with pytest.raises(ValueError):
        ply_io.write_ply_mesh(a, v, t, c, class_ids=cls[:-1])
