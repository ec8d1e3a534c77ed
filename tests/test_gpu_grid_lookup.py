"""GPU: lookup_points of the five block grids and label_mesh of the semantic ones (hv_lookup_points) against the numpy restatement
of the contract (tests/lookup_reference.py) applied to the grid's OWN dump: bitwise, on the planted cases of tests/lookup_cases.py -
every case, every mode, float32 and float64 points, radius 0, 1 and 2 - at the point counts around a wave and a workgroup, in every
placement, queued behind an integrate without synchronisation, without touching the grid; its refusals; and end to end on a wall
fused into a TSDF map and a voting grid, through extract_triangle_mesh / ray_cast and the labelled PLY file."""
import numpy as np
import pytest

from tests import lookup_cases as lc
from tests import lookup_reference as lr

pytestmark = pytest.mark.gpu

MODES = ("plain", "voting", "probabilistic", "voting2", "probabilistic2")


def make_grid(mode, bs, voxel=lc.VOXEL, max_blocks=64, max_points=1 << 13):
    from pyslam_amd import volumetric as V
    from pyslam_amd import volumetric_semantic as S

    cls = {"plain": V.VoxelBlockGrid, "voting": S.VoxelBlockSemanticGrid, "probabilistic": S.VoxelBlockSemanticProbabilisticGrid,
           "voting2": S.VoxelBlockSemanticGrid2, "probabilistic2": S.VoxelBlockSemanticProbabilisticGrid2}[mode]
    return cls(voxel, bs, max_blocks=max_blocks, max_points=max_points)


def gpu_carve(grid, depth, threshold):
    from pyslam_amd.volumetric import CameraFrustrum

    grid.carve(CameraFrustrum(*lc.INTR, lc.W, lc.H, np.eye(4), depth_max=lc.DEPTH_MAX, depth_min=lc.DEPTH_MIN), depth, threshold)


def planted(mode, case):
    grid = make_grid(mode, case.bs)
    lc.run_case(grid, case, mode != "plain", gpu_carve)
    return grid


def state_of(mode, grid):
    return lr.plain_state(grid.dump()) if mode == "plain" else lr.semantic_state(grid.dump2())


def param_sets(case, state):
    sets = list(case.params)
    if case.conf_voxel is not None and not state["plain"]:
        b, l = lr._index(state, case.bs)[case.conf_voxel]
        conf = np.float32(state["conf"][b, l])
        sets += [(1, float(conf)), (1, float(np.nextafter(conf, np.float32(2.0))))]
    return sets


def check(grid, state, bs, pts, mc, conf, radius, where):
    want = lr.lookup(state, pts, lc.VOXEL, bs, mc, conf, radius)
    got = grid.lookup_points(pts, mc, conf, radius, stats=True)
    bad = lr.same(want, got)
    assert bad is None, (where, bad, getattr(got, bad), want[bad])
    assert got.stats.as_tuple() == lr.status_counts(want["status"]), where
    return want


@pytest.mark.parametrize("bs", lc.BLOCK_SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_every_planted_case_answers_as_the_restatement(mode, bs):
    seen = set()
    for case in lc.cases(bs):
        grid = planted(mode, case)
        state = state_of(mode, grid)
        assert len(state["keys"]) == case.n_blocks() or case.name == "reset"
        for dtype in (np.float32, np.float64):
            pts = case.points(dtype)
            for mc, conf in param_sets(case, state):
                for radius in (0, 1, 2):
                    want = check(grid, state, bs, pts, mc, conf, radius, (case.name, np.dtype(dtype).name, mc, conf, radius))
                    seen.update(want["status"].tolist())
        if mode.startswith("probabilistic") and case.name == "chain":
            assert grid.prob_nodes_used() >= 2 and grid.label_overflows() == 0  # the maps did run into chained nodes
        grid.close()
    assert seen == {lr.MISSING, lr.OWN, lr.NEAR, lr.INVALID}


@pytest.mark.parametrize("mode", MODES)
def test_point_counts_around_a_wave_and_a_workgroup(mode):
    bs = 8
    case = lc.cases(bs)[0]
    grid = planted(mode, case)
    state = state_of(mode, grid)
    for n in lc.POINT_COUNTS + (257,):
        for dtype in (np.float32, np.float64):
            pts = np.ascontiguousarray(lc.counted_queries(case, n).astype(dtype))
            for radius in (0, 1, 2):
                check(grid, state, bs, pts, 1, 0.0, radius, (n, np.dtype(dtype).name, radius))
    r = grid.lookup_points(np.zeros((0, 3), np.float32), stats=True)
    assert r.stats.as_tuple() == (0, 0, 0, 0, 0) and len(r.status) == 0


@pytest.mark.parametrize("mode", ("plain", "probabilistic"))
def test_every_placement_gives_the_same_values(mode):
    import torch

    bs = 8
    case = lc.cases(bs)[0]
    grid = planted(mode, case)
    pts = lc.counted_queries(case, 129)
    host = grid.lookup_points(pts, radius=1)
    assert isinstance(host.status, np.ndarray)
    dev_pts = torch.from_numpy(pts).cuda()
    for got, on_gpu in ((grid.lookup_points(dev_pts, radius=1), True), (grid.lookup_points(dev_pts, radius=1, device=False), False),
                        (grid.lookup_points(pts, radius=1, device=True), True), (grid.lookup_points(torch.from_numpy(pts), radius=1), False)):
        for f in lr.FIELDS:
            a, b = getattr(host, f), getattr(got, f)
            if a is None:
                assert b is None
                continue
            assert (isinstance(b, torch.Tensor) and b.is_cuda) == on_gpu, f
            b = b.cpu().numpy() if isinstance(b, torch.Tensor) else b
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
    # two calls on equal inputs: bitwise equal
    again = grid.lookup_points(pts, radius=1)
    assert lr.same(host, again) is None


def test_a_device_call_without_stats_is_ordered_behind_the_integrate():
    import torch

    bs = 8
    grid = make_grid("voting", bs)
    case = lc.cases(bs)[0]
    pts = lc.counted_queries(case, 65)
    dev_pts = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    lc.run_case(grid, case, True, gpu_carve)  # queued on the grid's stream
    moved = dev_pts + 0.0                      # a torch kernel on torch's stream
    got = grid.lookup_points(moved, radius=1)  # no stats: nothing is read back, nothing waits
    found = (got.status == lr.OWN) | (got.status == lr.NEAR)  # (torch work queued behind the lookup)
    want = lr.lookup(state_of("voting", grid), pts, lc.VOXEL, bs, 1, 0.0, 1)
    assert lr.same(want, {f: getattr(got, f).cpu().numpy() for f in lr.FIELDS}) is None
    assert int(found.sum()) == lr.status_counts(want["status"])[1] + lr.status_counts(want["status"])[2] > 0


def test_a_lookup_changes_nothing():
    from pyslam_amd.volumetric import CameraFrustrum

    bs = 8
    case = [c for c in lc.cases(bs) if c.name == "reset"][0]
    grid = planted("probabilistic", case)
    cls_img, inst_img = np.full((lc.H, lc.W), 3, np.int32), np.full((lc.H, lc.W), 7, np.int32)
    assert grid.assoc_vote(CameraFrustrum(*lc.INTR, lc.W, lc.H, np.eye(4), depth_max=lc.DEPTH_MAX, depth_min=lc.DEPTH_MIN), cls_img, inst_img)
    before, pairs = grid.dump2(), grid.assoc_pairs()
    assert len(pairs[0]) > 0
    blocks, nodes = grid.num_blocks(), grid.prob_nodes_used()
    for radius in (0, 1, 2):
        for dtype in (np.float32, np.float64):
            grid.lookup_points(lc.counted_queries(case, 129).astype(dtype), radius=radius, stats=True)
    after, pairs_after = grid.dump2(), grid.assoc_pairs()
    for a, b in zip(before + pairs, after + pairs_after):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert (grid.num_blocks(), grid.prob_nodes_used(), grid.dropped_points()) == (blocks, nodes, 0)


def test_refusals():
    import ctypes

    from pyslam_amd import _lib as L
    from pyslam_amd.volumetric import ScalableTSDFVolume

    ERR_INVALID, ERR_MODE = -1, -4  # hv_status (include/hipvol.h)
    pts = np.zeros((4, 3), np.float32)
    for mode in ("plain", "voting"):
        grid = make_grid(mode, 8)
        for radius in (3, -1):
            with pytest.raises(L.HipVolError, match="radius must be 0, 1 or 2"):
                grid.lookup_points(pts, radius=radius)
        with pytest.raises(ValueError, match="float32 or float64"):
            grid.lookup_points(pts.astype(np.int32))
        with pytest.raises(ValueError, match=r"shape \[n, 3\]"):
            grid.lookup_points(np.zeros((4, 2), np.float32))
    # a label output on the plain grid, and a TSDF volume, at the C interface
    plain = make_grid("plain", 8)
    prm = L.HvLookupParams(1, 0.0, 0)
    status, ids = np.zeros(4, np.uint8), np.zeros(4, np.int32)
    for k in range(3):
        labels = [None, None, None]
        labels[k] = L.ptr(ids)
        rc = plain._lib.hv_lookup_points(plain._h, L.ptr(pts), L.HV_F32, 4, ctypes.byref(prm), L.ptr(status), None, None, None, *labels, None, L.HV_HOST)
        assert rc == ERR_INVALID and b"plain voxel grid" in plain._lib.hv_last_error()
    assert plain._lib.hv_lookup_points(plain._h, L.ptr(pts), 2, 4, ctypes.byref(prm), L.ptr(status), None, None, None, None, None, None, None,
                                       L.HV_HOST) == ERR_INVALID
    assert plain._lib.hv_lookup_points(plain._h, None, L.HV_F32, 4, ctypes.byref(prm), L.ptr(status), None, None, None, None, None, None, None,
                                       L.HV_HOST) == ERR_INVALID
    tsdf = ScalableTSDFVolume(0.02, 0.08, max_blocks=16)
    rc = tsdf._lib.hv_lookup_points(tsdf._h, L.ptr(pts), L.HV_F32, 4, ctypes.byref(prm), L.ptr(status), None, None, None, None, None, None, None, L.HV_HOST)
    assert rc == ERR_MODE


# ---- end to end: a wall fused into a TSDF map and a voting grid ------------------------------------------------------------------
WALL_Z, WALL_VOXEL = 2.05, 0.125
WALL_SHIFTS = ((0.0, 0.0), (0.25, 0.0), (0.0, 0.25))


def wall_scene():
    """-> (TSDF volume, voting grid) of the same voxel size, fused from the same three 64 x 48 frames of a fronto-parallel wall at
    z = 2.05 m seen from cameras shifted in x / y; the wall's left half (world x < 0) is class 1 / instance 1, its right half 2 / 2."""
    from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume

    K = PinholeCameraIntrinsic(lc.W, lc.H, *lc.INTR)
    tsdf = ScalableTSDFVolume(WALL_VOXEL, 4 * WALL_VOXEL, max_blocks=256)
    grid = make_grid("voting", 8, voxel=WALL_VOXEL, max_blocks=256)
    u = np.arange(lc.W, dtype=np.float64)[None, :].repeat(lc.H, 0)
    depth = np.full((lc.H, lc.W), WALL_Z, np.float32)
    rgb = np.full((lc.H, lc.W, 3), 128, np.uint8)
    poses = []
    for sx, sy in WALL_SHIFTS:
        T = np.eye(4)  # world -> camera: the camera sits at (sx, sy, 0)
        T[0, 3], T[1, 3] = -sx, -sy
        world_x = (u - lc.INTR[2]) / lc.INTR[0] * WALL_Z + sx
        cls = np.where(world_x < 0.0, 1, 2).astype(np.int32)
        tsdf.integrate(RGBDImage.create_from_color_and_depth(rgb, depth, 1.0, 4.0, False), K, T)
        grid.integrate_rgbd(depth, rgb, *lc.INTR, T, class_ids_image=cls, object_ids_image=cls.copy(), max_depth=4.0)
        poses.append(T)
    return tsdf, grid, K, poses


def test_a_tsdf_mesh_and_a_ray_cast_image_take_their_labels_from_the_grid(tmp_path):
    """label_mesh(extract_triangle_mesh(device=True), radius=1) and label_mesh(ray_cast(...)["vertex"], radius=1) equal the
    restatement bitwise; both classes occur; at least half the points are found - a floor against a vacuous test, which the
    restatement alone clears on the grid's dump.  Measured on an MI355X: 821 mesh vertices, all 821 found (every one in its own
    voxel: share 1.0000); 3 071 of 3 072 pixels hit by the ray cast, all found (1.0000)."""
    import torch

    from pyslam_amd.dense import ply_io

    tsdf, grid, K, poses = wall_scene()
    state = lr.semantic_state(grid.dump2())
    mesh = tsdf.extract_triangle_mesh(device=True)
    assert isinstance(mesh.vertices, torch.Tensor) and mesh.vertices.is_cuda and len(mesh.vertices) > 500
    verts_before = mesh.vertices.clone()
    labels = grid.label_mesh(mesh, radius=1)
    verts = mesh.vertices.cpu().numpy()
    assert np.array_equal(verts, verts_before.cpu().numpy())
    want = lr.lookup(state, verts, WALL_VOXEL, 8, 1, 0.0, 1)
    n, own, near, missing, invalid = lr.status_counts(want["status"])
    print(f"mesh: {n} vertices, own {own}, near {near}, missing {missing}, invalid {invalid}: found {(own + near) / n:.4f}")
    assert 2 * (own + near) >= n and invalid == 0  # the restatement alone clears the floor
    for name, field in (("class_ids", "class_id"), ("object_ids", "object_id"), ("confidences", "confidence"), ("status", "status")):
        got = getattr(labels, name)
        assert got.is_cuda and got.cpu().numpy().tobytes() == want[field].tobytes(), name
    found = want["status"] != lr.MISSING
    assert set(want["class_id"][found].tolist()) == {1, 2}
    # the labels follow the wall's halves: away from the seam a vertex on the left is class 1, on the right class 2
    cls = labels.class_ids.cpu().numpy()
    assert (cls[found & (verts[:, 0] < -0.25)] == 1).all() and (cls[found & (verts[:, 0] > 0.25)] == 2).all()
    # a host extraction gives the same labels, as numpy arrays
    host_labels = grid.label_mesh(tsdf.extract_triangle_mesh(), radius=1)
    assert isinstance(host_labels.class_ids, np.ndarray) and host_labels.class_ids.tobytes() == want["class_id"].tobytes()

    # the ray-cast vertex image, with its mask
    cast = tsdf.ray_cast(K, poses[0], depth_min=0.25, depth_max=4.0, weight_threshold=0.0, render_attributes=("vertex", "mask"), device=True)
    image = grid.label_mesh(cast["vertex"], radius=1)
    assert tuple(image.class_ids.shape) == (lc.H, lc.W)
    vimg, mask = cast["vertex"].cpu().numpy(), cast["mask"].cpu().numpy().astype(bool)
    want_img = lr.lookup(state, vimg.reshape(-1, 3), WALL_VOXEL, 8, 1, 0.0, 1)
    for name, field in (("class_ids", "class_id"), ("object_ids", "object_id"), ("confidences", "confidence"), ("status", "status")):
        assert getattr(image, name).cpu().numpy().tobytes() == want_img[field].tobytes(), name
    hit = want_img["status"].reshape(lc.H, lc.W)[mask]
    print(f"ray cast: {int(mask.sum())} pixels hit, found {float((hit != lr.MISSING).mean()):.4f}")
    assert mask.sum() > lc.H * lc.W // 2 and 2 * int((hit != lr.MISSING).sum()) >= int(mask.sum())
    assert set(want_img["class_id"].reshape(lc.H, lc.W)[mask & (want_img["status"].reshape(lc.H, lc.W) != lr.MISSING)].tolist()) == {1, 2}

    # PLY: with labels the geometry reads back equal; without, the file is what the writer gave before labels existed
    host_mesh = tsdf.extract_triangle_mesh()
    a, b = str(tmp_path / "labelled.ply"), str(tmp_path / "plain.ply")
    ply_io.write_ply_mesh(a, host_mesh.vertices, host_mesh.triangles, host_mesh.vertex_colors, class_ids=host_labels.class_ids,
                          object_ids=host_labels.object_ids)
    pts, cols, faces = ply_io.read_ply(a)
    assert np.array_equal(pts, host_mesh.vertices) and np.array_equal(faces, host_mesh.triangles)
    got_cls, got_obj = ply_io.read_ply_labels(a)
    assert np.array_equal(got_cls, host_labels.class_ids) and np.array_equal(got_obj, host_labels.object_ids)
    ply_io.write_ply_mesh(b, host_mesh.vertices, host_mesh.triangles, host_mesh.vertex_colors)
    header = (f"ply\nformat binary_little_endian 1.0\ncomment Created by pyslam_amd\nelement vertex {len(pts)}\nproperty double x\n"
              f"property double y\nproperty double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face {len(faces)}\n"
              "property list uchar uint vertex_indices\nend_header\n").encode()
    data = open(b, "rb").read()
    assert data.startswith(header) and len(data) == len(header) + len(pts) * 27 + len(faces) * 13
    assert np.array_equal(ply_io.read_ply(b)[0], host_mesh.vertices) and ply_io.read_ply_labels(b) == (None, None)
