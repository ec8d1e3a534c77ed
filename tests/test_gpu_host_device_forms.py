"""GPU: the entry points that take their arrays from the host (numpy) or from the device (torch CUDA tensors) compute the same bits
either way - the counterpart of test_gpu_binding_streams.py (the TSDF readers) for the writers and the image operations.

Images of 61x47 pixels (2867: no plane's byte count is a multiple of 256, the alignment of the staged pieces) and 1001 points.  Each
case runs once with numpy arrays and once with device tensors of the same values - through the Python binding where that accepts
tensors, else through the C library with the tensors' addresses - and the results are compared as bytes: the outputs, or the dumps and
get_voxels() of two volumes built either way.  Two cases run again after a call with a four times larger image, i.e. from a staging
buffer that has been freed and reallocated in between."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 61, 47
FX = FY = 58.0
CX, CY = 30.0, 23.0
N = 1001
VOX = 0.05


def plane_depth(w, h, scale=1.0):
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = 1.0 / (1.0 - 0.3 * (u / scale - CX) / FX) + 0.002 * ((u + 2 * v) % 7)
    d[(u.astype(int) * 3 + v.astype(int)) % 41 == 0] = 0.0  # some invalid pixels
    return d.astype(np.float32)


class Data:
    def __init__(self):
        rng = np.random.default_rng(11)
        u, v = np.meshgrid(np.arange(W), np.arange(H))
        self.depth = plane_depth(W, H)
        self.rgb = np.stack([(4 * u) % 256, (5 * v) % 256, (u + v) % 256], axis=-1).astype(np.uint8)
        self.cls = ((u // 9 + v // 11) % 5).astype(np.int32)
        self.inst = ((u // 13) * 4 + v // 12 + 1).astype(np.int32)
        self.inst[::5, ::7] = -1
        self.obj = (self.inst + 100).astype(np.int32)
        self.T = np.eye(4)
        self.T[0, 3] = 0.03
        x, y = rng.uniform(-0.5, 0.5, N), rng.uniform(-0.4, 0.4, N)
        self.points = np.stack([x, y, 1.0 + 0.3 * x], axis=1).astype(np.float32)
        self.points64 = self.points.astype(np.float64) + 1e-9
        self.colors = rng.integers(0, 256, (N, 3), dtype=np.uint8)
        self.pcls = rng.integers(0, 5, N, dtype=np.int32)
        self.pinst = rng.integers(1, 9, N, dtype=np.int32)
        self.pdepth = rng.uniform(0.5, 3.0, N).astype(np.float32)
        self.big_depth = plane_depth(2 * W, 2 * H, 2.0)
        self.map_x = (u + 0.37 * np.sin(v / 5.0) + 0.5).astype(np.float32)
        self.map_y = (v + 0.41 * np.cos(u / 7.0) - 0.25).astype(np.float32)


@pytest.fixture(scope="module")
def data():
    return Data()


def dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def place(arrays, device):
    import torch

    out = [dev(a) if device else (None if a is None else np.ascontiguousarray(a)) for a in arrays]
    if device:
        torch.cuda.synchronize()  # (the direct library calls below are not ordered against torch's stream by a binding)
    return out


def same_bytes(a, b, what):
    import torch

    a, b = (x.cpu().numpy() if torch.is_tensor(x) else np.ascontiguousarray(x) for x in (a, b))
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), f"{what}: the device form differs from the host form"


def sorted_rows(*cols):
    """get_voxels() lists the voxels in pool order, which is not fixed: the rows sorted by position."""
    table = np.concatenate([np.asarray(c, np.float64).reshape(len(cols[0]), -1) for c in cols], axis=1)
    return table[np.lexsort(table.T[::-1])]


def same_grid(a, b, what):
    assert a.num_blocks() == b.num_blocks() > 0, what
    for i, (x, y) in enumerate(zip(a.dump(), b.dump())):
        same_bytes(x, y, f"{what}: dump()[{i}]")
    va, vb = a.get_voxels(), b.get_voxels()
    same_bytes(sorted_rows(va.points, va.colors), sorted_rows(vb.points, vb.colors), f"{what}: get_voxels()")


def same_semantic(a, b, what):
    assert a.num_blocks() == b.num_blocks() > 0, what
    for i, (x, y) in enumerate(zip(a.dump2(), b.dump2())):
        same_bytes(x, y, f"{what}: dump2()[{i}]")
    va, vb = a.get_voxels(1, -1.0), b.get_voxels(1, -1.0)
    rows = [sorted_rows(v.points, v.colors, v.class_ids, v.object_ids, v.confidences) for v in (va, vb)]
    assert len(rows[0]) > 100, what
    same_bytes(rows[0], rows[1], f"{what}: get_voxels()")


def both(make, act, compare, what):
    """Two volumes, act(volume, device) on the host and on the device, compared."""
    vols = []
    for device in (False, True):
        vol = make()
        act(vol, device)
        vol.synchronize()
        vols.append(vol)
    compare(vols[0], vols[1], what)
    for vol in vols:
        vol.close()


def make_grid():
    from pyslam_amd.volumetric import VoxelBlockGrid

    return VoxelBlockGrid(VOX, 8, max_blocks=1 << 10, max_points=1 << 14)


def make_semantic(kind="VoxelBlockSemanticGrid"):
    import pyslam_amd.volumetric_semantic as vs

    return getattr(vs, kind)(VOX, 8, max_blocks=1 << 10, max_points=1 << 14)


@pytest.mark.parametrize("wide", (False, True))
def test_voxel_block_grid_points(data, wide):
    def act(vol, device):
        pts, cols = place((data.points64 if wide else data.points, data.colors), device)
        vol.integrate(pts, cols)

    both(make_grid, act, same_grid, "VoxelBlockGrid.integrate")


def test_voxel_block_grid_rgbd(data):
    def act(vol, device):
        depth, rgb = place((data.depth, data.rgb), device)
        vol.integrate_rgbd(depth, rgb, FX, FY, CX, CY, data.T, max_depth=5.0)

    both(make_grid, act, same_grid, "VoxelBlockGrid.integrate_rgbd")


@pytest.mark.parametrize("full", (True, False))
@pytest.mark.parametrize("kind", ("VoxelBlockSemanticGrid", "VoxelBlockSemanticProbabilisticGrid"))
def test_integrate_points_semantic(data, kind, full):
    """hv_integrate_points_semantic with all five arrays, and with colours, instance ids and depths absent."""
    from pyslam_amd import _lib as L

    def act(vol, device):
        arrays = (data.points, data.colors, data.pcls, data.pinst, data.pdepth) if full else (data.points, None, data.pcls, None, None)
        pts, cols, cls, inst, dep = place(arrays, device)
        L.check(vol._lib.hv_integrate_points_semantic(vol._h, L.ptr(pts), 0, N, L.ptr(cols), L.HV_COLOR_U8 if full else L.HV_COLOR_NONE, L.ptr(cls),
                                                      L.ptr(inst), L.ptr(dep), L.HV_DEVICE if device else L.HV_HOST))
        vol.synchronize()  # (the operands are dropped on return)

    both(lambda: make_semantic(kind), act, same_semantic, f"hv_integrate_points_semantic({kind}, full={full})")


@pytest.mark.parametrize("with_objects", (True, False))
def test_integrate_rgbd_semantic(data, with_objects):
    def act(vol, device):
        depth, rgb, cls, obj = place((data.depth, data.rgb, data.cls, data.obj if with_objects else None), device)
        vol.integrate_rgbd(depth, rgb, FX, FY, CX, CY, data.T, cls, obj, max_depth=5.0)

    both(make_semantic, act, same_semantic, f"hv_integrate_rgbd_semantic(objects={with_objects})")


def frustum(data):
    from pyslam_amd.volumetric import CameraFrustrum

    return CameraFrustrum(FX, FY, CX, CY, W, H, data.T, 5.0, 0.1)


@pytest.mark.parametrize("with_depth", (True, False))
def test_assign_object_ids(data, with_depth):
    """The association (hv_assoc_vote stages the images), then both remaps: with the map still on the device
    (hv_remap_instance_ids_last) and with it as a dict (hv_remap_instance_ids)."""
    import pyslam_amd.volumetric_semantic as vs

    results = []

    def act(vol, device):
        vol.integrate_rgbd(data.depth, data.rgb, FX, FY, CX, CY, data.T, data.cls, data.obj, max_depth=5.0)
        vs.set_next_object_id(500)  # (the counter is the process's: both forms hand out the same ids)
        cls, inst, depth = place((data.cls, data.inst, data.depth if with_depth else None), device)
        id_map = vol.assign_object_ids_to_instance_ids(frustum(data), cls, inst, depth, depth_threshold=0.1, min_votes=1)
        last = vol.remap_instance_ids(inst, id_map)  # (the map has not been read: it is used where it lies)
        as_dict = dict(id_map)
        again = vol.remap_instance_ids(inst, as_dict)
        results.append((as_dict, last, again))

    both(make_semantic, act, same_semantic, f"assign_object_ids_to_instance_ids(depth={with_depth})")
    (map_h, last_h, again_h), (map_d, last_d, again_d) = results
    assert map_h == map_d and len(set(map_h.values())) >= 4
    same_bytes(last_h, last_d, "hv_remap_instance_ids_last")
    same_bytes(again_h, again_d, "hv_remap_instance_ids")
    same_bytes(last_h, again_h, "the two remaps")
    assert (last_h != data.inst).any()


def grown(vol, data):
    """A call whose image is four times larger: the staging buffer is freed and reallocated."""
    vol.filter_shadow_points(data.big_depth)


@pytest.mark.parametrize("case", ("u8x3_nearest", "f32_linear"))
def test_remap(data, case):
    img = data.rgb if case == "u8x3_nearest" else data.depth
    linear = case == "f32_linear"
    vol = make_grid()
    host = vol.remap(img, data.map_x, data.map_y, linear)
    assert (host != img).any()
    same_bytes(host, vol.remap(dev(img), data.map_x, data.map_y, linear), f"hv_remap({case})")
    grown(vol, data)
    same_bytes(host, vol.remap(img, data.map_x, data.map_y, linear), f"hv_remap({case}) after the buffer grew")
    same_bytes(host, vol.remap(dev(img), data.map_x, data.map_y, linear), f"hv_remap({case}) on the device after the buffer grew")
    vol.close()


def test_filter_shadow_points(data):
    vol = make_grid()
    host = vol.filter_shadow_points(data.depth)
    assert (host != data.depth).any() and (host == data.depth).any()
    same_bytes(host, vol.filter_shadow_points(dev(data.depth)), "hv_filter_shadow_points")
    grown(vol, data)
    same_bytes(host, vol.filter_shadow_points(data.depth), "hv_filter_shadow_points after the buffer grew")
    same_bytes(host, vol.filter_shadow_points(dev(data.depth)), "hv_filter_shadow_points on the device after the buffer grew")
    vol.close()


def test_tsdf_import_numerators(data):
    from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume

    def make():
        return ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)

    src = make()
    depth = np.where(data.depth > 0, data.depth, 1.0).astype(np.float32)
    src.integrate(RGBDImage.create_from_color_and_depth(data.rgb, depth, 1.0, 4.0, False), PinholeCameraIntrinsic(W, H, FX, FY, CX, CY), data.T)
    keys = src.unit_keys()
    payload = src.export_numerators(keys)
    assert len(keys) > 10 and np.count_nonzero(payload) > 1000
    same_bytes(payload, src.export_numerators(keys, out=dev(np.zeros_like(payload))), "hv_tsdf_export_numerators")

    def act(vol, device):
        (p,) = place((payload,), device)
        vol.import_numerators(keys, p)

    def compare(a, b, what):
        assert a.num_blocks() == b.num_blocks() == len(keys)
        for i, (x, y) in enumerate(zip(a.dump(), b.dump())):
            same_bytes(x, y, f"{what}: dump()[{i}]")
        same_bytes(a.dump()[0], src.dump()[0], f"{what}: the unit keys against the source's")

    both(make, act, compare, "hv_tsdf_import_numerators")
    src.close()
