"""GPU: the VOXEL_GRID reads and edits (get_voxels, get_voxels_in_bb, get_voxels_in_camera_frustrum, carve, remove_low_count_voxels,
size; k_vg_collect / k_vg_carve / k_vg_remove_low_count and the host-side query setup of hv_query.h) on planted grids
(tests/grid_query_cases.py), held to the numpy restatement (tests/grid_query_reference.py) run on the GPU grid's OWN dump() and to
the oracle fed the same batches.

Bar: bit for bit, as sorted row sets and whole dumps.  No tolerance and no allowance anywhere.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import grid_query_cases as qc
from tests import grid_query_reference as qr
from tests import planted_states as ps
from tests.test_gpu_voxel_grid import make_oracle

pytestmark = pytest.mark.gpu

HV_OK, HV_ERR_MODE = 0, -4
SENTINEL = np.float32(-12345.678)


def gpu_grid(voxel, bs):
    from pyslam_amd.volumetric import VoxelBlockGrid

    return VoxelBlockGrid(voxel, bs, max_blocks=1 << 10, max_points=1 << 14)


class GpuFront:
    """VoxelBlockGrid behind the step vocabulary of grid_query_cases, through its Python front ends: boxes alternate between a
    BoundingBox3D and a plain array, frusta between the scalar and the K-matrix constructor of CameraFrustrum; every query is asked
    twice and must return the same set.  device_image: carve gets its depth image as a torch CUDA tensor."""

    def __init__(self, grid, device_image=False):
        self.grid, self.device_image, self.calls = grid, device_image, 0

    def integrate(self, pts, cols):
        self.grid.integrate(pts, cols)

    def dump(self):
        return self.grid.dump()

    def size(self):
        return self.grid.size()

    def frustum(self, f):
        from pyslam_amd.volumetric import CameraFrustrum

        fx, fy, cx, cy = (float(x) for x in f["intr"])
        if self.calls % 2:
            K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
            return CameraFrustrum(K, f["W"], f["H"], f["T_cw"], f["dmax"], f["dmin"])
        return CameraFrustrum(fx, fy, cx, cy, f["W"], f["H"], f["T_cw"], depth_max=f["dmax"], depth_min=f["dmin"])

    def query(self, step):
        from pyslam_amd.volumetric import BoundingBox3D

        g, kind = self.grid, step[0]
        if kind == "all":
            return g.get_voxels(step[1])
        if kind == "box":
            bb = step[1]
            return g.get_voxels_in_bb(BoundingBox3D(bb[:3], bb[3:]) if self.calls % 2 else bb, min_count=step[2])
        return g.get_voxels_in_camera_frustrum(self.frustum(step[1]), min_count=step[2])

    def apply(self, step):
        self.calls += 1
        g, kind = self.grid, step[0]
        if kind in ("all", "box", "frustum"):
            a, b = self.query(step), self.query(step)
            first = qc.sorted_rows(a.points, a.colors)
            qc.assert_rows_equal(qc.sorted_rows(b.points, b.colors), first, "a repeated query returns another set")
            return a.points, a.colors
        if kind == "carve":
            depth = step[2]
            if self.device_image:
                import torch

                depth = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).cuda()
            return g.carve(self.frustum(step[1]), depth, step[3])
        if kind == "remove":
            return g.remove_low_count_voxels(step[1])
        return g.integrate(step[1], step[2])


def run(name, device_image=False):
    c = qc.case(name)
    gpu = GpuFront(gpu_grid(c["voxel"], c["bs"]), device_image)
    cpu = qc.OracleFront(make_oracle(c["voxel"], c["bs"]))
    assert qc.run_case(c, gpu, (cpu,)) == len(c["steps"])
    assert gpu.grid.dropped_points() == 0
    return gpu, cpu


@pytest.mark.parametrize("name", qc.CASE_NAMES)
def test_case_equals_restatement_and_oracle(name):
    """Planting, every query and every edit of the case: GPU == restatement on the GPU's own dump == oracle (see run_case)."""
    run(name)


@pytest.mark.parametrize("name", [n for n in qc.CASE_NAMES if n.startswith("carve_") or n == "frustum_generic_33x17"])
def test_carve_reads_a_torch_cuda_image(name):
    run(name, device_image=True)


def test_front_ends_and_no_op_carves():
    from pyslam_amd import _lib as L
    from pyslam_amd.volumetric import BoundingBox3D

    c = qc.case("carve_identity_0.015_8_thr0.03")
    g = gpu_grid(c["voxel"], c["bs"])
    for pts, cols in c["batches"]:
        g.integrate(pts, cols)
    before = g.dump()
    mask, pts, cols = qr.select_all(before, 1)
    assert g.size() == g.get_total_voxel_count() == int(mask.sum()) > 0
    rows = qc.sorted_rows(pts, cols)
    # get_points() and get_colors() are two queries, each in a row order of its own: compare them as separate sets
    assert np.array_equal(qc.bits(qc.sort_rows(g.get_points())[0]), qc.bits(qc.sort_rows(pts)[0]))
    assert np.array_equal(qc.bits(qc.sort_rows(g.get_colors())[0]), qc.bits(qc.sort_rows(cols)[0]))
    v = g.get_voxels()
    qc.assert_rows_equal(qc.sorted_rows(v.points, v.colors), rows)
    bb = np.array([-0.1, -0.05, 0.5, 0.12, 0.2, 1.2])
    want = qc.sorted_rows(*qr.select_box(before, bb, 1, c["voxel"], c["bs"])[1:])
    assert len(want) > 0
    for box in (bb, list(bb), BoundingBox3D(*bb), BoundingBox3D(bb[:3], bb[3:])):
        v = g.get_voxels_in_bb(box)
        qc.assert_rows_equal(qc.sorted_rows(v.points, v.colors), want)
    # carve: a depth image of the wrong size, an empty one and a null pointer are no-ops
    front = GpuFront(g)
    f, depth, thr = c["steps"][1][1:4]
    fr = front.frustum(f)
    g.carve(fr, np.ones((f["H"] + 1, f["W"]), np.float32), thr)
    g.carve(fr, np.ones((f["W"], f["H"]), np.float32), thr)
    g.carve(fr, np.ones((0, f["W"]), np.float32), thr)
    assert g._lib.hv_carve(g._h, L.ptr(fr.intr), fr.width, fr.height, L.ptr(fr.T_cw), fr.depth_max, fr.depth_min, None, float(thr),
                           L.HV_HOST) == HV_OK
    qc.assert_dumps_equal(g.dump(), before)
    g.carve(fr, depth.astype(np.float64), thr)  # a float64 image is converted, not misread
    qc.assert_dumps_equal(g.dump(), qr.carve(before, f["intr"], f["W"], f["H"], f["T_cw"], f["dmax"], f["dmin"], depth, thr, c["voxel"], c["bs"]))


# ---- the size-then-data protocol through the ABI ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def protocol_grid():
    c = qc.case("scattered_0.05_5")
    g = gpu_grid(c["voxel"], c["bs"])
    for pts, cols in c["batches"]:
        g.integrate(pts, cols)
    return c, g, g.dump()


def abi_call(g, step, points, colors, cap, n, loc):
    from pyslam_amd import _lib as L

    lib, kind = g._lib, step[0]
    p, c = L.ptr(points), L.ptr(colors)
    if kind == "all":
        return lib.hv_get_voxels(g._h, step[1], 0.0, p, c, cap, n, loc)
    if kind == "box":
        bb = np.ascontiguousarray(step[1], np.float64)
        return lib.hv_get_voxels_in_bb(g._h, L.ptr(bb), step[2], 0.0, p, c, cap, n, loc)
    f = step[1]
    T = np.ascontiguousarray(f["T_cw"], np.float64)
    return lib.hv_get_voxels_in_frustum(g._h, L.ptr(f["intr"]), f["W"], f["H"], L.ptr(T), f["dmax"], f["dmin"], step[2], 0.0, p, c, cap, n, loc)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", ["all", "box", "frustum"])
def test_size_then_data_protocol(kind, device):
    """Null outputs return n.  For cap in {0, 1, n-1, n, n+7} into buffers of cap + 16 sentinel rows: *n is the full count, exactly
    min(n, cap) rows are written, each a distinct member of the full set (which members is not specified), and the rows behind them
    keep the sentinel - also when the kernel writes straight into the caller's device buffer."""
    import torch
    from pyslam_amd import _lib as L

    c, g, before = protocol_grid()
    step = next(s for s in c["steps"] if s[0] == kind and s[-1] == 1)
    want = qr.apply_step(before, step, c["voxel"], c["bs"])
    full = {r.tobytes() for r in qc.sorted_rows(want[2], want[3])}
    n_full = len(full)
    assert n_full == len(want[2]) and n_full > 64  # rows are distinct; more than one wave appends
    n = ctypes.c_int64(-7)
    assert abi_call(g, step, None, None, 0, ctypes.byref(n), L.HV_HOST) == HV_OK and n.value == n_full
    n = ctypes.c_int64(-7)
    assert abi_call(g, step, None, None, 5, ctypes.byref(n), L.HV_DEVICE) == HV_OK and n.value == n_full
    for cap in (0, 1, n_full - 1, n_full, n_full + 7):
        pts, cols = (np.full((cap + 16, 3), SENTINEL, np.float32) for _ in range(2))
        if device:
            held = [torch.from_numpy(a).cuda() for a in (pts, cols)]
            torch.cuda.synchronize()
        else:
            held = [pts, cols]
        n = ctypes.c_int64(-7)
        assert abi_call(g, step, held[0], held[1], cap, ctypes.byref(n), L.HV_DEVICE if device else L.HV_HOST) == HV_OK
        assert n.value == n_full, (cap, n.value)
        if device:
            g.synchronize()
            pts, cols = (t.cpu().numpy() for t in held)
        m = min(n_full, cap)
        rows = np.hstack([pts, cols])
        written = [r.tobytes() for r in rows[:m]]
        assert len(set(written)) == m and set(written) <= full, cap
        assert (rows[m:].view(np.uint32) == SENTINEL.view(np.uint32)).all(), cap
        if m == n_full:
            assert set(written) == full
    qc.assert_dumps_equal(g.dump(), before)


def test_a_tsdf_handle_is_refused_and_nothing_is_written():
    from pyslam_amd import _lib as L
    from tests.test_gpu_tsdf_deintegrate import assert_bitwise
    from tests.test_gpu_tsdf_edges import volume

    states, _ = ps.two_walls(2, 1)
    vol = ps.plant(volume(ps.VOX, ps.TRUNC), states)
    before = vol.dump()
    for loc in (L.HV_HOST, L.HV_DEVICE):
        pts, cols = (np.full((32, 3), SENTINEL, np.float32) for _ in range(2))
        n = ctypes.c_int64(-7)
        host = loc == L.HV_HOST
        if host:
            held = [pts, cols]
        else:
            import torch

            held = [torch.from_numpy(a).cuda() for a in (pts, cols)]
            torch.cuda.synchronize()
        assert vol._lib.hv_get_voxels(vol._h, 0, 0.0, L.ptr(held[0]), L.ptr(held[1]), 32, ctypes.byref(n), loc) == HV_ERR_MODE
        assert n.value == -7
        got = held if host else [t.cpu().numpy() for t in held]
        assert all((a.view(np.uint32) == SENTINEL.view(np.uint32)).all() for a in got)
    bb = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    n = ctypes.c_int64(-7)
    assert vol._lib.hv_get_voxels_in_bb(vol._h, L.ptr(bb), 1, 0.0, None, None, 0, ctypes.byref(n), L.HV_HOST) == HV_ERR_MODE and n.value == -7
    assert vol._lib.hv_remove_low_count_voxels(vol._h, 2 ** 31 - 1) == HV_ERR_MODE
    assert b"voxel" in vol._lib.hv_last_error().lower()
    assert_bitwise(vol.dump(), before)
