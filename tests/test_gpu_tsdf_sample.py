"""GPU: ScalableTSDFVolume.sample_points (hv_tsdf_sample_points, hv_sample.hip) on planted voxel states (tests/planted_states.py,
tests/sample_cases.py), held to the numpy restatement (tests/sample_reference.py) run on the planted volume's OWN dump().

Bar: every output equal to the restatement bit for bit off the fragile points, whose share is capped at 1e-4
(tests/test_sample_reference_cpu.py asserts it is 0.0 for every point set used here); the linear field within the two bounds that
file derives.  Voxel 0.02, sdf_trunc 0.08, at most ~30 units per case.
"""
import functools
import itertools

import numpy as np
import pytest

from tests import planted_states as ps
from tests import sample_cases as sc
from tests import sample_reference as sr
from tests.test_gpu_tsdf_deintegrate import assert_bitwise
from tests.test_gpu_tsdf_edges import volume

pytestmark = pytest.mark.gpu

VOX, TRUNC = sc.VOX, sc.TRUNC
OUTPUTS = ("sdf", "gradient", "color", "weight", "status")
FRAGILE_SHARE = 1e-4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def planted(states):
    vol = volume(VOX, TRUNC)
    if len(states[0]):
        ps.plant(vol, states)
    assert_bitwise(vol.dump(), ps.as_dump(states))
    return vol


@functools.lru_cache(maxsize=None)
def cluster():
    vol = planted(sc.cluster_states())
    return vol, vol.dump()


@functools.lru_cache(maxsize=None)
def cluster_reference(n, threshold, f32=False):
    p = sc.cluster_points(n)
    return sr.sample_points(cluster()[1], VOX, TRUNC, p.astype(np.float32) if f32 else p, threshold)


def assert_equals_restatement(got, ref, label, names=OUTPUTS):
    """got: {name: array}; equal to the restatement bit for bit off the fragile points (share <= FRAGILE_SHARE)."""
    fragile = ref["fragile"]
    assert fragile.mean() <= FRAGILE_SHARE if len(fragile) else True, (label, fragile.mean())
    keep = ~fragile
    for name in names:
        g, r = np.asarray(got[name]), ref[name]
        assert g.shape == r.shape and g.dtype == r.dtype, (label, name, g.shape, g.dtype)
        assert np.array_equal(bits(g[keep]), bits(r[keep])), (label, name, int((g[keep] != r[keep]).sum()))


def as_dict(res):
    return {name: getattr(res, name) for name in OUTPUTS}


def call_abi(vol, points, threshold, want):
    """hv_tsdf_sample_points with exactly the outputs `want`; the others are NULL.  Buffers start as 0xAB bytes."""
    from pyslam_amd import _lib as L

    n = len(points)
    shapes = {"sdf": ((n,), np.float32), "gradient": ((n, 3), np.float32), "color": ((n, 3), np.float32), "weight": ((n,), np.float32),
              "status": ((n,), np.uint8)}
    out = {name: np.full(int(np.prod(shapes[name][0])) * np.dtype(shapes[name][1]).itemsize, 0xAB, np.uint8).view(shapes[name][1]).reshape(shapes[name][0])
           for name in want}
    p = np.ascontiguousarray(points)
    L.check(vol._lib.hv_tsdf_sample_points(vol._h, L.ptr(p), L.HV_F64 if p.dtype == np.float64 else L.HV_F32, n, float(threshold),
                                           *(L.ptr(out.get(name)) for name in OUTPUTS), L.HV_HOST))
    return out


@pytest.mark.parametrize("n", sc.POINT_COUNTS)
def test_sparse_cluster_equals_the_restatement(n):
    """Missing units, unobserved voxels, one-voxel units and unit borders on every side: every status occurs; block counts of 1,
    63, 64, 65 and 4097 points (a partial wave, a full one, one lane of a second, many workgroups)."""
    vol, _ = cluster()
    p = sc.cluster_points(n)
    ref = cluster_reference(n, 0.0)
    res = vol.sample_points(p, gradient=True, color=True)
    assert all(isinstance(getattr(res, name), np.ndarray) for name in OUTPUTS)
    assert_equals_restatement(as_dict(res), ref, n)
    if n == 4097:
        assert set(np.unique(res.status)) == {sr.OUTSIDE, sr.UNOBSERVED, sr.NEAREST, sr.TRILINEAR}
    # the same values as float32: equal to the float64 call on the widened values, and to the restatement
    p32 = p.astype(np.float32)
    a, b = vol.sample_points(p32, gradient=True, color=True), vol.sample_points(p32.astype(np.float64), gradient=True, color=True)
    for name in OUTPUTS:
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert_equals_restatement(as_dict(a), cluster_reference(n, 0.0, True), (n, "float32"))
    # outputs not asked for are None, the others unchanged
    plain = vol.sample_points(p, gradient=False, color=False)
    assert plain.gradient is None and plain.color is None
    assert_equals_restatement(as_dict(plain), ref, (n, "plain"), ("sdf", "weight", "status"))


@pytest.mark.parametrize("n", sc.POINT_COUNTS)
def test_every_subset_of_outputs(n):
    """Any output pointer may be NULL: every subset (the empty one included) gives the restatement's values in what it asks for."""
    vol, _ = cluster()
    p = sc.cluster_points(n)
    ref = cluster_reference(n, 0.0)
    for k in range(len(OUTPUTS) + 1):
        for want in itertools.combinations(OUTPUTS, k):
            assert_equals_restatement(call_abi(vol, p, 0.0, want), ref, (n, want), want)


@pytest.mark.parametrize("threshold", sc.THRESHOLDS)
def test_weight_thresholds(threshold):
    vol, _ = cluster()
    p = sc.cluster_points(4097)
    ref = cluster_reference(4097, threshold)
    res = vol.sample_points(p, weight_threshold=threshold, gradient=True, color=True)
    assert_equals_restatement(as_dict(res), ref, threshold)
    observed = res.status >= sr.NEAREST
    assert (res.weight[observed] > threshold).all() and not res.weight[~observed].any()
    if threshold > 0:
        low = cluster_reference(4097, 0.0)["status"]
        assert (res.status <= low).all() and (res.status < low).sum() > 100


def test_hand_made_cases():
    vol = planted(sc.hand_states())
    points, _ = sc.hand_points()
    res = vol.sample_points(points, gradient=True, color=True)
    for (name, _, want), got in zip(sc.HAND_POINTS, res.status):
        assert got == want, name
    assert_equals_restatement(as_dict(res), sr.sample_points(vol.dump(), VOX, TRUNC, points), "hand")
    # the empty volume: all OUTSIDE, every output 0
    empty = volume(VOX, TRUNC)
    res = empty.sample_points(points, gradient=True, color=True)
    for name in OUTPUTS:
        assert not np.asarray(getattr(res, name)).any(), name
    # n = 0
    res = vol.sample_points(np.zeros((0, 3)), gradient=True, color=True)
    assert [getattr(res, name).shape for name in OUTPUTS] == [(0,), (0, 3), (0, 3), (0,), (0,)]
    from pyslam_amd import _lib as L

    assert vol._lib.hv_tsdf_sample_points(vol._h, None, L.HV_F64, 0, 0.0, None, None, None, None, None, L.HV_HOST) == 0


def test_linear_field():
    vol = planted(sc.linear_states())
    p = sc.linear_points()
    res = vol.sample_points(p, gradient=True)
    assert (res.status == sr.TRILINEAR).all()
    err_sdf = np.abs(res.sdf.astype(np.float64) - (p[:, 0] - sc.X0)).max()
    err_grad = np.abs(res.gradient.astype(np.float64) - [1.0, 0.0, 0.0]).max()
    print(f"linear field: max |sdf error| {err_sdf:.3e} (bound {sc.LINEAR_SDF_BOUND:.3e}), max |gradient error| {err_grad:.3e} "
          f"(bound {sc.LINEAR_GRADIENT_BOUND:.3e})")
    assert err_sdf <= sc.LINEAR_SDF_BOUND
    assert err_grad <= sc.LINEAR_GRADIENT_BOUND
    assert_equals_restatement({"sdf": res.sdf, "gradient": res.gradient}, sr.sample_points(vol.dump(), VOX, TRUNC, p), "linear", ("sdf", "gradient"))


def test_queries_only_read():
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    vol = planted(sc.cluster_states())
    mesh = vol.extract_triangle_mesh()
    before = (vol.dump(), vol.dirty_keys(), vol.touched_keys(), vol.num_blocks())
    p = sc.cluster_points(4097)
    vol.sample_points(p, gradient=True, color=True)
    vol.sample_points(p.astype(np.float32), weight_threshold=3.0)
    H, W = 70, 9
    vol.check_frame(sc.wall_depth(H, W, "float32", 1.0), PinholeCameraIntrinsic(W, H, *sc.intrinsics(H, W)), ps.camera_pose(2, 1))
    assert_bitwise(vol.dump(), before[0])
    assert np.array_equal(vol.dirty_keys(), before[1]) and np.array_equal(vol.touched_keys(), before[2]) and vol.num_blocks() == before[3]
    again = vol.extract_triangle_mesh()
    for name in ("vertices", "triangles", "vertex_colors"):
        a, b = np.asarray(getattr(again, name)), np.asarray(getattr(mesh, name))
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), name


def test_two_calls_and_another_pool_order_are_bitwise_equal():
    vol, _ = cluster()
    p = sc.cluster_points(4097)
    first = as_dict(vol.sample_points(p, gradient=True, color=True))
    second = as_dict(vol.sample_points(p, gradient=True, color=True))
    # the same map unpacked into a fresh volume, and planted with its units in reverse key order: other pool orders
    unpacked = volume(VOX, TRUNC)
    unpacked.unpack(vol.pack())
    states = sc.cluster_states()
    backwards = volume(VOX, TRUNC)
    ps.plant(backwards, tuple(np.ascontiguousarray(x[::-1]) for x in states))
    assert_bitwise(backwards.dump(), vol.dump())
    for other in (second, as_dict(unpacked.sample_points(p, gradient=True, color=True)), as_dict(backwards.sample_points(p, gradient=True, color=True))):
        for name in OUTPUTS:
            assert np.array_equal(bits(first[name]), bits(other[name])), name


def test_torch_cuda_in_gives_torch_cuda_out():
    import torch

    vol, _ = cluster()
    p = sc.cluster_points(4097)
    host = vol.sample_points(p, gradient=True, color=True)
    for dtype in (torch.float64, torch.float32):
        t = torch.from_numpy(p).to(dtype).cuda()
        dev = vol.sample_points(t, gradient=True, color=True)
        want = host if dtype == torch.float64 else vol.sample_points(p.astype(np.float32), gradient=True, color=True)
        for name in OUTPUTS:
            x = getattr(dev, name)
            assert isinstance(x, torch.Tensor) and x.is_cuda, name
            assert np.array_equal(bits(x.cpu().numpy()), bits(getattr(want, name))), (dtype, name)
    # a torch tensor on the host is host memory; device= overrides where the results go
    cpu = vol.sample_points(torch.from_numpy(p), gradient=True, color=True)
    forced = vol.sample_points(p, gradient=True, color=True, device=True)
    back = vol.sample_points(torch.from_numpy(p).cuda(), gradient=True, color=True, device=False)
    for name in OUTPUTS:
        assert isinstance(getattr(cpu, name), np.ndarray) and isinstance(getattr(back, name), np.ndarray) and getattr(forced, name).is_cuda
        assert np.array_equal(bits(getattr(cpu, name)), bits(getattr(host, name)))
        assert np.array_equal(bits(getattr(back, name)), bits(getattr(host, name)))
        assert np.array_equal(bits(getattr(forced, name).cpu().numpy()), bits(getattr(host, name)))


def test_errors_leave_the_outputs_untouched():
    from pyslam_amd import _lib as L
    from pyslam_amd.volumetric import ScalableTSDFVolume, VoxelBlockGrid

    vol, _ = cluster()
    p = sc.cluster_points(65)
    sdf = np.full(65, 7.5, np.float32)
    status = np.full(65, 9, np.uint8)

    def refused(v, points=p, dtype=L.HV_F64, n=65, threshold=0.0, code=-1):
        rc = v._lib.hv_tsdf_sample_points(v._h, L.ptr(points), dtype, n, threshold, L.ptr(sdf), None, None, None, L.ptr(status), L.HV_HOST)
        assert rc != 0 and (code is None or rc == code), rc
        assert (sdf == 7.5).all() and (status == 9).all()

    HV_ERR_INVALID, HV_ERR_MODE = -1, -4
    grid = VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12)
    assert not hasattr(grid, "sample_points")
    refused(grid, code=HV_ERR_MODE)
    with pytest.raises(L.HipVolError, match="TSDF"):
        ScalableTSDFVolume.sample_points(grid, p)
    owner = volume(VOX, TRUNC)
    owner.set_owner(0, 2)
    refused(owner, code=HV_ERR_MODE)
    with pytest.raises(L.HipVolError, match="owner-sharded"):
        owner.sample_points(p)
    tiled = volume(VOX, TRUNC)
    tiled.set_tile(0, 0, 80, 120)
    refused(tiled, code=HV_ERR_MODE)
    with pytest.raises(L.HipVolError, match="tile-sharded"):
        tiled.sample_points(p)
    for threshold in (-1.0, float("nan"), float("inf")):
        refused(vol, threshold=threshold, code=HV_ERR_INVALID)
        with pytest.raises(L.HipVolError, match="weight_threshold"):
            vol.sample_points(p, weight_threshold=threshold)
    refused(vol, n=-1, code=HV_ERR_INVALID)
    refused(vol, points=None, code=HV_ERR_INVALID)
    refused(vol, dtype=2, code=HV_ERR_INVALID)
    for bad in (np.zeros((5, 2)), np.zeros((5, 3), np.int32), np.zeros(6), np.zeros((5, 3), np.float16)):
        with pytest.raises(ValueError):
            vol.sample_points(bad)
