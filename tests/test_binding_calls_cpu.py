"""What the Python binding sends over the C ABI, pinned call for call against a recording stand-in for the library
(tests/recording_lib.py; no GPU): for every public method of ScalableTSDFVolume, VoxelBlockGrid and VoxelBlockSemanticGrid with host
operands - numpy arrays and host torch tensors - the function name, every scalar argument (value and Python type), every pointer
(the operand's own address, or that of the array the method returns), dtype and shape of every result, every stats field under its
own name (the stand-in writes a distinct prime into each), one call for a zero count, no call for zero frames, and every refusal's
exception type and message before any library call.  test_binding_covers_every_public_method keeps the list complete."""
import ctypes

import numpy as np
import pytest

from pyslam_amd import _lib as L
from pyslam_amd import volumetric as V
from pyslam_amd import volumetric_semantic as S
from tests.recording_lib import HANDLE, STATS_PRIMES, addr, ref, volume

IH, IW = 6, 8
K = V.PinholeCameraIntrinsic(IW, IH, 8.0, 7.0, 3.3, 4.1)
UNSUPPORTED = "Unsupported image format"
I64 = ctypes.c_int64
ANY = ("p", "any")  # a pointer to an operand the binding builds for the call alone
SKIP = ("skip",)  # a pointer that may be anything (an empty operand)
NO_HANDLE = ("hv_host_register", "hv_host_unregister")  # the calls that take no volume
HND = ("p", HANDLE)
COVERED = set()


def covers(*names):
    """Decorator: the test exercises these public methods (test_binding_covers_every_public_method keeps the list complete)."""
    COVERED.update(names)
    return lambda test: test


def P(a):
    return ("p", addr(a))


def REF(cls):
    return ("ref", cls.__name__)


def norm(a):
    if a is None or isinstance(a, tuple):
        return a
    if isinstance(a, (ctypes.c_void_p, ctypes._Pointer)):
        return ("p", addr(a))
    if hasattr(a, "_obj"):
        return ("ref", type(a._obj).__name__)
    if isinstance(a, ctypes.Array):
        return ("array", len(a))
    return (type(a).__name__, a)


def expect(vol, *calls):
    """The calls recorded since the last expect(): (name, arguments after the handle), compared one by one."""
    got, vol._lib.calls = vol._lib.calls, []
    assert [name for name, _ in got] == [c[0] for c in calls]
    for (name, args), want in zip(got, calls):
        have, want = [norm(a) for a in args], [HND] * (name not in NO_HANDLE) + [norm(a) for a in want[1:]]
        assert len(have) == len(want), (name, have, want)
        for i, (h, w) in enumerate(zip(have, want)):
            ok = True if w == SKIP else (h is not None and h[0] == "p" and bool(h[1])) if w == ANY else h == w
            assert ok, f"{name} argument {i}: {h} != {w}"
    return got


def refused(vol, exc, message, fn, *args, **kw):
    with pytest.raises(exc) as e:
        fn(*args, **kw)
    assert message in str(e.value), str(e.value)
    assert type(e.value) is exc and vol._lib.calls == []


def primes(result, struct):
    """Every field of the stats struct arrived under its own name."""
    for name, value in STATS_PRIMES[struct].items():
        assert getattr(result, name) == value and type(getattr(result, name)) is int, name


def shaped(a, shape, dtype):
    assert tuple(a.shape) == tuple(shape) and np.dtype(a.dtype) == np.dtype(dtype) and isinstance(a, np.ndarray), (a.shape, a.dtype)


@pytest.fixture(params=["numpy", "torch"])
def host(request):
    """numpy array -> the host operand of this run: itself, or a torch tensor of the same memory."""
    if request.param == "numpy":
        return lambda a: a
    torch = pytest.importorskip("torch")
    return torch.from_numpy


def frames(F=None, u16=False, seed=0):
    rng = np.random.default_rng(seed)
    lead = () if F is None else (F,)
    depth = (0.5 + 3.0 * rng.random(lead + (IH, IW))).astype(np.float32)
    return (np.rint(depth * 1000).astype(np.uint16) if u16 else depth), rng.integers(0, 256, lead + (IH, IW, 3)).astype(np.uint8)


def pose(i=0):
    T = np.eye(4)
    T[:3, 3] = (0.1 * i, 0.2, 0.3)
    return T


def tsdf():
    return volume(V.ScalableTSDFVolume, voxel_length=0.02, sdf_trunc=0.08, res=16)


def frustum():
    return V.CameraFrustrum(8.0, 7.0, 3.3, 4.1, IW, IH, pose(1), 5.0, 0.1)


# ---- ScalableTSDFVolume: posed frames -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("u16", [False, True])
@covers("integrate", "deintegrate")
def test_tsdf_single_frames(host, u16):
    depth, color = frames(u16=u16)
    d, c = host(depth), host(color)
    kind = L.HV_DEPTH_U16 if u16 else L.HV_DEPTH_F32
    vol = tsdf()
    for name in ("hv_tsdf_integrate", "hv_tsdf_deintegrate"):
        vol._lib.script(name, peek={6: (np.float64, 4), 7: (np.float64, 16)})
    assert vol.integrate(V.RGBDImage(c, d, 1000.0, 3.5), K, pose(1)) is None
    expect(vol, ("hv_tsdf_integrate", P(d), kind, P(c), IH, IW, ANY, ANY, 1000.0, 3.5, L.HV_HOST))
    assert vol._inflight[0] is None and vol._inflight[1] is d and vol._inflight[2] is c
    st = vol.deintegrate(V.RGBDImage(c, d, 1000.0, 3.5), K, pose(2))
    expect(vol, ("hv_tsdf_deintegrate", P(d), kind, P(c), IH, IW, ANY, ANY, 1000.0, 3.5, L.HV_HOST, REF(L.HvDeintegrateStats)))
    assert type(st) is V.DeintegrationStats
    primes(st, L.HvDeintegrateStats)
    assert vol._inflight[0][0] is d and vol._inflight[0][1] is c and vol._inflight_prev[0] is d
    for seen, T in zip(vol._lib.peeked, (pose(1), pose(2))):
        np.testing.assert_array_equal(seen[6], K.as_array())
        np.testing.assert_array_equal(seen[7], T.reshape(-1))
    for fn in (vol.integrate, vol.deintegrate):
        refused(vol, RuntimeError, "T_cw must be a 4x4 matrix", fn, V.RGBDImage(c, d, 1.0, 4.0), K, np.eye(3))
        refused(vol, RuntimeError, UNSUPPORTED, fn, V.RGBDImage(host(color[:, :-1].copy()), d, 1.0, 4.0), K, np.eye(4))
        refused(vol, RuntimeError, UNSUPPORTED, fn, V.RGBDImage(c, d, 1.0, 4.0), V.PinholeCameraIntrinsic(IW + 1, IH, 1, 1, 0, 0), np.eye(4))


@covers("integrate_batch", "deintegrate_batch", "reintegrate_batch")
def test_tsdf_batches(host):
    depth, color = frames(3)
    d, c = host(depth), host(color)
    To, Tn = np.stack([pose(i) for i in range(3)]), np.stack([pose(i + 5) for i in range(3)])
    vol = tsdf()
    for name in ("hv_tsdf_integrate_batch", "hv_tsdf_deintegrate_batch"):
        vol._lib.script(name, peek={7: (np.float64, 4), 8: (np.float64, 48)})
    vol._lib.script("hv_tsdf_reintegrate_batch", peek={7: (np.float64, 4), 8: (np.float64, 48), 9: (np.float64, 48)})
    head = (P(d), L.HV_DEPTH_F32, P(c), 3, IH, IW, ANY, ANY)
    assert vol.integrate_batch(d, c, K, To, depth_scale=2, depth_trunc=5) is None
    expect(vol, ("hv_tsdf_integrate_batch",) + head + (2.0, 5.0, L.HV_HOST))
    assert vol._inflight[1] is d and vol._inflight[2] is c
    st = vol.deintegrate_batch(d, c, K, To.reshape(3, 16), depth_scale=2, depth_trunc=5)
    expect(vol, ("hv_tsdf_deintegrate_batch",) + head + (2.0, 5.0, L.HV_HOST, REF(L.HvDeintegrateStats)))
    primes(st, L.HvDeintegrateStats)
    st = vol.reintegrate_batch(d, c, K, To, Tn)
    expect(vol, ("hv_tsdf_reintegrate_batch",) + head + (ANY, 1.0, 4.0, L.HV_HOST, REF(L.HvDeintegrateStats)))
    primes(st, L.HvDeintegrateStats)
    assert type(st) is V.DeintegrationStats
    for seen in vol._lib.peeked:
        np.testing.assert_array_equal(seen[7], K.as_array())
        np.testing.assert_array_equal(seen[8], To.reshape(-1))
    np.testing.assert_array_equal(vol._lib.peeked[2][9], Tn.reshape(-1))
    # zero frames: no call, the empty answer
    d0, c0 = host(depth[:0]), host(color[:0])
    assert vol.integrate_batch(d0, c0, K, To[:0]) is None
    assert vol.deintegrate_batch(d0, c0, K, To[:0]) == V.DeintegrationStats()
    assert vol.reintegrate_batch(d0, c0, K, To[:0], Tn[:0]) == V.DeintegrationStats()
    expect(vol)
    for fn, extra in ((vol.integrate_batch, ()), (vol.deintegrate_batch, ()), (vol.reintegrate_batch, (Tn,))):
        refused(vol, RuntimeError, UNSUPPORTED, fn, d, c, K, To[:2], *extra)
        refused(vol, RuntimeError, UNSUPPORTED, fn, d, c, K, np.zeros((4, 12)), *extra)
        refused(vol, RuntimeError, UNSUPPORTED, fn, d, host(color[:2]), K, To, *extra)
        refused(vol, RuntimeError, UNSUPPORTED, fn, host(depth[0]), host(color[0]), K, To[0], *(e[0] for e in extra))
    refused(vol, RuntimeError, UNSUPPORTED, vol.reintegrate_batch, d, c, K, To, Tn[:2])


@covers("integrate_frames")
def test_tsdf_integrate_frames(host):
    depth, color = frames(3)
    T = np.stack([pose(i) for i in range(3)])
    vol = tsdf()
    vol._lib.script("hv_tsdf_integrate_frames", peek={7: (np.float64, 4), 8: (np.float64, 48)})
    ds, cs = [host(x) for x in depth], [host(x) for x in color]
    assert vol.integrate_frames(ds, cs, K, T, depth_scale=2, depth_trunc=5) is None
    (_, args), = expect(vol, ("hv_tsdf_integrate_frames", ("array", 3), L.HV_DEPTH_F32, ("array", 3), 3, IH, IW, ANY, ANY, 2.0, 5.0))
    assert [args[1][f] for f in range(3)] == [addr(x) for x in ds] and [args[3][f] for f in range(3)] == [addr(x) for x in cs]
    np.testing.assert_array_equal(vol._lib.peeked[0][8], T.reshape(-1))
    assert vol.integrate_frames([], [], K, T[:0]) is None
    expect(vol)
    refused(vol, RuntimeError, UNSUPPORTED, vol.integrate_frames, ds, cs[:2], K, T)
    refused(vol, RuntimeError, UNSUPPORTED, vol.integrate_frames, ds, cs, K, T[:2])
    refused(vol, RuntimeError, UNSUPPORTED, vol.integrate_frames, [ds[0], host(depth[1].astype(np.uint16))], cs[:2], K, T[:2])


# ---- ScalableTSDFVolume: map operations ---------------------------------------------------------------------------------------
@covers("prune", "integrate_volume", "register_volume", "remove_small_components")
def test_tsdf_prune_merge_register_remove():
    vol, src = tsdf(), tsdf()
    src._h = ctypes.c_void_p(0xCAFE)
    SRC = ("p", 0xCAFE)
    st = vol.prune()
    expect(vol, ("hv_tsdf_prune", 1, None, None, REF(L.HvPruneStats)))
    assert type(st) is V.PruneStats
    primes(st, L.HvPruneStats)
    vol._lib.script("hv_tsdf_prune", peek={2: (np.int32, 3), 3: (np.int32, 3)})
    bounds = ((-1.0, 0.0, 0.5), (1.0, 2.0, 3.0))
    vol.prune(empty=False, bounds=bounds)
    expect(vol, ("hv_tsdf_prune", 0, ANY, ANY, REF(L.HvPruneStats)))
    lo, hi = V.unit_range_of_bounds(bounds, 0.02, 16)
    np.testing.assert_array_equal(vol._lib.peeked[0][2], lo)
    np.testing.assert_array_equal(vol._lib.peeked[0][3], hi)
    refused(vol, ValueError, "bounds must be (min_xyz, max_xyz) with three coordinates each", vol.prune, bounds=((0, 0), (1, 1)))

    vol._lib.script("hv_tsdf_integrate_volume", peek={2: (np.float64, 16)})
    st = vol.integrate_volume(src)
    vol.integrate_volume(src, pose(3))
    expect(vol, ("hv_tsdf_integrate_volume", SRC, ANY, REF(L.HvMergeStats)), ("hv_tsdf_integrate_volume", SRC, ANY, REF(L.HvMergeStats)))
    assert type(st) is V.MergeStats
    primes(st, L.HvMergeStats)
    np.testing.assert_array_equal(vol._lib.peeked[1][2], np.eye(4).reshape(-1))
    np.testing.assert_array_equal(vol._lib.peeked[2][2], pose(3).reshape(-1))
    refused(vol, TypeError, "integrate_volume: source must be a volume", vol.integrate_volume, object())
    refused(vol, ValueError, "integrate_volume: transformation must be a 4x4 matrix", vol.integrate_volume, src, np.eye(3))

    vol._lib.script("hv_tsdf_register_volume", 2, peek={2: (np.float64, 16)})
    r = vol.register_volume(src, pose(4))
    (_, args), = expect(vol, ("hv_tsdf_register_volume", SRC, ANY, REF(L.HvRegisterParams), REF(L.HvRegisterResult), None, 0, REF(I64)))
    prm = ref(args[3])
    assert (prm.weight_threshold, prm.tsdf_band, prm.residual_trunc, prm.huber_delta, prm.max_iterations) == (3.0, 0.5, 0.04, 0.02, 30)
    np.testing.assert_array_equal(vol._lib.peeked[-1][2], pose(4).reshape(-1))
    assert type(r) is V.RegistrationResult and r.trace is None and r.transformation.shape == (4, 4) and r.information.shape == (6, 6)
    assert r.anchor.shape == (3,) and r.success is False and (r.iterations, r.inliers, r.candidates) == (0, 0, 0)
    r = vol.register_volume(src, max_iterations=7, residual_trunc=0.3, huber_delta=0.1, trace=True)
    (_, args), = expect(vol, ("hv_tsdf_register_volume", SRC, ANY, REF(L.HvRegisterParams), REF(L.HvRegisterResult), ANY, 7, REF(I64)))
    assert (ref(args[3]).residual_trunc, ref(args[3]).huber_delta, ref(args[3]).max_iterations) == (0.3, 0.1, 7)
    assert len(r.trace) == 2 and set(r.trace[0]) == {"iteration", "status", "inliers", "candidates", "sq_error", "A", "H", "g", "xi"}
    assert r.trace[0]["A"].shape == (4, 4) and r.trace[0]["H"].shape == (6, 6) and r.trace[0]["g"].shape == (6,) and r.trace[0]["xi"].shape == (6,)
    refused(vol, TypeError, "register_volume: source must be a volume", vol.register_volume, None)
    refused(vol, ValueError, "register_volume: init must be a 4x4 matrix", vol.register_volume, src, np.eye(3))

    st = vol.remove_small_components(5)
    vol.remove_small_components(9, weight_threshold=2, margin=3)
    expect(vol, ("hv_tsdf_remove_components", 0.0, 5, 4, REF(L.HvRemoveComponentsStats)),
           ("hv_tsdf_remove_components", 2.0, 9, 3, REF(L.HvRemoveComponentsStats)))
    assert type(st) is V.ComponentRemovalStats
    primes(st, L.HvRemoveComponentsStats)


def test_trace_rows_name_every_column():
    """The per-linearisation records of tracking and registration: each column under its own name."""
    row = np.arange(100, 100 + L.HV_TRACK_COLOR_TRACE_STRIDE, dtype=np.float64)
    iu = np.triu_indices(6)
    for r, photometric in ((row[:L.HV_TRACK_TRACE_STRIDE], False), (row, True)):
        t, = V._trace_rows(r[None])
        assert (t["level"], t["iteration"], t["status"], t["inliers"], t["valid"], t["sq_error"]) == (100, 101, 102, 103, 104, 105.0)
        np.testing.assert_array_equal(t["A"], r[6:22].reshape(4, 4))
        np.testing.assert_array_equal(t["H"][iu], r[22:43])
        np.testing.assert_array_equal(t["H"], t["H"].T)
        np.testing.assert_array_equal(t["g"], r[43:49])
        np.testing.assert_array_equal(t["xi"], r[49:55])
        assert ("photometric_inliers" in t) == photometric and (not photometric or (t["photometric_inliers"], t["sq_intensity_error"]) == (156, 157.0))
        assert all(type(t[k]) is int for k in ("level", "iteration", "status", "inliers", "valid")) and type(t["sq_error"]) is float


@covers("reset", "set_color_order", "set_tile", "set_rectify_maps", "set_owner", "mark_merged", "synchronize", "reserve_blocks",
        "set_stream", "register_host_memory", "unregister_host_memory", "profile_enable", "profile_read", "profile_launches",
        "num_blocks", "max_blocks", "dropped_points", "bytes_per_block", "close")
def test_tsdf_settings_and_counters():
    vol = tsdf()
    mx, my = np.zeros((3, 5), np.float32), np.ones((3, 5), np.float32)
    vol.reset(), vol.set_color_order(True), vol.set_color_order(), vol.set_tile(1, 2, 3, 4), vol.set_rectify_maps(None, None)
    vol.set_rectify_maps(mx, my), vol.set_owner(1, 4), vol.mark_merged(), vol.synchronize(), vol.reserve_blocks(100)
    vol.set_stream(0x1234), vol.register_host_memory(0x1000, 64), vol.unregister_host_memory(0x1000), vol.profile_enable(), vol.profile_enable(False)
    expect(vol, ("hv_reset",), ("hv_tsdf_set_color_order", 1), ("hv_tsdf_set_color_order", 0), ("hv_tsdf_set_tile", 1, 2, 3, 4),
           ("hv_tsdf_set_rectify_maps", None, None, 0, 0, L.HV_HOST), ("hv_tsdf_set_rectify_maps", P(mx), P(my), 3, 5, L.HV_HOST),
           ("hv_tsdf_set_owner", 1, 4), ("hv_tsdf_mark_merged",), ("hv_synchronize",), ("hv_reserve_blocks", 100),
           ("hv_set_stream", ("p", 0x1234)), ("hv_host_register", ("p", 0x1000), 64), ("hv_host_unregister", ("p", 0x1000)),
           ("hv_profile_enable", 1), ("hv_profile_enable", 0))
    vol._lib.script("hv_profile_read", 1.5, 7, 9)
    assert vol.profile_read() == (1.5, 7, 9)
    expect(vol, ("hv_profile_read", REF(ctypes.c_double), REF(I64), REF(I64)))
    for i, name in enumerate(("num_blocks", "max_blocks", "dropped_points", "bytes_per_block")):
        vol._lib.script("hv_" + name, 41 + i)
        n = getattr(vol, name)()
        assert n == 41 + i and type(n) is int
        expect(vol, ("hv_" + name, REF(I64)))
    vol._lib.script("hv_profile_read_launches", 3)
    out = vol.profile_launches()
    expect(vol, ("hv_profile_read_launches", None, 0, REF(I64)), ("hv_profile_read_launches", P(out), 3, REF(I64)))
    shaped(out, (3,), np.float32)
    vol._lib.script("hv_profile_read_launches", 0)
    shaped(vol.profile_launches(), (0,), np.float32)
    expect(vol, ("hv_profile_read_launches", None, 0, REF(I64)))
    vol.close()
    expect(vol, ("hv_destroy",))
    assert vol._h is None
    vol.close()
    assert vol._lib.calls == []


@covers("extract_triangle_mesh", "extract_point_cloud")
def test_tsdf_extraction():
    vol = tsdf()
    for dtype, suffix in ((None, ""), (np.float64, ""), (np.float32, "_f32")):
        dt = np.float32 if suffix else np.float64
        vol._lib.script("hv_tsdf_extract_mesh" + suffix, 5, 7)
        m = vol.extract_triangle_mesh(dtype=dtype)
        expect(vol, ("hv_tsdf_extract_mesh" + suffix, None, None, 0, None, 0, REF(I64), REF(I64)),
               ("hv_tsdf_extract_mesh" + suffix, P(m.vertices), P(m.vertex_colors), 5, P(m.triangles), 7, REF(I64), REF(I64)))
        assert type(m) is V.TriangleMesh
        shaped(m.vertices, (5, 3), dt), shaped(m.vertex_colors, (5, 3), dt), shaped(m.triangles, (7, 3), np.int32)
        vol._lib.script("hv_tsdf_extract_points" + suffix, 4).script("hv_tsdf_extract_point_normals", 4)
        pc = vol.extract_point_cloud(dtype=dtype)
        expect(vol, ("hv_tsdf_extract_points" + suffix, None, None, 0, REF(I64)),
               ("hv_tsdf_extract_points" + suffix, P(pc.points), P(pc.colors), 4, REF(I64)))
        assert type(pc) is V.PointCloud and pc.normals is None
        shaped(pc.points, (4, 3), dt), shaped(pc.colors, (4, 3), dt)
        pc = vol.extract_point_cloud(normals=True, dtype=dtype)
        expect(vol, ("hv_tsdf_extract_points" + suffix, None, None, 0, REF(I64)),
               ("hv_tsdf_extract_points" + suffix, P(pc.points), P(pc.colors), 4, REF(I64)),
               ("hv_tsdf_extract_point_normals", P(pc.normals), 4, REF(I64)))
        shaped(pc.normals, (4, 3), np.float64)
    vol._lib.script("hv_tsdf_extract_mesh", 0, 0).script("hv_tsdf_extract_points", 0)
    m, pc = vol.extract_triangle_mesh(), vol.extract_point_cloud(normals=True)
    expect(vol, ("hv_tsdf_extract_mesh", None, None, 0, None, 0, REF(I64), REF(I64)), ("hv_tsdf_extract_points", None, None, 0, REF(I64)))
    shaped(m.vertices, (0, 3), np.float64), shaped(m.triangles, (0, 3), np.int32), shaped(pc.points, (0, 3), np.float64)
    shaped(pc.normals, (0, 3), np.float64)
    vol._lib.script("hv_tsdf_extract_mesh", 0, 2)  # (triangles without vertices: the fetch still runs, as it does today)
    vol.extract_triangle_mesh()
    assert vol._lib.names() == ["hv_tsdf_extract_mesh"] * 2
    vol._lib.calls = []
    for fn in (vol.extract_triangle_mesh, vol.extract_point_cloud):
        refused(vol, TypeError, "extraction dtype must be float64 (Open3D's) or float32, got int32", fn, dtype=np.int32)


@covers("ray_cast")
def test_tsdf_ray_cast():
    vol = tsdf()
    vol._lib.script("hv_tsdf_ray_cast", peek={3: (np.float64, 4), 4: (np.float64, 16)})
    out = vol.ray_cast(K, pose(1))
    expect(vol, ("hv_tsdf_ray_cast", IH, IW, ANY, ANY, 0.1, 3.0, 3.0, 1.0, P(out["depth"]), P(out["vertex"]), P(out["normal"]), P(out["color"]),
                 P(out["mask"]), L.HV_HOST))
    assert list(out) == ["depth", "vertex", "normal", "color", "mask"]
    shaped(out["depth"], (IH, IW), np.float32), shaped(out["mask"], (IH, IW), np.bool_)
    for a in ("vertex", "normal", "color"):
        shaped(out[a], (IH, IW, 3), np.float32)
    np.testing.assert_array_equal(vol._lib.peeked[0][3], K.as_array())
    np.testing.assert_array_equal(vol._lib.peeked[0][4], pose(1).reshape(-1))
    out = vol.ray_cast(K, pose(1), depth_min=1, depth_max=2, weight_threshold=0, depth_scale=1000, render_attributes=("mask", "normal"))
    expect(vol, ("hv_tsdf_ray_cast", IH, IW, ANY, ANY, 1.0, 2.0, 0.0, 1000.0, None, None, P(out["normal"]), None, P(out["mask"]), L.HV_HOST))
    assert list(out) == ["mask", "normal"]
    refused(vol, ValueError, "ray_cast: unknown render attribute(s) ['rgb']; choose from ('depth', 'vertex', 'normal', 'color', 'mask')",
            vol.ray_cast, K, pose(1), render_attributes=("depth", "rgb"))
    refused(vol, RuntimeError, "T_cw must be a 4x4 matrix", vol.ray_cast, K, np.eye(3))


@covers("track_frame_to_model")
def test_tsdf_track(host):
    depth, color = frames()
    d, c = host(depth), host(color)
    vol = tsdf()
    r = vol.track_frame_to_model(d, K, pose(1))
    (_, args), = expect(vol, ("hv_tsdf_track", P(d), L.HV_DEPTH_F32, IH, IW, ANY, ANY, REF(L.HvTrackParams), REF(L.HvTrackResult), None, 0,
                              REF(I64), L.HV_HOST))
    prm = ref(args[7])
    assert (prm.depth_scale, prm.depth_min, prm.depth_max, prm.weight_threshold, prm.depth_outlier_trunc, prm.depth_huber_delta) == \
        (1.0, 0.1, 3.0, 3.0, 0.07, 0.05)
    assert prm.n_levels == 3 and list(prm.iterations)[:4] == [10, 5, 4, 0]
    assert type(r) is V.OdometryResult and r.iterations == (0, 0, 0) and r.trace is None and r.photometric_inliers is None
    assert r.intensity_rmse is None and r.transformation.shape == (4, 4) and r.information.shape == (6, 6)
    vol._lib.script("hv_tsdf_track_color", 2)
    r = vol.track_frame_to_model(d, K, pose(1), iterations=(3, 2), trace=True, color=c, intensity_weight=0.5, intensity_huber_delta=0.2)
    (_, args), = expect(vol, ("hv_tsdf_track_color", P(d), L.HV_DEPTH_F32, P(c), IH, IW, ANY, ANY, REF(L.HvTrackColorParams),
                              REF(L.HvTrackColorResult), ANY, 5, REF(I64), L.HV_HOST))
    assert (ref(args[8]).intensity_weight, ref(args[8]).intensity_huber_delta, ref(args[8]).base.n_levels) == (0.5, 0.2, 2)
    assert len(r.trace) == 2 and "photometric_inliers" in r.trace[0] and r.photometric_inliers == 0 and r.intensity_rmse == 0.0
    vol._lib.script("hv_tsdf_track", 1)
    r = vol.track_frame_to_model(d, K, pose(1), trace=True)
    expect(vol, ("hv_tsdf_track", P(d), L.HV_DEPTH_F32, IH, IW, ANY, ANY, REF(L.HvTrackParams), REF(L.HvTrackResult), ANY, 19, REF(I64), L.HV_HOST))
    assert len(r.trace) == 1 and "photometric_inliers" not in r.trace[0]
    refused(vol, RuntimeError, UNSUPPORTED, vol.track_frame_to_model, host(depth[:, :-1].copy()), K, pose(1))
    refused(vol, RuntimeError, UNSUPPORTED, vol.track_frame_to_model, d, K, pose(1), color=host(color[:-1].copy()))
    refused(vol, RuntimeError, "T_cw must be a 4x4 matrix", vol.track_frame_to_model, d, K, np.eye(3))


@pytest.mark.parametrize("f64", [False, True])
@covers("sample_points")
def test_tsdf_sample_points(host, f64):
    pts = np.random.default_rng(1).random((5, 3)).astype(np.float64 if f64 else np.float32)
    p = host(pts)
    vol = tsdf()
    for device in (None, False):
        r = vol.sample_points(p, device=device)
        expect(vol, ("hv_tsdf_sample_points", P(p), L.HV_F64 if f64 else L.HV_F32, 5, 0.0, P(r.sdf), P(r.gradient), None, P(r.weight),
                     P(r.status), L.HV_HOST))
        assert type(r) is V.SampleResult and r.color is None
        shaped(r.sdf, (5,), np.float32), shaped(r.gradient, (5, 3), np.float32), shaped(r.weight, (5,), np.float32)
        shaped(r.status, (5,), np.uint8)
    r = vol.sample_points(p, weight_threshold=2, gradient=False, color=True)
    expect(vol, ("hv_tsdf_sample_points", P(p), L.HV_F64 if f64 else L.HV_F32, 5, 2.0, P(r.sdf), None, P(r.color), P(r.weight), P(r.status),
                 L.HV_HOST))
    assert r.gradient is None
    shaped(r.color, (5, 3), np.float32)
    p0 = host(pts[:0])
    r = vol.sample_points(p0)
    expect(vol, ("hv_tsdf_sample_points", SKIP, L.HV_F64 if f64 else L.HV_F32, 0, 0.0, P(r.sdf), P(r.gradient), None, P(r.weight), P(r.status),
                 L.HV_HOST))
    kind = "torch.int64" if hasattr(p, "data_ptr") and not isinstance(p, np.ndarray) else "int64"
    refused(vol, ValueError, f"sample_points: points must be float32 or float64, got {kind}", vol.sample_points, host(np.zeros((5, 3), np.int64)))
    refused(vol, ValueError, "sample_points: points must have shape [n, 3], got (5, 2)", vol.sample_points, host(pts[:, :2].copy()))
    refused(vol, ValueError, "sample_points: points must have shape [n, 3], got (3,)", vol.sample_points, host(pts[0].copy()))


@covers("check_frame")
def test_tsdf_check_frame(host):
    depth, _ = frames()
    d = host(depth)
    vol = tsdf()
    vol._lib.script("hv_tsdf_check_frame", peek={5: (np.float64, 4), 6: (np.float64, 16)})
    for device in (None, False):
        r = vol.check_frame(d, K, pose(2), device=device)
        (_, args), = expect(vol, ("hv_tsdf_check_frame", P(d), L.HV_DEPTH_F32, IH, IW, ANY, ANY, REF(L.HvCheckParams), P(r.sdf), P(r.cls),
                                  REF(L.HvCheckStats), L.HV_HOST))
        prm = ref(args[7])
        assert (prm.depth_scale, prm.depth_min, prm.depth_max, prm.weight_threshold, prm.tolerance) == (1.0, 0.1, 3.0, 0.0, 0.04)
        assert type(r) is V.FrameCheck and type(r.stats) is V.FrameCheckStats
        assert (r.invalid, r.unknown, r.consistent, r.in_front, r.behind) == (2, 3, 5, 7, 11) == r.stats.as_tuple()
        shaped(r.sdf, (IH, IW), np.float32), shaped(r.cls, (IH, IW), np.uint8)
    np.testing.assert_array_equal(vol._lib.peeked[0][6], pose(2).reshape(-1))
    r = vol.check_frame(d, K, pose(2), depth_scale=1000, depth_min=0.5, depth_max=2, weight_threshold=1, tolerance=0.01)
    (_, args), = vol._lib.calls
    prm = ref(args[7])
    assert (prm.depth_scale, prm.depth_min, prm.depth_max, prm.weight_threshold, prm.tolerance) == (1000.0, 0.5, 2.0, 1.0, 0.01)
    vol._lib.calls = []
    refused(vol, RuntimeError, UNSUPPORTED, vol.check_frame, host(depth[:-1].copy()), K, pose(2))
    refused(vol, RuntimeError, "T_cw must be a 4x4 matrix", vol.check_frame, d, K, np.eye(3))


@covers("distance_field")
def test_tsdf_distance_field():
    vol = tsdf()
    bounds = ((0.0, 0.01, -0.05), (0.11, 0.15, 0.03))  # voxels 0..5, 0..7, -3..1
    f = vol.distance_field(bounds, 0.03)
    (_, args), = expect(vol, ("hv_tsdf_distance_field", REF(L.HvDistanceParams), P(f.distance.base), None, P(f.cls.base), REF(L.HvDistanceStats),
                              L.HV_HOST))
    prm = ref(args[1])
    assert (list(prm.origin), list(prm.shape), prm.radius, prm.weight_threshold) == ([-2, -2, -5], [10, 12, 9], 2, 0.0)
    assert type(f) is V.DistanceField and type(f.stats) is V.DistanceFieldStats and f.dist2 is None
    primes(f.stats, L.HvDistanceStats)
    shaped(f.distance, (6, 8, 5), np.float32), shaped(f.cls, (6, 8, 5), np.uint8)
    assert f.distance.base.shape == (10, 12, 9) and addr(f.distance) == addr(f.distance.base) + 4 * ((2 * 12 + 2) * 9 + 2)
    assert (f.origin.tolist(), f.shape, f.radius, f.voxel_length) == ([0, 0, -3], (6, 8, 5), 2, 0.02)
    f = vol.distance_field(bounds, 0.03, weight_threshold=1, pad=False, outputs=("dist2",))
    (_, args), = expect(vol, ("hv_tsdf_distance_field", REF(L.HvDistanceParams), None, P(f.dist2), None, REF(L.HvDistanceStats), L.HV_HOST))
    assert (list(ref(args[1]).origin), list(ref(args[1]).shape), ref(args[1]).weight_threshold) == ([0, 0, -3], [6, 8, 5], 1.0)
    shaped(f.dist2, (6, 8, 5), np.uint32)
    assert f.distance is None and f.cls is None
    refused(vol, ValueError, "distance_field: unknown output(s) ['sdf']; choose from ('distance', 'dist2', 'cls')", vol.distance_field, bounds,
            0.03, outputs=("sdf",))
    refused(vol, ValueError, "distance_field: bounds must be (lo_xyz, hi_xyz), finite, lo <= hi", vol.distance_field, (bounds[1], bounds[0]), 0.03)
    refused(vol, ValueError, "distance_field: bounds must be (lo_xyz, hi_xyz):", vol.distance_field, 3, 0.03)
    refused(vol, ValueError, "distance_field: max_distance must be positive and finite, got 0.0", vol.distance_field, bounds, 0.0)
    refused(vol, ValueError, "distance_field: max_distance 100.0 is 5000 voxels; the radius is limited to 1024", vol.distance_field, bounds, 100.0)
    refused(vol, ValueError, "distance_field: bounds reach beyond voxel index +-2^30", vol.distance_field, ((0, 0, 0), (1e9, 1, 1)), 0.03)
    refused(vol, ValueError, "; the limit is 4096 per axis (a smaller box, a smaller max_distance or pad=False)", vol.distance_field,
            ((0, 0, 0), (100.0, 1, 1)), 0.03)


@covers("surface_components")
def test_tsdf_surface_components():
    vol = tsdf()
    size = ("hv_tsdf_surface_components", 0.0, None, None, None, None, 0, None, None, 0, REF(I64), REF(I64), REF(L.HvComponentsStats), L.HV_HOST)
    vol._lib.script("hv_tsdf_surface_components", 3, 10)
    r = vol.surface_components()
    expect(vol, size, ("hv_tsdf_surface_components", 0.0, P(r.seed), P(r.sites), P(r.lo), P(r.hi), 3, None, None, 10, REF(I64), REF(I64),
                       REF(L.HvComponentsStats), L.HV_HOST))
    assert type(r) is V.SurfaceComponents and type(r.stats) is V.SurfaceComponentsStats and r.site_index is None and r.site_label is None
    primes(r.stats, L.HvComponentsStats)
    assert len(r) == 5 and r.voxel_length == 0.02
    shaped(r.seed, (3, 3), np.int32), shaped(r.sites, (3,), np.int64), shaped(r.lo, (3, 3), np.int32), shaped(r.hi, (3, 3), np.int32)
    r = vol.surface_components(weight_threshold=2, sites=True)
    expect(vol, ("hv_tsdf_surface_components", 2.0) + size[2:],
           ("hv_tsdf_surface_components", 2.0, P(r.seed), P(r.sites), P(r.lo), P(r.hi), 3, P(r.site_index), P(r.site_label), 10, REF(I64), REF(I64),
            REF(L.HvComponentsStats), L.HV_HOST))
    shaped(r.site_index, (10, 3), np.int32), shaped(r.site_label, (10,), np.int32)
    vol._lib.script("hv_tsdf_surface_components", 0, 0)
    r = vol.surface_components(sites=True)
    expect(vol, size)
    shaped(r.seed, (0, 3), np.int32), shaped(r.sites, (0,), np.int64), shaped(r.site_index, (0, 3), np.int32), shaped(r.site_label, (0,), np.int32)
    primes(r.stats, L.HvComponentsStats)


@covers("dump", "touched_keys", "unit_keys", "dirty_keys")
def test_tsdf_dump_and_key_lists():
    vol = tsdf()
    vol._lib.script("hv_num_blocks", 2)
    keys, t, w, c = vol.dump()
    expect(vol, ("hv_num_blocks", REF(I64)), ("hv_tsdf_dump", P(keys), P(t), P(w), P(c), REF(I64)))
    shaped(keys, (2, 3), np.int32), shaped(t, (2, 4096), np.float32), shaped(w, (2, 4096), np.float32), shaped(c, (2, 4096, 3), np.float64)
    for method, name in (("touched_keys", "hv_tsdf_touched"), ("unit_keys", "hv_tsdf_unit_keys"), ("dirty_keys", "hv_tsdf_dirty_keys")):
        vol._lib.script(name, 4)
        keys = getattr(vol, method)()
        expect(vol, (name, None, 0, REF(I64)), (name, P(keys), 4, REF(I64)))
        shaped(keys, (4, 3), np.int32)
        vol._lib.script(name, 0)
        shaped(getattr(vol, method)(), (0, 3), np.int32)
        expect(vol, (name, None, 0, REF(I64)))


@covers("halo_lists_device", "halo_plan_device", "halo_plan_fetch", "halo_pack_planned", "halo_unpack_planned", "halo_unpack",
        "export_numerators", "import_numerators")
def test_tsdf_halo_and_numerators():
    torch = pytest.importorskip("torch")
    vol = tsdf()
    dirty, held = torch.zeros(8, dtype=torch.int64), torch.zeros(9, dtype=torch.int64)
    vol._lib.script("hv_merge_halo_lists_device", 3, 4)
    assert vol.halo_lists_device(dirty, held) == (3, 4)
    expect(vol, ("hv_merge_halo_lists_device", P(dirty), 8, P(held), 9, REF(I64), REF(I64)))
    da, ha = torch.zeros((2, 8), dtype=torch.int64), torch.zeros((2, 9), dtype=torch.int64)
    dc, hc = np.array([3, 1], np.int64), np.array([4, 2], np.int64)
    vol._lib.script("hv_merge_halo_plan_device", 6)
    assert vol.halo_plan_device(da, dc, ha, hc, 2, 1, all_dirty_kept=True) == 6
    expect(vol, ("hv_merge_halo_plan_device", P(da), P(dc), 8, P(ha), P(hc), 9, 2, 1, 1, REF(I64)))
    vol._lib.script("hv_merge_halo_plan_fetch", 3)
    keys, action = vol.halo_plan_fetch()
    expect(vol, ("hv_merge_halo_plan_fetch", None, None, 0, REF(I64)), ("hv_merge_halo_plan_fetch", P(keys), P(action), 3, REF(I64)))
    shaped(keys, (3, 3), np.int32), shaped(action, (3,), np.uint8)
    vol._lib.script("hv_merge_halo_plan_fetch", 0)
    keys, action = vol.halo_plan_fetch()
    expect(vol, ("hv_merge_halo_plan_fetch", None, None, 0, REF(I64)))
    shaped(keys, (0, 3), np.int32), shaped(action, (0,), np.uint8)
    payload = np.zeros((2, 4096, 5), np.float32)
    keys, action = np.zeros((2, 3), np.int32), np.ones(2, np.uint8)
    vol.halo_pack_planned(1, 2, payload), vol.halo_unpack_planned(3, 4, payload), vol.halo_unpack(keys, payload, action)
    out = vol.export_numerators(keys)
    assert vol.export_numerators(keys, out=payload) is payload
    vol.import_numerators(keys, payload)
    expect(vol, ("hv_merge_halo_pack_planned", 1, 2, P(payload)), ("hv_merge_halo_unpack_planned", 3, 4, P(payload)),
           ("hv_merge_halo_unpack", P(keys), 2, P(payload), P(action), L.HV_HOST), ("hv_tsdf_export_numerators", P(keys), 2, P(out), L.HV_HOST),
           ("hv_tsdf_export_numerators", P(keys), 2, P(payload), L.HV_HOST), ("hv_tsdf_import_numerators", P(keys), 2, P(payload), L.HV_HOST))
    shaped(out, (2, 4096, 5), np.float32)


@covers("pack", "unpack", "save")
def test_tsdf_packed_maps(host, tmp_path):
    vol = tsdf()
    out = vol.pack()
    expect(vol, ("hv_tsdf_pack_size", REF(L.HvPackInfo)), ("hv_tsdf_pack", P(out), 5, L.HV_HOST, REF(L.HvPackInfo)))
    shaped(out, (5,), np.uint8)
    buf = np.arange(16, dtype=np.uint8)
    st = vol.unpack(host(buf))
    expect(vol, ("hv_tsdf_unpack", P(buf), 16, L.HV_HOST, REF(L.HvPackInfo)))
    assert type(st) is V.PackStats
    primes(st, L.HvPackInfo)
    vol.unpack(bytes(buf))
    expect(vol, ("hv_tsdf_unpack", ANY, 16, L.HV_HOST, REF(L.HvPackInfo)))
    st = vol.save(tmp_path / "map.bin")
    expect(vol, ("hv_tsdf_pack_size", REF(L.HvPackInfo)), ("hv_tsdf_pack", ANY, 5, L.HV_HOST, REF(L.HvPackInfo)))
    primes(st, L.HvPackInfo)
    assert (tmp_path / "map.bin").stat().st_size == 5 and [p.name for p in tmp_path.iterdir()] == ["map.bin"]
    refused(vol, ValueError, "a packed map is a 1-D uint8 buffer, got", vol.unpack, host(np.zeros(4, np.float32)))
    refused(vol, ValueError, "a packed map is a 1-D uint8 buffer, got", vol.unpack, host(np.zeros((4, 4), np.uint8)))


# ---- what every volume class has: image filters, carving ----------------------------------------------------------------------
@covers("filter_shadow_points", "remap")
def test_filter_and_remap(host):
    depth, color = frames()
    d = host(depth)
    vol = tsdf()
    out = vol.filter_shadow_points(d)
    out2 = vol.filter_shadow_points(d, delta_x=3, delta_y=4, fill_value=0)
    expect(vol, ("hv_filter_shadow_points", P(d), IH, IW, 2, 2, -1.0, P(out), L.HV_HOST),
           ("hv_filter_shadow_points", P(d), IH, IW, 3, 4, 0.0, P(out2), L.HV_HOST))
    assert type(out) is type(d) and tuple(out.shape) == (IH, IW) and str(out.dtype).endswith("float32")
    out = vol.filter_shadow_points(host(depth.astype(np.float64)))  # converted: the library reads float32
    (_, args), = expect(vol, ("hv_filter_shadow_points", ANY, IH, IW, 2, 2, -1.0, P(out), L.HV_HOST))
    mx, my = np.zeros((IH, IW), np.float32), np.ones((IH, IW), np.float32)
    for img, kind, C in ((color, 0, 3), (depth, 1, 1), (depth.astype(np.int32), 2, 1)):
        out = vol.remap(img, mx, my)
        out2 = vol.remap(img, mx, my, linear=True)
        expect(vol, ("hv_remap", P(img), kind, C, IH, IW, P(mx), P(my), 0, P(out), L.HV_HOST),
               ("hv_remap", P(img), kind, C, IH, IW, P(mx), P(my), 1, P(out2), L.HV_HOST))
        shaped(out, img.shape, img.dtype)
    refused(vol, RuntimeError, "remap: unsupported image dtype float64", vol.remap, depth.astype(np.float64), mx, my)


@covers("carve")
def test_carve(host):
    depth, _ = frames()
    d = host(depth)
    f = frustum()
    for vol in (volume(V.VoxelBlockGrid, voxel_size=0.05, block_size=8), volume(S.VoxelBlockSemanticGrid, voxel_size=0.05, block_size=8)):
        assert vol.carve(f, d) is None and vol.carve(f, d, 0.5) is None
        expect(vol, ("hv_carve", P(f.intr), IW, IH, P(f.T_cw), 5.0, f.depth_min, P(d), 0.01, L.HV_HOST),
               ("hv_carve", P(f.intr), IW, IH, P(f.T_cw), 5.0, f.depth_min, P(d), 0.5, L.HV_HOST))
        assert vol.carve(f, host(depth[:-1].copy())) is None and vol.carve(f, host(depth[:0].copy())) is None  # the reference returns
        expect(vol)


# ---- VoxelBlockGrid -----------------------------------------------------------------------------------------------------------
def grid():
    return volume(V.VoxelBlockGrid, voxel_size=0.05, block_size=8)


POINT_REFUSALS = (("points must be a contiguous Nx3 array", lambda p, c: (p[:, :2].copy(), None)),
                  ("points must be a contiguous Nx3 array", lambda p, c: (p[0].copy(), None)),
                  ("colors must be a contiguous Nx3 array", lambda p, c: (p, c[:, :2].copy())),
                  ("points and colors must have the same size", lambda p, c: (p, c[:-1].copy())))


@covers("integrate")
def test_grid_integrate_points(host):
    rng = np.random.default_rng(2)
    p32, p64 = rng.random((5, 3)).astype(np.float32), rng.random((5, 3))
    c8, c32 = rng.integers(0, 256, (5, 3)).astype(np.uint8), rng.random((5, 3)).astype(np.float32)
    vol = grid()
    for pts, fn in ((p32, "hv_integrate_points"), (p64, "hv_integrate_points_f64")):
        p, a, b = host(pts), host(c8), host(c32)
        assert vol.integrate(p) is None and vol.integrate(p, a) is None and vol.integrate(p, b) is None
        expect(vol, (fn, P(p), 5, None, L.HV_COLOR_NONE, L.HV_HOST), (fn, P(p), 5, P(a), L.HV_COLOR_U8, L.HV_HOST),
               (fn, P(p), 5, P(b), L.HV_COLOR_F32, L.HV_HOST))
    vol.integrate(host(p32.astype(np.float16)))  # anything but float64 goes through float32
    expect(vol, ("hv_integrate_points", ANY, 5, None, L.HV_COLOR_NONE, L.HV_HOST))
    assert vol.integrate(host(p32[:0]), host(c8[:0])) is None
    expect(vol)
    for message, make in POINT_REFUSALS:
        p, c = make(p32, c8)
        refused(vol, RuntimeError, message, vol.integrate, host(p), None if c is None else host(c))
    kind = "torch.float64" if host(p64) is not p64 else "float64"
    refused(vol, RuntimeError, f"Colors must be uint8 or float32, got dtype with {kind}", vol.integrate, host(p32), host(p64))


@covers("integrate_rgbd", "integrate_rgbd_batch")
def test_grid_integrate_rgbd(host):
    vol = grid()
    vol._lib.script("hv_integrate_rgbd_points", peek={7: (np.float64, 4), 8: (np.float64, 16)})
    vol._lib.script("hv_integrate_rgbd_points_batch", peek={8: (np.float64, 4), 9: (np.float64, 32)})
    for u16 in (False, True):
        kind = L.HV_DEPTH_U16 if u16 else L.HV_DEPTH_F32
        depth, color = frames(u16=u16)
        d, c = host(depth), host(color)
        vol.integrate_rgbd(d, c, 8.0, 7.0, 3.3, 4.1, pose(1))
        vol.integrate_rgbd(d, c, 8.0, 7.0, 3.3, 4.1, pose(1), max_depth=4, min_depth=1, depth_scale=1000)
        expect(vol, ("hv_integrate_rgbd_points", P(d), kind, 1.0, P(c), IH, IW, ANY, ANY, 0.0, 3.0e38, L.HV_HOST),
               ("hv_integrate_rgbd_points", P(d), kind, 1000.0, P(c), IH, IW, ANY, ANY, 1.0, 4.0, L.HV_HOST))
        depth, color = frames(2, u16=u16)
        d, c = host(depth), host(color)
        T = np.stack([pose(1), pose(2)])
        vol.integrate_rgbd_batch(d, c, 8.0, 7.0, 3.3, 4.1, T)
        expect(vol, ("hv_integrate_rgbd_points_batch", P(d), kind, 1.0, P(c), 2, IH, IW, ANY, ANY, 0.0, 3.0e38, L.HV_HOST))
        np.testing.assert_array_equal(vol._lib.peeked[-1][8], [8.0, 7.0, 3.3, 4.1])
        np.testing.assert_array_equal(vol._lib.peeked[-1][9], T.reshape(-1))
    np.testing.assert_array_equal(vol._lib.peeked[0][8], pose(1).reshape(-1))
    depth, color = frames()
    refused(vol, RuntimeError, f"integrate_rgbd: colour image {(IH, IW - 1, 3)} does not match depth {(IH, IW)}", vol.integrate_rgbd,
            host(depth), host(color[:, :-1].copy()), 8.0, 7.0, 3.3, 4.1, pose(1))
    refused(vol, RuntimeError, "T_cw must be a 4x4 matrix", vol.integrate_rgbd, host(depth), host(color), 8.0, 7.0, 3.3, 4.1, np.eye(3))


@covers("get_voxels", "get_points", "get_colors", "get_voxels_in_bb", "get_voxels_in_camera_frustrum", "remove_low_count_voxels",
        "remove_low_confidence_voxels", "clear", "reset", "size", "get_total_voxel_count", "empty", "get_block_size", "set_owner",
        "dump", "keys_from_points")
def test_grid_queries_and_housekeeping():
    vol = grid()
    f = frustum()
    bb = V.BoundingBox3D((0, 1, 2), (3, 4, 5))
    bba = np.arange(6, dtype=np.float64)
    tail0, tail = (None, None, 0, REF(I64), L.HV_HOST), lambda r: (P(r.points), P(r.colors), 3, REF(I64), L.HV_HOST)
    for n in (3, 0):
        for name in ("hv_get_voxels", "hv_get_voxels_in_bb", "hv_get_voxels_in_frustum"):
            vol._lib.script(name, n, peek={1: (np.float64, 6)} if name == "hv_get_voxels_in_bb" else None)
        results = [vol.get_voxels(), vol.get_voxels(2, 0.5), vol.get_voxels_in_bb(bb, 2), vol.get_voxels_in_bb(bba),
                   vol.get_voxels_in_camera_frustrum(f, 3, 0.25)]
        heads = [("hv_get_voxels", 1, 0.0), ("hv_get_voxels", 2, 0.5), ("hv_get_voxels_in_bb", ANY, 2, 0.0), ("hv_get_voxels_in_bb", P(bba), 1, 0.0),
                 ("hv_get_voxels_in_frustum", P(f.intr), IW, IH, P(f.T_cw), 5.0, f.depth_min, 3, 0.25)]
        expect(vol, *[call for h, r in zip(heads, results) for call in ([h + tail0, h + tail(r)] if n else [h + tail0])])
        for r in results:
            assert type(r) is V.VoxelGridData
            shaped(r.points, (n, 3), np.float32), shaped(r.colors, (n, 3), np.float32)
    np.testing.assert_array_equal(vol._lib.peeked[0][1], [0, 1, 2, 3, 4, 5])
    vol._lib.script("hv_get_voxels", 3)
    shaped(vol.get_points(), (3, 3), np.float32), shaped(vol.get_colors(), (3, 3), np.float32)
    assert [(n, norm(a[1]), norm(a[2])) for n, a in vol._lib.calls] == [("hv_get_voxels", ("int", 1), ("float", 0.0))] * 4
    vol._lib.calls = []
    vol._lib.script("hv_size", 17)
    assert vol.remove_low_count_voxels(3) is None and vol.remove_low_confidence_voxels(0.5) is None and vol.clear() is None
    assert vol.reset() is None and vol.size() == 17 and vol.get_total_voxel_count() == 17 and vol.get_block_size() == 8
    assert vol.set_owner(1, 4) is None and vol.empty() is True
    vol._lib.script("hv_num_blocks", 2)
    assert vol.empty() is False
    expect(vol, ("hv_remove_low_count_voxels", 3), ("hv_reset",), ("hv_reset",), ("hv_size", REF(I64)), ("hv_size", REF(I64)),
           ("hv_set_owner", 1, 4), ("hv_num_blocks", REF(I64)), ("hv_num_blocks", REF(I64)))
    keys, hashes, counts, sums = vol.dump()
    expect(vol, ("hv_num_blocks", REF(I64)), ("hv_dump_blocks", P(keys), P(hashes), P(counts), P(sums), REF(I64)))
    shaped(keys, (2, 3), np.int32), shaped(hashes, (2,), np.uint64), shaped(counts, (2, 512), np.int32), shaped(sums, (2, 512, 6), np.float32)
    pts = np.zeros((5, 3), np.float32)
    vk, bk, lk, h = vol.keys_from_points(pts)
    expect(vol, ("hv_keys_from_points", P(pts), 5, P(vk), P(bk), P(lk), P(h)))
    shaped(vk, (5, 3), np.int32), shaped(bk, (5, 3), np.int32), shaped(lk, (5, 3), np.int32), shaped(h, (5,), np.uint64)


# ---- VoxelBlockSemanticGrid ---------------------------------------------------------------------------------------------------
def sem():
    return volume(S.VoxelBlockSemanticGrid, voxel_size=0.05, block_size=8)


@covers("integrate", "integrate_segment", "integrate_rgbd", "set_depth_threshold", "set_depth_decay_rate")
def test_semantic_integrate(host):
    rng = np.random.default_rng(3)
    p32, p64 = rng.random((5, 3)).astype(np.float32), rng.random((5, 3))
    c8, c32 = rng.integers(0, 256, (5, 3)).astype(np.uint8), rng.random((5, 3)).astype(np.float32)
    cls, inst, dep = np.arange(5, dtype=np.int32), np.arange(5, dtype=np.int32) + 7, rng.random(5).astype(np.float32)
    vol = sem()
    name = "hv_integrate_points_semantic"
    for pts, pdt in ((p32, 0), (p64, 1)):
        p = host(pts)
        vol.integrate(p), vol.integrate(p, host(c8), host(cls)), vol.integrate(p, host(c32), host(cls), host(inst), host(dep))
        expect(vol, (name, P(p), pdt, 5, None, L.HV_COLOR_NONE, None, None, None, L.HV_HOST),
               (name, P(p), pdt, 5, P(c8), L.HV_COLOR_U8, P(cls), None, None, L.HV_HOST),
               (name, P(p), pdt, 5, P(c32), L.HV_COLOR_F32, P(cls), P(inst), P(dep), L.HV_HOST))
    assert vol.integrate(host(p32[:0])) is None
    expect(vol)
    for message, make in POINT_REFUSALS:
        p, c = make(p32, c8)
        refused(vol, RuntimeError, message, vol.integrate, host(p), None if c is None else host(c))
    refused(vol, RuntimeError, "Colors must be uint8 or float32, got dtype with float64", vol.integrate, host(p32), host(p64))
    refused(vol, RuntimeError, "points and class_ids must have the same size", vol.integrate, host(p32), None, host(cls[:-1].copy()))
    refused(vol, RuntimeError, "points and instance_ids must have the same size", vol.integrate, host(p32), None, host(cls), host(inst[:-1].copy()))
    refused(vol, RuntimeError, "points and depths must have the same size", vol.integrate, host(p32), None, None, None, host(dep[:-1].copy()))
    refused(vol, RuntimeError, "instance_ids but no class_ids is not supported", vol.integrate, host(p32), None, None, host(inst))
    vol._lib.script(name, peek={6: (np.int32, 5), 7: (np.int32, 5)})
    vol.integrate_segment(host(p32), host(c8), 4, 2)
    expect(vol, (name, P(p32), 0, 5, P(c8), L.HV_COLOR_U8, ANY, ANY, None, L.HV_HOST))
    assert vol._lib.peeked[0][6].tolist() == [2] * 5 and vol._lib.peeked[0][7].tolist() == [4] * 5
    assert vol.integrate_segment(host(p32), host(c8), -1, 2) is None and vol.integrate_segment(host(p32), host(c8), 4, -1) is None
    vol.set_depth_threshold(0.2), vol.set_depth_decay_rate(3)
    expect(vol, ("hv_set_depth_threshold", 0.2), ("hv_set_depth_decay_rate", 3.0))
    depth, color = frames()
    labels, objects = np.zeros((IH, IW), np.int32), np.ones((IH, IW), np.int32)
    T = pose(1)
    big = float(np.finfo(np.float32).max)
    vol._lib.script("hv_integrate_rgbd_semantic", peek={7: (np.float64, 4)})
    vol.integrate_rgbd(host(depth), host(color), 8.0, 7.0, 3.3, 4.1, T)
    vol.integrate_rgbd(host(depth), host(color), 8.0, 7.0, 3.3, 4.1, T, host(labels), host(objects), max_depth=4, min_depth=1, use_depths=False)
    expect(vol, ("hv_integrate_rgbd_semantic", P(depth), P(color), None, None, IH, IW, ANY, P(T), 0.0, big, 1, L.HV_HOST),
           ("hv_integrate_rgbd_semantic", P(depth), P(color), P(labels), P(objects), IH, IW, ANY, P(T), 1.0, 4.0, 0, L.HV_HOST))
    np.testing.assert_array_equal(vol._lib.peeked[-1][7], [8.0, 7.0, 3.3, 4.1])
    refused(vol, RuntimeError, "depth and colour image sizes differ", vol.integrate_rgbd, host(depth), host(color[:-1].copy()), 8.0, 7.0, 3.3, 4.1, T)
    refused(vol, RuntimeError, "depth and class_ids image sizes differ", vol.integrate_rgbd, host(depth), host(color), 8.0, 7.0, 3.3, 4.1, T,
            host(labels[:-1].copy()))
    refused(vol, RuntimeError, "depth and object_ids image sizes differ", vol.integrate_rgbd, host(depth), host(color), 8.0, 7.0, 3.3, 4.1, T,
            None, host(labels[:, :-1].copy()))


@covers("get_voxels", "get_voxels_in_bb", "get_voxels_in_camera_frustrum", "get_class_segments", "get_points", "get_colors", "get_ids",
        "get_object_segments")
def test_semantic_queries():
    vol = sem()
    f = frustum()
    bba = np.arange(6, dtype=np.float64)
    tail0 = (None, None, None, None, None, 0, REF(I64))

    def tail(r, sem_too=True):
        return (P(r.points), P(r.colors)) + ((P(r.class_ids), P(r.object_ids), P(r.confidences)) if sem_too else (ANY, ANY, ANY)) + (3, REF(I64))

    for n in (3, 0):
        for name in ("hv_get_voxels_semantic", "hv_get_voxels_semantic_in_bb", "hv_get_voxels_semantic_in_frustum"):
            vol._lib.script(name, n)
        results = [vol.get_voxels(), vol.get_voxels(2, 0.5), vol.get_voxels_in_bb(bba, 2, include_semantics=True), vol.get_voxels_in_bb(bba),
                   vol.get_voxels_in_camera_frustrum(f, 3, 0.25, True), vol.get_voxels_in_camera_frustrum(f)]
        heads = [("hv_get_voxels_semantic", 1, 0.0), ("hv_get_voxels_semantic", 2, 0.5), ("hv_get_voxels_semantic_in_bb", P(bba), 2, 0.0),
                 ("hv_get_voxels_semantic_in_bb", P(bba), 1, 0.0),
                 ("hv_get_voxels_semantic_in_frustum", P(f.intr), IW, IH, P(f.T_cw), 5.0, f.depth_min, 3, 0.25),
                 ("hv_get_voxels_semantic_in_frustum", P(f.intr), IW, IH, P(f.T_cw), 5.0, f.depth_min, 1, 0.0)]
        stripped = (False, False, False, True, False, True)
        expect(vol, *[call for h, r, s in zip(heads, results, stripped) for call in ([h + tail0, h + tail(r, not s)] if n else [h + tail0])])
        for r, s in zip(results, stripped):
            assert type(r) is V.VoxelGridData
            shaped(r.points, (n, 3), np.float64), shaped(r.colors, (n, 3), np.float32)
            m = 0 if s else n
            shaped(r.class_ids, (m,), np.int32), shaped(r.object_ids, (m,), np.int32), shaped(r.confidences, (m,), np.float32)
    vol._lib.script("hv_get_voxels_semantic", 3)
    shaped(vol.get_points(), (3, 3), np.float64), shaped(vol.get_colors(), (3, 3), np.float32)
    cls, obj = vol.get_ids()
    shaped(cls, (3,), np.int32), shaped(obj, (3,), np.int32)
    g = vol.get_class_segments(4, 0.5)
    assert type(g) is S.ClassDataGroup and len(g) == 1 and g[0].class_id == 0 and g[0].points.shape == (3, 3)
    assert [(n, norm(a[1]), norm(a[2])) for n, a in vol._lib.calls] == [("hv_get_voxels_semantic", ("int", 1), ("float", -1.0))] * 6 + \
        [("hv_get_voxels_semantic", ("int", 5), ("float", 0.5))] * 2
    vol._lib.calls = []
    vol._lib.script("hv_object_segments_compute", 4, 1)
    g = vol.get_object_segments(2, 0.5)
    o, = g.object_vector
    expect(vol, ("hv_object_segments_compute", 2, 0.5, REF(I64), REF(I64)),
           ("hv_object_segments_fetch", P(o.points.base), P(o.colors.base), None, ANY, ANY, ANY))
    assert type(g) is S.ObjectDataGroup and o.points.base.shape == (4, 3) and o.points.base.dtype == np.float64 and o.colors.base.dtype == np.float32
    vol._lib.script("hv_object_segments_compute", 0, 0)
    assert vol.get_object_segments().object_vector == []
    expect(vol, ("hv_object_segments_compute", 1, 0.0, REF(I64), REF(I64)))


@covers("assoc_vote", "assoc_pairs", "assoc_set_pairs", "assoc_decide", "assign_object_ids_to_instance_ids", "assoc_pairs_export",
        "assoc_pairs_import")
def test_semantic_association(host):
    torch = pytest.importorskip("torch")
    vol = sem()
    f = frustum()
    depth, _ = frames()
    cls, inst = np.zeros((IH, IW), np.int32), np.ones((IH, IW), np.int32)
    c, i, d = host(cls), host(inst), host(depth)
    head = (P(f.intr), IW, IH, P(f.T_cw), 5.0, f.depth_min, P(cls), P(inst))
    assert vol.assoc_vote(f, c, i) is True and vol.assoc_vote(f, c, i, d, 0.3, True) is True
    assert vol.assoc_vote(f, c, i, host(depth[:-1].copy())) is True  # a depth image of another size: no depth filter
    expect(vol, ("hv_assoc_vote",) + head + (None, 0.1, 0, L.HV_HOST), ("hv_assoc_vote",) + head + (P(depth), 0.3, 1, L.HV_HOST),
           ("hv_assoc_vote",) + head + (None, 0.1, 0, L.HV_HOST))
    assert vol.assoc_vote(f, None, i) is False and vol.assoc_vote(f, c, None) is False and vol.assoc_vote(f, host(cls[:-1].copy()), i) is False
    assert vol.assoc_vote(f, c, host(inst[:, :-1].copy())) is False and vol.assoc_vote(f, host(cls[:0].copy()), i) is False
    assert vol.assign_object_ids_to_instance_ids(f, None, i) == {}
    expect(vol)
    refused(vol, RuntimeError, "Class ids must be single-channel", vol.assoc_vote, f, host(np.zeros((IH, IW, 3), np.int32)), i)
    refused(vol, RuntimeError, "Instance ids must be single-channel", vol.assoc_vote, f, c, host(np.zeros((IH, IW, 3), np.int32)))
    vol._lib.script("hv_assoc_pairs_fetch", 2)
    keys, counts = vol.assoc_pairs()
    expect(vol, ("hv_assoc_pairs_fetch", None, None, 0, REF(I64)), ("hv_assoc_pairs_fetch", P(keys), P(counts), 2, REF(I64)))
    shaped(keys, (2,), np.uint64), shaped(counts, (2,), np.int32)
    vol._lib.script("hv_assoc_pairs_fetch", 0)
    keys0, counts0 = vol.assoc_pairs()
    expect(vol, ("hv_assoc_pairs_fetch", None, None, 0, REF(I64)))
    shaped(keys0, (0,), np.uint64), shaped(counts0, (0,), np.int32)
    vol.assoc_set_pairs(keys, counts)
    m = vol.assoc_decide()
    expect(vol, ("hv_assoc_pairs_set", P(keys), P(counts), 2), ("hv_assoc_decide", 0.5, 3))
    assert type(m) is S.LazyIdMap and m.on_device_of(vol) and vol._lib.calls == []
    # the next association replaces the map: an unread one that is still held is fetched first
    m2 = vol.assign_object_ids_to_instance_ids(f, c, i, d, 0.3, True, 0.25, 5)
    expect(vol, ("hv_assoc_map_fetch", ANY, ANY, 1 << 16, REF(I64)), ("hv_assoc_vote",) + head + (P(depth), 0.3, 1, L.HV_HOST),
           ("hv_assoc_decide", 0.25, 5))
    assert dict(m) == {} and vol._lib.calls == [] and not m.on_device_of(vol) and m2.on_device_of(vol)
    vol._lib.script("hv_assoc_map_fetch", 2)
    assert dict(m2) == {0: 0} and len(m2) == 1  # (the stand-in leaves the buffers zeroed: two entries with the key 0)
    expect(vol, ("hv_assoc_map_fetch", ANY, ANY, 1 << 16, REF(I64)))
    vol.assoc_vote(f, c, i)  # the map has been read: nothing to fetch
    expect(vol, ("hv_assoc_vote",) + head + (None, 0.1, 0, L.HV_HOST))
    msg, msgs = torch.zeros(9, dtype=torch.int64), torch.zeros(18, dtype=torch.int64)
    vol.assoc_pairs_export(msg), vol.assoc_pairs_import(msgs, 2)
    expect(vol, ("hv_assoc_pairs_export", P(msg), 4), ("hv_assoc_pairs_import", P(msgs), 2, 4))


@covers("remap_instance_ids")
def test_semantic_remap_instance_ids():
    vol = sem()
    img = np.arange(IH * IW, dtype=np.int32).reshape(IH, IW)
    ids = {3: 30, 4: 40}
    vol._lib.script("hv_remap_instance_ids", peek={4: (np.int32, 2), 5: (np.int32, 2)})
    for fn in (lambda: vol.remap_instance_ids(img, ids), lambda: S.remap_instance_ids(img, ids, volume=vol)):
        out = fn()
        expect(vol, ("hv_remap_instance_ids", P(img), IH, IW, ANY, ANY, 2, P(out), L.HV_HOST))
        shaped(out, (IH, IW), np.int32)
        assert vol._lib.peeked[-1][4].tolist() == [3, 4] and vol._lib.peeked[-1][5].tolist() == [30, 40]
    for dt in (np.int8, np.uint8, np.int16, np.uint16):  # the narrower types: looked up as int32, written back in their own type
        out = vol.remap_instance_ids(img.astype(dt), ids)
        expect(vol, ("hv_remap_instance_ids", ANY, IH, IW, ANY, ANY, 2, ANY, L.HV_HOST))
        shaped(out, (IH, IW), dt)
        narrow = img.astype(dt)
        assert vol.remap_instance_ids(narrow, {}) is narrow
    empty = img[:0]
    assert vol.remap_instance_ids(empty, ids).size == 0
    expect(vol)
    vol._lib.script("hv_remap_instance_ids", peek={})
    out = vol.remap_instance_ids(img, {})  # (an empty map and an int32 image: the call is made, with zero entries)
    expect(vol, ("hv_remap_instance_ids", P(img), IH, IW, ANY, ANY, 0, P(out), L.HV_HOST))
    refused(vol, RuntimeError, "Instance ids must be single-channel", vol.remap_instance_ids, np.zeros((IH, IW, 3), np.int32), ids)
    refused(vol, RuntimeError, "Unsupported instance id type", vol.remap_instance_ids, img.astype(np.float32), ids)
    refused(vol, RuntimeError, "Unsupported instance id type", vol.remap_instance_ids, img.astype(np.int64), ids)
    # the map of the volume's last association is used where it lies
    m = vol.assoc_decide()
    vol._lib.calls = []
    out = vol.remap_instance_ids(img, m)
    expect(vol, ("hv_remap_instance_ids_last", P(img), IH, IW, P(out), L.HV_HOST))
    shaped(out, (IH, IW), np.int32)
    assert vol.remap_instance_ids(empty, m).size == 0
    expect(vol)
    refused(vol, RuntimeError, "Instance ids must be single-channel", vol.remap_instance_ids, np.zeros((IH, IW, 3), np.int32), m)
    refused(vol, RuntimeError, "Unsupported instance id type", vol.remap_instance_ids, img.astype(np.float32), m)
    other = sem()  # on another volume the map is an ordinary mapping: fetched from its own volume, sent as lists
    out = other.remap_instance_ids(img, m)
    assert vol._lib.names() == ["hv_assoc_map_fetch"] and other._lib.names() == ["hv_remap_instance_ids"]


@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int16, np.uint16])
def test_narrow_image_through_a_live_lazy_map(dtype):
    """A narrow host image remapped through the map of the volume's last association: looked up as int32 with the device copy of
    the map, written back in the image's own type (before the shared remap body this path raised NameError)."""
    vol = sem()
    m = vol.assoc_decide()
    vol._lib.script("hv_assoc_map_fetch", 1)
    vol._lib.calls = []
    img = np.arange(IH * IW).reshape(IH, IW).astype(dtype)
    out = vol.remap_instance_ids(img, m)
    assert vol._lib.names()[-1] == "hv_remap_instance_ids_last" and "hv_remap_instance_ids" not in vol._lib.names()
    name, args = vol._lib.calls[-1]
    assert [norm(a) for a in args[2:4]] + [norm(args[5])] == [("int", IH), ("int", IW), ("int", L.HV_HOST)]
    shaped(out, (IH, IW), dtype)


@covers("merge_segments", "remove_segment", "remove_low_confidence_segments", "remove_low_count_voxels", "remove_low_confidence_voxels",
        "label_overflows", "prob_nodes_used", "clear", "reset", "size", "get_total_voxel_count", "empty", "get_block_size", "set_owner",
        "dump", "dump2", "dump_marginals")
def test_semantic_housekeeping():
    vol = sem()
    vol._lib.script("hv_size", 17).script("hv_label_overflows", 5).script("hv_prob_nodes_used", 6)
    vol.merge_segments(1, 2), vol.remove_segment(3), vol.remove_low_confidence_segments(2), vol.remove_low_count_voxels(3)
    vol.remove_low_confidence_voxels(1), vol.clear(), vol.reset(), vol.set_owner(1, 4)
    assert (vol.size(), vol.get_total_voxel_count(), vol.label_overflows(), vol.prob_nodes_used(), vol.get_block_size()) == (17, 17, 5, 6, 8)
    assert vol.empty() is True
    expect(vol, ("hv_merge_segments", 1, 2), ("hv_remove_segment", 3), ("hv_remove_low_confidence_segments", 2), ("hv_remove_low_count_voxels", 3),
           ("hv_remove_low_confidence_voxels", 1.0), ("hv_reset",), ("hv_reset",), ("hv_set_owner", 1, 4), ("hv_size", REF(I64)),
           ("hv_size", REF(I64)), ("hv_label_overflows", REF(I64)), ("hv_prob_nodes_used", REF(I64)), ("hv_num_blocks", REF(I64)))
    vol._lib.script("hv_num_blocks", 2)
    keys, ints, pos, col, conf, nlab, labels, logp = vol.dump2(max_labels=3)
    expect(vol, ("hv_num_blocks", REF(I64)),
           ("hv_dump_blocks_semantic2", P(keys), P(ints), P(conf), P(pos), P(col), P(nlab), P(labels), P(logp), 3, REF(I64)))
    shaped(keys, (2, 3), np.int32), shaped(ints, (2, 512, 4), np.int32), shaped(pos, (2, 512, 3), np.float64), shaped(col, (2, 512, 3), np.float32)
    shaped(conf, (2, 512), np.float32), shaped(nlab, (2, 512), np.int32), shaped(labels, (2, 512, 3, 2), np.int32), shaped(logp, (2, 512, 3), np.float32)
    assert len(vol.dump()) == 4
    oc, cc = vol.dump_marginals()
    got = expect(vol, ("hv_num_blocks", REF(I64)), ("hv_dump_blocks_semantic2", ANY, ANY, ANY, ANY, ANY, ANY, ANY, ANY, 7, REF(I64)),
                 ("hv_num_blocks", REF(I64)), ("hv_dump_marginals_semantic", P(oc), P(cc), REF(I64)))
    assert got
    shaped(oc, (2, 512), np.float32), shaped(cc, (2, 512), np.float32)


# ---- the list is complete -----------------------------------------------------------------------------------------------------
NEED_A_DEVICE = {"adopt_torch_stream": "makes a torch CUDA stream", "fuse_keyframe": "takes device-resident images only",
                 "load": "creates a volume (hv_create)", "packed_info": "calls the library's own validator, no volume involved"}


def test_binding_covers_every_public_method():
    """Every public method of the three classes was exercised above, or is named in NEED_A_DEVICE."""
    names = {n for cls in (V.ScalableTSDFVolume, V.VoxelBlockGrid, S.VoxelBlockSemanticGrid) for n in dir(cls)
             if not n.startswith("_") and callable(getattr(cls, n))}
    assert names - set(NEED_A_DEVICE) <= COVERED, sorted(names - set(NEED_A_DEVICE) - COVERED)
    assert COVERED <= names, sorted(COVERED - names)
