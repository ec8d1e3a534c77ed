"""GPU: ScalableTSDFVolume.track_frame_to_model (hv_tsdf_track) against the numpy restatement of its contract
(tests/track_reference.py) step by step, against the ground truth of the noisy synthetic stream, on the closed-form
plane-and-sphere scene (one unconstrained motion), far from the world origin, and its API promises.

The reference gets, for every traced step, the GPU's own state A, the public ray_cast maps at that level's intrinsics and the same
source depth.  Per pixel the two compute the same float64 operations in the same order, so only the summation order differs.
"""
import numpy as np
import pytest
import torch

from tests import track_reference as tr
from tests import tsdf_closed_form as cf

pytestmark = pytest.mark.gpu

VOXEL, SDF_TRUNC, DEPTH_TRUNC = 0.005, 0.04, 4.0  # == bench.py
ITERATIONS = (10, 5, 4)


def _K(w, h, k):
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    return PinholeCameraIntrinsic(w, h, *k)


def perturbed(T_cw, axis_r, axis_t, deg, metres):
    """The camera moved by `deg` about axis_r and `metres` along axis_t (camera frame)."""
    xi = np.concatenate([np.radians(deg) * np.asarray(axis_r, float) / np.linalg.norm(axis_r),
                         metres * np.asarray(axis_t, float) / np.linalg.norm(axis_t)])
    return np.linalg.inv(np.linalg.inv(T_cw) @ tr.exp_twist(xi))


DIRECTIONS = [((1, 0, 0), (0, 1, 0)), ((0, 1, 1), (1, 0, -1)), ((-1, 1, 0), (1, 1, 1)), ((0, 0, 1), (-1, 1, 0))]


@pytest.fixture(scope="module")
def bench_map():
    """The bench-shaped map: the noisy synthetic 640x480 / 5 mm stream, 64 frames through integrate_batch."""
    from pyslam_amd.synthetic import SyntheticRGBD
    from pyslam_amd.volumetric import ScalableTSDFVolume

    s = SyntheticRGBD("synthetic_640x480_5mm")
    depth, rgb, T = s.batch(0, 64)
    K = _K(s.width, s.height, s.intrinsics)
    vol = ScalableTSDFVolume(VOXEL, SDF_TRUNC, max_blocks=1 << 16)
    vol.integrate_batch(torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda(), K, T, depth_scale=1.0, depth_trunc=DEPTH_TRUNC)
    vol.synchronize()
    return s, vol, K, depth, rgb, T


def test_kernel_matches_reference_step_by_step(bench_map):
    """Every traced step through track_reference.check_call: counts exact, sums within the float64 summation bound, solve,
    schedule and outputs."""
    s, vol, K, depth, _, T = bench_map
    i = 40
    T0 = perturbed(T[i], (1, 1, 0), (0, 1, -1), 2.0, 0.04)
    out = vol.track_frame_to_model(depth[i], K, T0, iterations=ITERATIONS, trace=True)
    assert out.success and len(out.trace) == sum(out.iterations)

    def model(level, Kl, h, w):
        m = vol.ray_cast(_K(w, h, Kl), T0, 0.1, 3.0, 3.0, render_attributes=("depth", "normal", "mask"))
        return m["depth"], m["normal"], m["mask"]

    rep = tr.check_call(out, depth[i], s.intrinsics, T0, model, ITERATIONS)
    print("step by step: %d rows, max xi rel %.3g, pivots near the threshold at %s" % (rep["rows"], rep["xi_rel"], rep["near_pivot"]))
    assert not rep["near_pivot"]


def test_accuracy_against_ground_truth(bench_map):
    """Perturbed starts (2 cm / 1 deg, 5 cm / 3 deg, several directions), the previous frame's pose and the true pose."""
    _, vol, K, depth, _, T = bench_map
    errs = []
    for i in (12, 40):
        for d in DIRECTIONS:
            for deg, metres in ((1.0, 0.02), (3.0, 0.05)):
                out = vol.track_frame_to_model(depth[i], K, perturbed(T[i], *d, deg, metres))
                errs.append(tr.pose_error(out.transformation, T[i]))
                assert out.success and out.fitness > 0.5, (i, d, deg, out)
    for i in (13, 27, 41, 55):
        out = vol.track_frame_to_model(depth[i], K, T[i - 1])
        errs.append(tr.pose_error(out.transformation, T[i]))
    errs = np.array(errs)
    print("perturbed / previous-frame starts: max %.3g m, %.3g deg" % tuple(errs.max(0)))
    assert (errs[:, 0] <= 2e-3).all() and (errs[:, 1] <= 0.1).all(), errs.max(0)
    stay = []
    for i in (12, 40, 63):
        out = vol.track_frame_to_model(depth[i], K, T[i])
        stay.append(tr.pose_error(out.transformation, T[i]))
    stay = np.array(stay)
    print("true-pose starts: max %.3g m, %.3g deg" % tuple(stay.max(0)))
    assert (stay[:, 0] <= 5e-4).all() and (stay[:, 1] <= 0.02).all(), stay.max(0)


def _plane_frames():
    """cf's plane alone, rendered at cf's poses (exact z-depth)."""
    out = []
    fx, fy, cx, cy = cf.K
    v, u = np.mgrid[0:cf.H, 0:cf.W].astype(np.float64)
    for T in cf.POSES:
        T_wc = np.linalg.inv(T)
        d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ T_wc[:3, :3].T
        t = (cf.PLANE_D - T_wc[:3, 3] @ cf.PLANE_N) / (d @ cf.PLANE_N)
        out.append((np.where(t > 0.05, t, 0.0).astype(np.float32), np.zeros((cf.H, cf.W, 3), np.uint8), T))
    return out


def _fused(frames):
    from pyslam_amd.volumetric import RGBDImage, ScalableTSDFVolume

    vol = ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 14)
    for depth, rgb, T in frames:
        vol.integrate(RGBDImage(rgb, depth, 1.0, cf.DEPTH_TRUNC), _K(cf.W, cf.H, cf.K), T)
    return vol


def test_information_has_the_closed_form_null_motion():
    """Plane + sphere: the one unconstrained motion is the rotation about the axis through the sphere centre along the plane normal.
    The fused map's normals are the TSDF's (GetNormalAt), not exact, so that direction is weak rather than null."""
    frames = cf.frames()
    vol = _fused(frames)
    depth, _, T0 = frames[0]
    out = vol.track_frame_to_model(depth, _K(cf.W, cf.H, cf.K), T0, weight_threshold=0.5)
    ev, V = np.linalg.eigh(out.information)
    n_a = T0[:3, :3] @ cf.PLANE_N
    c_a = T0[:3, :3] @ cf.SPHERE_C + T0[:3, 3]
    twist = np.concatenate([n_a, np.cross(c_a, n_a)])
    twist /= np.linalg.norm(twist)
    print("plane + sphere: |cos| %.5f, eigenvalues / largest %s" % (abs(V[:, 0] @ twist), ev / ev[-1]))
    assert abs(V[:, 0] @ twist) >= 0.99
    assert ev[0] < 0.1 * ev[1] and ev[0] < 1e-3 * ev[-1], ev


def test_plane_only_volume_leaves_three_motions_free():
    """One plane: rotation about its normal and the two translations along it are free.  The three weakest eigenvectors of the
    information span that subspace."""
    frames = _plane_frames()
    vol = _fused(frames)
    depth, _, T0 = frames[0]
    out = vol.track_frame_to_model(depth, _K(cf.W, cf.H, cf.K), T0, weight_threshold=0.5)
    ev, V = np.linalg.eigh(out.information)
    n_a = T0[:3, :3] @ cf.PLANE_N
    # constrained: the translation along n and the two rotations about in-plane axes (through the plane's points); the free
    # subspace is orthogonal to t = n, so the weak eigenvectors have no component along (0, n)
    print("plane only: eigenvalues / largest %s, success %s" % (ev / ev[-1], out.success))
    weak = V[:, :3]
    assert np.abs(weak[3:].T @ n_a).max() < 0.05
    assert np.linalg.norm(weak[:3].T @ n_a) > 0.95  # the rotation about n lies in that subspace
    assert ev[2] < 1e-2 * ev[-1], ev


def test_far_from_the_origin_matches_the_origin(bench_map):
    """The world translated by ~(-302, 203, -53) m: the same relative pose as at the origin (the anchor-frame design)."""
    from pyslam_amd.volumetric import ScalableTSDFVolume

    _, _, K, depth, rgb, T = bench_map
    offset = np.array([-301.7, 203.3, -52.9])
    shift = np.eye(4)
    shift[:3, 3] = -offset  # p_world' = p_world + offset  ->  T_cw' = T_cw @ shift
    sl = slice(24, 48)
    res = []
    for sh in (np.eye(4), shift):
        vol = ScalableTSDFVolume(VOXEL, SDF_TRUNC, max_blocks=1 << 16)
        vol.integrate_batch(torch.from_numpy(depth[sl]).cuda(), torch.from_numpy(rgb[sl]).cuda(), K, T[sl] @ sh, depth_scale=1.0,
                            depth_trunc=DEPTH_TRUNC)
        out = vol.track_frame_to_model(depth[36], K, perturbed(T[36], (1, 0, 1), (0, 1, 0), 1.0, 0.02) @ sh)
        assert out.success
        res.append(out.transformation @ np.linalg.inv(sh))
        del vol
    dt, dr = tr.pose_error(res[0], res[1])
    print("far from the origin: %.3g m, %.3g deg" % (dt, dr))
    assert dt <= 5e-4 and dr <= 0.02, (dt, dr)


def test_operands_determinism_and_read_only(bench_map):
    _, vol, K, depth, _, T = bench_map
    u16 = np.round(depth[20] * 5000.0).clip(0, 65535).astype(np.uint16)
    f32 = u16.astype(np.float32) / np.float32(5000.0)
    T0 = perturbed(T[20], (0, 1, 0), (1, 0, 0), 1.0, 0.02)
    d0 = vol.dump()
    m0 = vol.extract_triangle_mesh()
    outs = [vol.track_frame_to_model(f32, K, T0), vol.track_frame_to_model(u16, K, T0, depth_scale=5000.0),
            vol.track_frame_to_model(torch.from_numpy(f32).cuda(), K, T0), vol.track_frame_to_model(f32, K, T0)]
    for o in outs[1:]:
        assert np.array_equal(o.transformation, outs[0].transformation) and np.array_equal(o.information, outs[0].information)
        assert o.fitness == outs[0].fitness and o.inlier_rmse == outs[0].inlier_rmse and o.iterations == outs[0].iterations
    assert outs[0].success
    for a, b in zip(d0, vol.dump()):
        assert np.array_equal(a, b)
    m1 = vol.extract_triangle_mesh()
    for a, b in ((m0.vertices, m1.vertices), (m0.triangles, m1.triangles), (m0.vertex_colors, m1.vertex_colors)):
        assert np.array_equal(a, b)


def test_empty_volume_and_errors():
    from pyslam_amd import _lib as L
    from pyslam_amd.volumetric import ScalableTSDFVolume, VoxelBlockGrid

    depth, _, T0 = cf.frames()[0]
    K = _K(cf.W, cf.H, cf.K)
    empty = ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 10)
    out = empty.track_frame_to_model(depth, K, T0)
    assert not out.success and np.array_equal(out.transformation, T0) and out.fitness == 0.0
    with pytest.raises(L.HipVolError, match="level"):
        empty.track_frame_to_model(depth, K, T0, iterations=())
    with pytest.raises(RuntimeError):
        empty.track_frame_to_model(depth[:, :-1], K, T0)
    sharded = ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 10)
    sharded.set_owner(0, 2)
    with pytest.raises(L.HipVolError, match="whole volume"):
        sharded.track_frame_to_model(depth, K, T0)
    grid = VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12)
    prm, res = L.HvTrackParams(), L.HvTrackResult()
    prm.depth_scale, prm.depth_min, prm.depth_max, prm.weight_threshold = 1.0, 0.1, 3.0, 3.0
    prm.depth_outlier_trunc, prm.depth_huber_delta, prm.n_levels = 0.07, 0.05, 1
    prm.iterations[0] = 1
    d = np.ones((4, 4), np.float32)
    intr = np.array([100.0, 100.0, 2.0, 2.0])
    with pytest.raises(L.HipVolError, match="TSDF"):
        L.check(grid._lib.hv_tsdf_track(grid._h, L.ptr(d), L.HV_DEPTH_F32, 4, 4, L.ptr(intr), L.ptr(np.eye(4)), L.ctypes.byref(prm),
                                        L.ctypes.byref(res), None, 0, None, L.HV_HOST))


def test_track_is_ordered_after_async_integrate():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    frames = cf.frames()
    depth = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    T = np.stack([f[2] for f in frames])
    K = _K(cf.W, cf.H, cf.K)
    T0 = perturbed(T[1], (1, 0, 0), (0, 0, 1), 1.0, 0.02)
    vol = ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 14)
    torch.cuda.synchronize()
    vol.integrate_batch(depth, rgb, K, T, depth_scale=1.0, depth_trunc=cf.DEPTH_TRUNC)
    early = vol.track_frame_to_model(depth[1], K, T0, weight_threshold=0.5)
    vol.synchronize()
    late = vol.track_frame_to_model(depth[1], K, T0, weight_threshold=0.5)
    assert late.success and late.fitness > 0.5
    assert np.array_equal(early.transformation, late.transformation) and early.fitness == late.fitness
