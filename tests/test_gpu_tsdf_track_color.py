"""GPU: hybrid frame-to-model tracking, ScalableTSDFVolume.track_frame_to_model(color=...) (hv_tsdf_track_color): against the numpy
restatement of its contract (tests/track_color_reference.py) step by step, on a fused textured wall where depth alone slides, with
weight 0 against the depth-only call bit for bit, against the ground truth of the synthetic stream, and its API promises.

The restatement, not the kernel, is the yardstick: it gets the GPU's own state A per traced step, the public ray_cast maps (depth,
normal, colour, mask) at that level's intrinsics and the same source frame.  Weight and Huber threshold are passed explicitly
everywhere: no test depends on the defaults.
"""
import numpy as np
import pytest
import torch

from tests import track_color_reference as tc
from tests import track_reference as tr
from tests import tsdf_closed_form as cf

pytestmark = pytest.mark.gpu

VOXEL, SDF_TRUNC, DEPTH_TRUNC = 0.005, 0.04, 4.0  # == bench.py
ITERATIONS = (10, 5, 4)
WEIGHT, DELTA_I = 0.01, 0.1
HYBRID = dict(intensity_weight=WEIGHT, intensity_huber_delta=DELTA_I)
WT = 0.5  # maps of three frames: the weight threshold the closed-form tests use
ATTRS = ("depth", "normal", "color", "mask")


def _K(w, h, k):
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    return PinholeCameraIntrinsic(w, h, *k)


def perturbed(T_cw, axis_r, axis_t, deg, metres):
    """The camera moved by `deg` about axis_r and `metres` along axis_t (camera frame)."""
    xi = np.concatenate([np.radians(deg) * np.asarray(axis_r, float) / np.linalg.norm(axis_r),
                         metres * np.asarray(axis_t, float) / np.linalg.norm(axis_t)])
    return np.linalg.inv(np.linalg.inv(T_cw) @ tr.exp_twist(xi))


def model_of(vol, T0, depth_min=0.1, depth_max=3.0, weight_threshold=3.0):
    def model(level, Kl, h, w):
        m = vol.ray_cast(_K(w, h, Kl), T0, depth_min, depth_max, weight_threshold, render_attributes=ATTRS)
        return m["depth"], m["normal"], m["mask"], m["color"]

    return model


def same(a, b, photometric=True):
    """Bitwise the same call result (the fields a depth-only result has; the photometric ones too where both have them)."""
    assert np.array_equal(a.transformation, b.transformation) and np.array_equal(a.information, b.information)
    assert a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse and a.success == b.success
    assert a.iterations == b.iterations and a.degenerate == b.degenerate and a.inliers == b.inliers and a.valid == b.valid
    if photometric:
        assert a.photometric_inliers == b.photometric_inliers and a.intensity_rmse == b.intensity_rmse


DIRECTIONS = [((1, 0, 0), (0, 1, 0)), ((0, 1, 1), (1, 0, -1)), ((-1, 1, 0), (1, 1, 1)), ((0, 0, 1), (-1, 1, 0))]  # == the depth-only test


@pytest.fixture(scope="module")
def bench_map():
    """The bench-shaped map: the noisy synthetic 640x480 / 5 mm stream, 64 frames through integrate_batch, colour and all."""
    from pyslam_amd.synthetic import SyntheticRGBD
    from pyslam_amd.volumetric import ScalableTSDFVolume

    s = SyntheticRGBD("synthetic_640x480_5mm")
    depth, rgb, T = s.batch(0, 64)
    K = _K(s.width, s.height, s.intrinsics)
    vol = ScalableTSDFVolume(VOXEL, SDF_TRUNC, max_blocks=1 << 16)
    vol.integrate_batch(torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda(), K, T, depth_scale=1.0, depth_trunc=DEPTH_TRUNC)
    vol.synchronize()
    return s, vol, K, depth, rgb, T


# -- 1. step by step -------------------------------------------------------------------------------------------------------------------

def test_kernel_matches_reference_step_by_step(bench_map):
    """Every traced hybrid step through track_color_reference.check_call: counts exact, the combined sums and both squared errors
    within the float64 summation bound, solve, schedule and outputs."""
    s, vol, K, depth, rgb, T = bench_map
    i = 40
    T0 = perturbed(T[i], (1, 1, 0), (0, 1, -1), 2.0, 0.04)
    out = vol.track_frame_to_model(depth[i], K, T0, iterations=ITERATIONS, trace=True, color=rgb[i], **HYBRID)
    assert out.success and len(out.trace) == sum(out.iterations)
    assert out.photometric_inliers > 0.5 * out.inliers, (out.photometric_inliers, out.inliers)
    rep = tc.check_call(out, depth[i], rgb[i], s.intrinsics, T0, model_of(vol, T0), ITERATIONS, lam=WEIGHT, idelta=DELTA_I)
    print("step by step: %d rows, max xi rel %.3g, photometric %d of %d inliers, intensity rmse %.4f, pivots near the threshold at %s"
          % (rep["rows"], rep["xi_rel"], out.photometric_inliers, out.inliers, out.intensity_rmse, rep["near_pivot"]))
    assert not rep["near_pivot"]


# -- 2. the fused textured wall --------------------------------------------------------------------------------------------------------

def texture(p):
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    r = 0.5 + 0.25 * np.sin(9.0 * x + 2.0 * y) + 0.2 * np.sin(5.0 * y - 3.0 * z + 1.0)
    g = 0.5 + 0.25 * np.sin(7.0 * y + 3.0 * z + 0.5) + 0.2 * np.sin(11.0 * x + 0.3)
    b = 0.5 + 0.25 * np.sin(6.0 * x - 8.0 * y + 2.0) + 0.2 * np.sin(4.0 * z + 13.0 * x)
    return np.clip(np.stack([r, g, b], -1), 0.0, 1.0)


def wall_frames(scale):
    """cf's plane alone with the texture, rendered at cf's poses at (cf.W / scale) x (cf.H / scale): [(depth, rgb, T_cw)], K."""
    W, H = cf.W // scale, cf.H // scale
    K = np.array([cf.K[0] / scale, cf.K[1] / scale, (cf.K[2] + 0.5) / scale - 0.5, (cf.K[3] + 0.5) / scale - 0.5])
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for T in cf.POSES:
        T_wc = np.linalg.inv(T)
        d = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1) @ T_wc[:3, :3].T
        t = (cf.PLANE_D - T_wc[:3, 3] @ cf.PLANE_N) / (d @ cf.PLANE_N)
        depth = np.where(t > 0.05, t, 0.0)
        rgb = np.rint(texture(T_wc[:3, 3] + depth[..., None] * d) * 255).astype(np.uint8)
        out.append((depth.astype(np.float32), rgb, T))
    return out, K, W, H


def fused_wall(scale):
    from pyslam_amd.volumetric import RGBDImage, ScalableTSDFVolume

    frames, K, W, H = wall_frames(scale)
    vol = ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 14)
    for depth, rgb, T in frames:
        vol.integrate(RGBDImage(rgb, depth, 1.0, cf.DEPTH_TRUNC), _K(W, H, K), T)
    vol.synchronize()
    return vol, frames, K, W, H


WALL_STARTS = [((0, 0, 1), (1, 0, 0), 1.0, 0.02), ((1, 1, 0), (-1, 1, 0), 2.0, 0.03)]  # both offsets have an in-plane part


@pytest.mark.parametrize("scale", [2, 1], ids=["320x240", "640x480"])
def test_textured_wall_is_tracked_where_depth_only_slides(scale):
    """One fused textured plane, frame 0 tracked from two starts.  Hybrid: success, not degenerate, within the project's tracking
    bound (2e-3 m, 0.1 deg) and at most a tenth of the depth-only error of the same start.  Depth only, on a fused plane, has weak
    rather than null free directions (test_plane_only_volume_leaves_three_motions_free): only its eigenvalues are asserted."""
    vol, frames, K, W, H = fused_wall(scale)
    depth, rgb, T_true = frames[0]
    cam = _K(W, H, K)
    for ar, at, deg, m in WALL_STARTS:
        T0 = perturbed(T_true, ar, at, deg, m)
        plain = vol.track_frame_to_model(depth, cam, T0, weight_threshold=WT, iterations=ITERATIONS)
        e_plain = tr.pose_error(plain.transformation, T_true)
        ev = np.linalg.eigvalsh(plain.information)
        print("wall %dx%d, start %g deg / %g m: depth only success %s degenerate %d, error %.3g m %.3g deg, eigenvalues / largest %s"
              % (W, H, deg, m, plain.success, plain.degenerate, *e_plain, np.array2string(ev / ev[-1], precision=2)))
        assert ev[2] < 1e-2 * ev[-1], ev
        for weight in (0.01, 0.1):
            out = vol.track_frame_to_model(depth, cam, T0, weight_threshold=WT, iterations=ITERATIONS, color=rgb, intensity_weight=weight,
                                           intensity_huber_delta=DELTA_I)
            e = tr.pose_error(out.transformation, T_true)
            evh = np.linalg.eigvalsh(out.information)
            ref = tc.track(depth, rgb, K, T0, model_of(vol, T0, weight_threshold=WT), ITERATIONS, lam=weight, idelta=DELTA_I)
            e_ref = tr.pose_error(ref["T_cw"], T_true)
            print("  hybrid weight %g: success %s degenerate %d iterations %s, error %.3g m %.3g deg (restatement on the same maps: %.3g m "
                  "%.3g deg), photometric %d of %d inliers, intensity rmse %.4f, eigenvalues / largest %s"
                  % (weight, out.success, out.degenerate, out.iterations, *e, *e_ref, out.photometric_inliers, out.inliers,
                     out.intensity_rmse, np.array2string(evh / evh[-1], precision=2)))
            assert out.success and out.degenerate == 0, out
            assert e[0] <= 2e-3 and e[1] <= 0.1, e
            assert e[0] <= 0.1 * e_plain[0], (e, e_plain)


# -- 3. weight 0 is the depth-only tracker ---------------------------------------------------------------------------------------------

def test_weight_zero_is_the_depth_only_call_bit_for_bit(bench_map):
    _, vol, K, depth, rgb, T = bench_map
    for i, d in ((12, DIRECTIONS[0]), (40, DIRECTIONS[2])):
        T0 = perturbed(T[i], *d, 3.0, 0.05)
        plain = vol.track_frame_to_model(depth[i], K, T0, iterations=ITERATIONS, trace=True)
        zero = vol.track_frame_to_model(depth[i], K, T0, iterations=ITERATIONS, trace=True, color=rgb[i], intensity_weight=0.0,
                                        intensity_huber_delta=DELTA_I)
        same(plain, zero, photometric=False)
        assert plain.photometric_inliers is None and plain.intensity_rmse is None
        assert zero.photometric_inliers > 0 and zero.intensity_rmse > 0.0
        assert len(plain.trace) == len(zero.trace)
        for x, y in zip(plain.trace, zero.trace):
            for key in x:
                assert np.array_equal(x[key], y[key]), key
    wall, frames, Kw, W, H = fused_wall(2)
    depth_w, rgb_w, T_true = frames[0]
    for ar, at, deg, m in WALL_STARTS:
        T0 = perturbed(T_true, ar, at, deg, m)
        plain = wall.track_frame_to_model(depth_w, _K(W, H, Kw), T0, weight_threshold=WT, iterations=ITERATIONS)
        zero = wall.track_frame_to_model(depth_w, _K(W, H, Kw), T0, weight_threshold=WT, iterations=ITERATIONS, color=rgb_w,
                                         intensity_weight=0.0, intensity_huber_delta=DELTA_I)
        same(plain, zero, photometric=False)


# -- 4. no harm where geometry suffices ------------------------------------------------------------------------------------------------

def test_accuracy_against_ground_truth_with_colour(bench_map):
    """The starts of the depth-only accuracy test with colour: the bounds that test asserts (2e-3 m, 0.1 deg)."""
    _, vol, K, depth, rgb, T = bench_map
    cases = [(i, perturbed(T[i], *d, deg, metres), "%d %s %g deg" % (i, d, deg)) for i in (12, 40) for d in DIRECTIONS
             for deg, metres in ((1.0, 0.02), (3.0, 0.05))]
    cases += [(i, T[i - 1], "%d from previous" % i) for i in (13, 27, 41, 55)]
    errs, plain_errs = [], []
    for i, T0, name in cases:
        plain = vol.track_frame_to_model(depth[i], K, T0, iterations=ITERATIONS)
        out = vol.track_frame_to_model(depth[i], K, T0, iterations=ITERATIONS, color=rgb[i], **HYBRID)
        errs.append(tr.pose_error(out.transformation, T[i]))
        plain_errs.append(tr.pose_error(plain.transformation, T[i]))
        print("start %s: depth only %.3g m %.3g deg, hybrid %.3g m %.3g deg" % (name, *plain_errs[-1], *errs[-1]))
        assert out.success and out.fitness > 0.5, (name, out)
    errs, plain_errs = np.array(errs), np.array(plain_errs)
    print("hybrid max %.3g m %.3g deg; depth only max %.3g m %.3g deg" % (*errs.max(0), *plain_errs.max(0)))
    assert (errs[:, 0] <= 2e-3).all() and (errs[:, 1] <= 0.1).all(), errs.max(0)


# -- 5. operands and promises ----------------------------------------------------------------------------------------------------------

def test_operands_determinism_and_read_only(bench_map):
    _, vol, K, depth, rgb, T = bench_map
    u16 = np.round(depth[20] * 5000.0).clip(0, 65535).astype(np.uint16)
    f32 = u16.astype(np.float32) / np.float32(5000.0)
    c = rgb[20]
    T0 = perturbed(T[20], (0, 1, 0), (1, 0, 0), 1.0, 0.02)
    kw = dict(iterations=ITERATIONS, **HYBRID)
    d0 = vol.dump()
    m0 = vol.extract_triangle_mesh()
    outs = [vol.track_frame_to_model(f32, K, T0, color=c, **kw),
            vol.track_frame_to_model(u16, K, T0, depth_scale=5000.0, color=c, **kw),
            vol.track_frame_to_model(torch.from_numpy(f32).cuda(), K, T0, color=torch.from_numpy(c).cuda(), **kw),
            vol.track_frame_to_model(torch.from_numpy(f32), K, T0, color=torch.from_numpy(c), **kw),
            vol.track_frame_to_model(f32, K, T0, color=torch.from_numpy(c), **kw),
            vol.track_frame_to_model(f32.astype(np.float64), K, T0, color=np.asfortranarray(c), **kw),
            vol.track_frame_to_model(f32, K, T0, color=c, **kw)]
    for o in outs[1:]:
        same(o, outs[0])
    assert outs[0].success and outs[0].photometric_inliers > 0
    for a, b in zip(d0, vol.dump()):
        assert np.array_equal(a, b)
    m1 = vol.extract_triangle_mesh()
    for a, b in ((m0.vertices, m1.vertices), (m0.triangles, m1.triangles), (m0.vertex_colors, m1.vertex_colors)):
        assert np.array_equal(a, b)
    with pytest.raises(RuntimeError):  # depth on the GPU, colour on the host
        vol.track_frame_to_model(torch.from_numpy(f32).cuda(), K, T0, color=c, **kw)
    with pytest.raises(RuntimeError):
        vol.track_frame_to_model(f32, K, T0, color=c.astype(np.float32), **kw)
    with pytest.raises(RuntimeError):
        vol.track_frame_to_model(f32, K, T0, color=c[:, :-1], **kw)


def test_bgr_order_with_swapped_channels_equals_rgb():
    from pyslam_amd.volumetric import RGBDImage, ScalableTSDFVolume

    frames, K, W, H = wall_frames(2)
    cam = _K(W, H, K)
    T0 = perturbed(frames[0][2], *WALL_STARTS[0])
    outs = []
    for bgr in (False, True):
        vol = ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 14)
        vol.set_color_order(bgr=bgr)
        for depth, rgb, T in frames:
            vol.integrate(RGBDImage(np.ascontiguousarray(rgb[..., ::-1]) if bgr else rgb, depth, 1.0, cf.DEPTH_TRUNC), cam, T)
        depth, rgb, _ = frames[0]
        outs.append(vol.track_frame_to_model(depth, cam, T0, weight_threshold=WT, iterations=ITERATIONS,
                                             color=np.ascontiguousarray(rgb[..., ::-1]) if bgr else rgb, **HYBRID))
    same(outs[0], outs[1])
    assert outs[0].success and outs[0].photometric_inliers > 0


def test_track_is_ordered_after_async_integrate():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    frames, K, W, H = wall_frames(2)
    depth = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    T = np.stack([f[2] for f in frames])
    cam = _K(W, H, K)
    T0 = perturbed(T[1], (1, 0, 0), (0, 0, 1), 1.0, 0.02)
    vol = ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 14)
    torch.cuda.synchronize()
    vol.integrate_batch(depth, rgb, cam, T, depth_scale=1.0, depth_trunc=cf.DEPTH_TRUNC)
    early = vol.track_frame_to_model(depth[1], cam, T0, weight_threshold=WT, color=rgb[1], **HYBRID)
    vol.synchronize()
    late = vol.track_frame_to_model(depth[1], cam, T0, weight_threshold=WT, color=rgb[1], **HYBRID)
    assert late.success and late.fitness > 0.5 and late.photometric_inliers > 0
    same(early, late)


@pytest.mark.parametrize("W,H,iterations", [(9, 1, (4,)), (64, 1, (4,)), (1, 9, (4,)), (1, 64, (4,)), (2, 2, (4,)), (2, 2, (4, 2)),
                                            (7, 5, (4, 3)), (7, 5, (4, 3, 2))], ids=str)
def test_small_images_and_levels_without_gradients(W, H, iterations):
    """Images and pyramid levels narrower or lower than 3 pixels have no photometric term, which is not an error: every row of such a
    level counts 0 photometric inliers, and a call without any is the depth-only call bit for bit.  (At 7x5 the levels above 0 are
    2x3 and 1x1; at level 0 neighbouring pixels of the tilted wall lie further apart in depth than depth_outlier_trunc, so the
    restatement finds no gradient there either.)  Every call is held to the restatement step by step."""
    frames, _, _, _ = wall_frames(1)
    from pyslam_amd.volumetric import RGBDImage, ScalableTSDFVolume

    vol = ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 14)
    for depth, rgb, T in frames:
        vol.integrate(RGBDImage(rgb, depth, 1.0, cf.DEPTH_TRUNC), _K(cf.W, cf.H, cf.K), T)
    K = np.array([cf.K[0] * W / cf.W, cf.K[1] * H / cf.H, cf.K[2] * W / cf.W, cf.K[3] * H / cf.H])
    cam = _K(W, H, K)
    T_true = frames[0][2]
    # the wall seen by the small camera
    T_wc = np.linalg.inv(T_true)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1) @ T_wc[:3, :3].T
    t = (cf.PLANE_D - T_wc[:3, 3] @ cf.PLANE_N) / (d @ cf.PLANE_N)
    depth = np.where(t > 0.05, t, 0.0).astype(np.float32)
    rgb = np.rint(texture(T_wc[:3, 3] + depth.astype(np.float64)[..., None] * d) * 255).astype(np.uint8)
    T0 = perturbed(T_true, (0, 0, 1), (1, 0, 0), 0.5, 0.01)
    out = vol.track_frame_to_model(depth, cam, T0, weight_threshold=WT, iterations=iterations, trace=True, color=rgb, **HYBRID)
    tc.check_call(out, depth, rgb, K, T0, model_of(vol, T0, weight_threshold=WT), iterations, lam=WEIGHT, idelta=DELTA_I)
    for row in out.trace:
        h, w = H >> row["level"], W >> row["level"]
        if h < 3 or w < 3:
            assert row["photometric_inliers"] == 0 and row["sq_intensity_error"] == 0.0, row
    print("%dx%d %s: iterations %s, photometric inliers per row %s" % (W, H, iterations, out.iterations,
                                                                     [r["photometric_inliers"] for r in out.trace]))
    none = all(r["photometric_inliers"] == 0 for r in out.trace)
    assert none or min(W, H) >= 3
    if none:
        plain = vol.track_frame_to_model(depth, cam, T0, weight_threshold=WT, iterations=iterations)
        assert out.photometric_inliers == 0 and out.intensity_rmse == 0.0
        same(plain, out, photometric=False)


def test_empty_volume_and_errors():
    from pyslam_amd import _lib as L
    from pyslam_amd.volumetric import ScalableTSDFVolume, VoxelBlockGrid

    depth, rgb, T0 = cf.frames()[0]
    K = _K(cf.W, cf.H, cf.K)
    empty = ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 10)
    out = empty.track_frame_to_model(depth, K, T0, color=rgb, **HYBRID)
    assert not out.success and np.array_equal(out.transformation, T0) and out.fitness == 0.0
    assert out.photometric_inliers == 0 and out.intensity_rmse == 0.0
    for bad in (dict(intensity_weight=-1e-3), dict(intensity_weight=float("nan")), dict(intensity_weight=float("inf")),
                dict(intensity_huber_delta=0.0), dict(intensity_huber_delta=-0.1), dict(intensity_huber_delta=float("nan"))):
        with pytest.raises(L.HipVolError, match="intensity"):
            empty.track_frame_to_model(depth, K, T0, color=rgb, **dict(HYBRID, **bad))
    with pytest.raises(L.HipVolError, match="level"):
        empty.track_frame_to_model(depth, K, T0, iterations=(), color=rgb, **HYBRID)
    with pytest.raises(L.HipVolError, match="level 0"):
        empty.track_frame_to_model(depth, K, T0, iterations=(0, 3), color=rgb, **HYBRID)
    with pytest.raises(L.HipVolError, match="depth range"):
        empty.track_frame_to_model(depth, K, T0, depth_min=2.0, depth_max=1.0, color=rgb, **HYBRID)
    with pytest.raises(L.HipVolError, match="positive"):
        empty.track_frame_to_model(depth, K, T0, depth_outlier_trunc=0.0, color=rgb, **HYBRID)
    with pytest.raises(L.HipVolError, match="finite"):
        empty.track_frame_to_model(depth, K, np.full((4, 4), np.nan), color=rgb, **HYBRID)
    with pytest.raises(RuntimeError):
        empty.track_frame_to_model(depth[:, :-1], K, T0, color=rgb[:, :-1], **HYBRID)
    sharded = ScalableTSDFVolume(cf.VOXEL, cf.TRUNC, max_blocks=1 << 10)
    sharded.set_owner(0, 2)
    with pytest.raises(L.HipVolError, match="whole volume"):
        sharded.track_frame_to_model(depth, K, T0, color=rgb, **HYBRID)

    grid = VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12)
    prm, res = L.HvTrackColorParams(), L.HvTrackColorResult()
    b = prm.base
    b.depth_scale, b.depth_min, b.depth_max, b.weight_threshold = 1.0, 0.1, 3.0, 3.0
    b.depth_outlier_trunc, b.depth_huber_delta, b.n_levels = 0.07, 0.05, 1
    b.iterations[0] = 1
    prm.intensity_weight, prm.intensity_huber_delta = WEIGHT, DELTA_I
    d = np.ones((4, 4), np.float32)
    c = np.zeros((4, 4, 3), np.uint8)
    intr = np.array([100.0, 100.0, 2.0, 2.0])

    def call(v, depth_p, color_p, dtype=L.HV_DEPTH_F32, loc=L.HV_HOST):
        return v._lib.hv_tsdf_track_color(v._h, depth_p, dtype, color_p, 4, 4, L.ptr(intr), L.ptr(np.eye(4)), L.ctypes.byref(prm),
                                          L.ctypes.byref(res), None, 0, None, loc)

    with pytest.raises(L.HipVolError, match="TSDF"):
        L.check(call(grid, L.ptr(d), L.ptr(c)))
    with pytest.raises(L.HipVolError, match="null"):
        L.check(call(empty, L.ptr(d), None))
    with pytest.raises(L.HipVolError, match="null"):
        L.check(call(empty, None, L.ptr(c)))
    with pytest.raises(L.HipVolError, match="dtype"):
        L.check(call(empty, L.ptr(d), L.ptr(c), dtype=77))
    with pytest.raises(L.HipVolError, match="loc"):
        L.check(call(empty, L.ptr(d), L.ptr(c), loc=77))
    L.check(call(empty, L.ptr(d), L.ptr(c)))
    assert res.base.success == 0 and res.photometric_inliers == 0
