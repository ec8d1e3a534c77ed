"""Inputs shared by the CPU and GPU tests of the plane-sweep matcher (tests/mvs_reference.py is the restatement they are held to)."""
import numpy as np

from pyslam_amd.prep import plane_sweep_views
from tests import mvs_reference as mr
from tests import stereo_cases as sc

# (H, W, D): the shapes at which the kernels change form - part of a wave, not a power of two, exactly one wave; several values per
# lane; one row, one column, the census window; one, two and three tiles of the winner kernel
SHAPES = ((37, 83, 16), (37, 83, 48), (37, 83, 64), (19, 70, 128), (19, 70, 256), (1, 50, 16), (50, 1, 16), (7, 9, 16), (3, 257, 16),
          (3, 513, 256))

# the stereo pairs the matcher is anchored to, and the one whose unique winners point left of the image
ANCHOR_CASES = ("stair_D64", "stair_D128", "stair_D256", "left_of_image_maxdiff-1", "starts_7x43")
STEREO_VIEW = np.array([[[1, 0, 0, -1], [0, 1, 0, 0], [0, 0, 1, 0]]], np.float32)  # A = I, b = (-1, 0, 0): u = x - w


def unit_planes(D):
    """min_depth / max_depth with which w_k = k exactly: w0 = 0 and step16 = 1 / 16"""
    kw = dict(min_depth=1.0 / (D - 1), max_depth=np.inf)
    w0, step16 = mr.plane_parameters(num_planes=D, **kw)
    assert w0 == 0 and step16 == np.float32(0.0625), (w0, step16)
    return kw


def stereo_anchor(name):
    """A planted stereo pair as a one-view plane sweep whose cost volume is stereo rule 3's.
    -> (left, right, the stereo parameters, the arguments of multiview_sgm)"""
    left, right, p = sc.planted(name)
    D = p["num_disparities"]
    kw = dict(num_planes=D, p1=p["p1"], p2=p["p2"], uniqueness_ratio=p["uniqueness_ratio"], paths=p["paths"], min_views=1, **unit_planes(D))
    return left, right, {**p, "max_diff": -1}, kw


def shift_view(dx_per_plane, dy_per_plane=0.0, x0=0.0, y0=0.0, dz_per_plane=0.0):
    """u = (x + x0 + w dx) / (1 + w dz), v = (y + y0 + w dy) / (1 + w dz)"""
    return np.array([[1, 0, x0, dx_per_plane], [0, 1, y0, dy_per_plane], [0, 0, 1, dz_per_plane]], np.float32)


def m3_edges():
    """An 8 x 12 image and three views with w_k = k: half-pixel steps to the left (u = x - k / 2: ties at even and odd x, u = -0.5
    and 0), half-pixel steps to the right (u = W - 1 and W - 0.5), and a view whose q_2 = 1 - k / 4 is 0 on plane 4 and negative
    behind it.  -> (ref, sources [3,8,12], views [3,3,4], arguments)"""
    H, W, D = 8, 12, 16
    rng = np.random.default_rng(12)
    ref = sc.smooth_texture(rng, H, W)[..., 0]
    sources = np.stack([np.roll(ref, -1, axis=1), np.roll(ref, 1, axis=1), sc.smooth_texture(rng, H, W)[..., 0]])
    views = np.stack([shift_view(-0.5), shift_view(0.5), shift_view(0.0, dz_per_plane=-0.25)])
    return np.ascontiguousarray(ref), np.ascontiguousarray(sources), views, dict(num_planes=D, uniqueness_ratio=0, **unit_planes(D))


def m4_rounding(N, seed=0):
    """A textured reference and N noisy sources behind integer shifts in different directions: n takes every value 0..N near the
    borders and sum / n every remainder.  -> (ref, sources [N,H,W], views [N,3,4], arguments without min_views)"""
    H, W, D = 10, 30, 16
    rng = np.random.default_rng(100 + 10 * N + seed)
    ref = sc.smooth_texture(rng, H, W)[..., 0]
    steps = ((-1, 0), (1, 0), (-1, 1), (2, -1))[:N]
    sources, views = [], []
    for dx, dy in steps:
        moved = np.roll(ref, (3 * dy, 3 * dx), axis=(0, 1)).astype(np.int32) + rng.integers(-20, 21, ref.shape)  # right at plane 3
        sources.append(np.clip(moved, 0, 255).astype(np.uint8))
        views.append(shift_view(dx, dy))
    return np.ascontiguousarray(ref), np.stack(sources), np.stack(views), dict(num_planes=D, **unit_planes(D))


def m6_one_blind_view():
    """Two views, the second of which looks past the image for every plane: n <= 1 < min_views = 2 everywhere, every cost is 64,
    the winner is plane 0 by rule 5 and unique under uniqueness_ratio = 0 - and rule M6 takes it."""
    left, right = sc.planted_shift(8, 28, 3, seed=2)
    views = np.stack([STEREO_VIEW[0], shift_view(-1.0, x0=-1000.0)])
    return left, np.stack([right, right]), views, dict(num_planes=16, uniqueness_ratio=0, min_views=2, **unit_planes(16))


def textured_views(H, W, D, N, channels=1, seed=0):
    """A textured reference, N pinhole views a small random rotation and translation away, and source images that show the
    reference's texture as the plane D // 3 maps it (over a texture of their own), with a little noise.
    -> (ref, sources [N,H,W(,3)], views [N,3,4], arguments)"""
    rng = np.random.default_rng(seed)
    f = float(max(H, W))
    K = np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    kw = dict(num_planes=D, min_depth=0.5, max_depth=6.0)
    # the motion is sized in pixels, so that a thin image keeps its sources in sight: at the nearest plane a translation moves a
    # pixel by about px along x and py along y (standard deviations), the rotations by half that
    px, py, w_max = min(W / 4.0, 8.0), min(H / 4.0, 5.0), 1.0 / kw["min_depth"]
    T_src = []
    for _ in range(N):
        r = rng.normal(0.0, 1.0, 3) * (py / (2 * f), px / (2 * f), min(py / W, px / H, 0.01))
        R = np.eye(3) + np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
        U, _, Vt = np.linalg.svd(R)
        T = np.eye(4)
        T[:3, :3] = U @ Vt
        T[:3, 3] = rng.normal(0.0, 1.0, 3) * (px / (f * w_max), py / (f * w_max), min(px / W, py / H, 0.02) / w_max)
        T_src.append(T)
    views = plane_sweep_views(K, np.eye(4), K, np.stack(T_src))
    c = 1 if channels == 1 else 3
    ref = sc.smooth_texture(rng, H, W, c)
    w = mr.inverse_depth(*mr.plane_parameters(kw["min_depth"], kw["max_depth"], D), 16 * np.arange(D))
    sources = []
    for v in views:
        img = sc.smooth_texture(rng, H, W, c)
        seen, ur, vr, _, _ = mr.project(v, H, W, w[D // 3:D // 3 + 1])
        ok = seen[..., 0]
        img[vr[..., 0][ok].astype(int), ur[..., 0][ok].astype(int)] = ref[ok]
        noisy = img.astype(np.int32) + rng.integers(-3, 4, img.shape)
        sources.append(np.clip(noisy, 0, 255).astype(np.uint8))
    ref, sources = np.ascontiguousarray(ref), np.ascontiguousarray(np.stack(sources))
    return (ref[..., 0], sources[..., 0], views, kw) if channels == 1 else (ref, sources, views, kw)


# ---- the synthetic room: a reference pose with two earlier poses as sources
TRUTH_CONFIG = "tiny_160x120_2cm"
TRUTH_POSE, TRUTH_SPACING = 150, 10         # the reference pose and the pose spacing of its two sources (i - s, i - 2 s)
# The room's depths span 1.1 .. 4.2 m and the sources stand 0.13 and 0.25 m away: with 32 planes down to 1 m the farther source
# moves about one pixel per plane (fx b / min_depth / (D - 1) = 1.06).  More planes or a shorter baseline give the census less than
# a pixel per plane to tell neighbours by, and fewer valid pixels: spacing 10 with 64 planes measures (0.666, 0.211, 0.486),
# spacing 3 with 64 planes down to 0.6 m (0.644, 0.309, 0.681)
TRUTH_PARAMS = dict(num_planes=32, min_depth=1.0, max_depth=np.inf)
# (share of valid pixels, share of them off by more than one plane step, median error in plane steps) of the restatement
TRUTH_MEASURED = (0.7723, 0.1205, 0.3351)


def synthetic_triple(i=TRUTH_POSE, spacing=TRUTH_SPACING, config=TRUTH_CONFIG):
    """-> (rgb_ref, rgb_sources [2,H,W,3], depth_ref float32, T_ref_cw, T_sources_cw [2,4,4], stream)"""
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD(config, noise=False, invalid_frac=0.0)
    depth, rgb, T = s[i]
    others = [s[i - spacing * k] for k in (1, 2)]
    return rgb, np.stack([o[1] for o in others]), depth, T, np.stack([o[2] for o in others]), s


def truth_figures(index, depth_true, min_depth, max_depth, num_planes):
    """The three figures of the ground-truth check: the share of valid pixels; among valid pixels, the share whose inverse depth is
    off by more than one plane step; the median error in plane steps."""
    w0, step16 = mr.plane_parameters(min_depth, max_depth, num_planes)
    valid = np.asarray(index) >= 0
    got = np.asarray(index).astype(np.float64) / 16.0
    true = (1.0 / np.asarray(depth_true, np.float64) - float(w0)) / (16.0 * float(step16))
    err = np.abs(got - true)[valid]
    return float(valid.mean()), float((err > 1.0).mean()), float(np.median(err))
