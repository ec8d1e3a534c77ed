"""CPU: the numpy restatement of the plane-sweep matcher (tests/mvs_reference.py) - anchored to the stereo restatement where the two
must agree, and its own rules (M3's edges, M4's rounding, M6) on planted inputs whose events are counted and asserted."""
import numpy as np
import pytest

from tests import mvs_cases as mc
from tests import mvs_reference as mr
from tests import stereo_reference as sr


@pytest.mark.parametrize("name", mc.ANCHOR_CASES)
def test_stereo_anchor(name):
    """One view with A = I, b = (-1, 0, 0) and w_k = k is a stereo pair: the index equals the disparity without a left-right check,
    except where the winner points left of the image - no view sees it there (M6)."""
    left, right, stereo, kw = mc.stereo_anchor(name)
    index, depth, parts = mr.multiview_sgm(left, [right], mc.STEREO_VIEW, return_parts=True, **kw)
    D = kw["num_planes"]
    np.testing.assert_array_equal(parts["C"], sr.cost_volume(sr.census(sr.grey(left)), sr.census(sr.grey(right)), D))
    disp, _ = sr.stereo_sgm(left, right, **{k: v for k, v in stereo.items() if k not in ("bf", "min_depth", "max_depth")})
    x = np.arange(left.shape[1])[None, :]
    outside = (disp >= 0) & (x - parts["k_star"] < 0)
    print(name, "valid", int((disp >= 0).sum()), "winners left of the image", int(outside.sum()))
    np.testing.assert_array_equal(index, np.where(outside, mr.INVALID, disp))
    if name.startswith("left_of_image"):
        assert outside.sum() >= 1
    # M9 with w_k = k: depth = 16 / k16, 0 at k16 <= 0
    k16 = index.astype(np.float32)
    with np.errstate(divide="ignore"):
        want = np.where(index > 0, np.float32(1.0) / (k16 * np.float32(0.0625)), np.float32(0)).astype(np.float32)
    np.testing.assert_array_equal(depth.view(np.uint32), want.view(np.uint32))


def test_m3_edges():
    ref, sources, views, kw = mc.m3_edges()
    H, W = ref.shape
    D = kw["num_planes"]
    w = np.arange(D, dtype=np.float32)
    left, right, behind = (mr.project(v, H, W, w) for v in views)
    for seen, ur, vr, q2, u in (left, right):
        half = (u - np.floor(u)) == np.float32(0.5)
        inside = half & (u > 0) & (u < W - 1)
        down, up = inside & (np.floor(u) % 2 == 0), inside & (np.floor(u) % 2 == 1)
        assert down.sum() > 0 and up.sum() > 0              # ties at even and at odd x
        assert (ur[down] == np.floor(u)[down]).all() and (ur[up] == np.floor(u)[up] + 1).all() and seen[inside].all()
    seen, ur, _, _, u = left
    at = u == np.float32(-0.5)
    assert at.sum() > 0 and seen[at].all() and (ur[at] == 0).all() and np.signbit(ur[at]).all()  # rintf(-0.5) = -0.0: pixel 0
    assert (u == 0).sum() > 0 and seen[u == 0].all()
    assert (u == np.float32(-1.0)).sum() > 0 and not seen[u == np.float32(-1.0)].any()
    seen, ur, _, _, u = right
    assert (u == W - 1).sum() > 0 and seen[u == W - 1].all()
    at = u == np.float32(W - 0.5)
    assert at.sum() > 0 and (ur[at] == W).all() and not seen[at].any()                          # W - 0.5 = 11.5 -> 12: outside
    seen, _, _, q2, _ = behind
    assert (q2 == 0).sum() == H * W and (q2 < 0).sum() == H * W * (D - 5) and (q2 > 0).sum() == H * W * 4
    assert not seen[q2 <= 0].any() and seen[q2 > 0].any()
    # the whole matcher runs through them (division by zero and NaN included) and never reads outside a source image
    index, depth, parts = mr.multiview_sgm(ref, sources, views, return_parts=True, **kw)
    assert parts["n"].max() == 3 and parts["n"].min() == 0
    assert index.dtype == np.int16 and depth.dtype == np.float32 and np.isfinite(depth).all()
    assert ((index == mr.INVALID) == (depth == 0)).all() or (index == 0).any()  # (plane 0 is w = 0: depth 0 by M9)


@pytest.mark.parametrize("N", [2, 3, 4])
def test_m4_rounding(N):
    ref, sources, views, kw = mc.m4_rounding(N)
    for min_views in range(1, N + 1):
        index, _, parts = mr.multiview_sgm(ref, sources, views, min_views=min_views, return_parts=True, **kw)
        total, n, C = parts["sum"], parts["n"], parts["C"]
        counted = n >= min_views
        assert (C[~counted] == 64).all()
        if min_views > 1:
            assert ((n > 0) & ~counted).sum() > 0  # seen by some views, by too few: 64
        r = (2 * total + n) % np.maximum(2 * n, 1)
        # the remainder has n's parity: its smallest value is sum / n at (even n) or just above (odd n) a half, its largest just below one
        for m in range(max(min_views, 2), N + 1):
            at = counted & (n == m)
            lo, hi = at & (r == m % 2), at & (r == 2 * m - 2 + m % 2)
            assert lo.sum() > 0 and hi.sum() > 0, (N, min_views, m, int(lo.sum()), int(hi.sum()))
            assert (C[lo] == (2 * total[lo] + m) // (2 * m)).all()
            assert (C[lo] * m >= total[lo]).all() and (C[hi] * m <= total[hi]).all()  # rounded up at a half, down below it
        # against exact rational rounding: C = floor(sum / n + 1 / 2)
        want = np.floor(total[counted] / n[counted] + 0.5).astype(np.int32)
        np.testing.assert_array_equal(C[counted], want)
        assert (index >= 0).sum() > 0


def test_m6_takes_a_winner_too_few_views_see():
    left, right, _, kw = mc.stereo_anchor("left_of_image_maxdiff-1")
    index, _, parts = mr.multiview_sgm(left, [right], mc.STEREO_VIEW, return_parts=True, **kw)
    n_star = np.take_along_axis(parts["n"], parts["k_star"][..., None], axis=2)[..., 0]
    unique = sr.unique(parts["S"], parts["k_star"], kw["uniqueness_ratio"])
    assert (unique & (n_star == 0)).sum() >= 1 and (index[unique & (n_star == 0)] == mr.INVALID).all()
    assert (index[unique & (n_star == 1)] >= 0).all() and (unique & (n_star == 1)).sum() > 0
    ref, sources, views, kw = mc.m6_one_blind_view()
    index, depth, parts = mr.multiview_sgm(ref, sources, views, return_parts=True, **kw)
    n_star = np.take_along_axis(parts["n"], parts["k_star"][..., None], axis=2)[..., 0]
    assert (parts["C"] == 64).all() and (parts["k_star"] == 0).all() and sr.unique(parts["S"], parts["k_star"], 0).all()
    assert (n_star == 1).all() and (index == mr.INVALID).all() and (depth == 0).all()
    index, _ = mr.multiview_sgm(ref, sources, views, **{**kw, "min_views": 1})
    assert (index >= 0).sum() > index.size // 2  # the same views with min_views = 1: the first view alone matches


def test_plane_parameters_and_depth():
    w0, step16 = mr.plane_parameters(0.5, 4.0, 64)
    assert w0 == np.float32(0.25) and step16 == np.float32((2.0 - 0.25) / (16.0 * 63))
    w = mr.inverse_depth(w0, step16, 16 * np.arange(64))
    assert w.dtype == np.float32 and w[0] == np.float32(0.25) and abs(float(w[63]) - 2.0) < 1e-6 and (np.diff(w) > 0).all()
    index = np.array([[-16, 0, 16 * 63, 8]], np.int16)
    depth = mr.depth_out(index, w0, step16)
    assert depth[0, 0] == 0 and depth[0, 1] == 4.0 and abs(depth[0, 2] - 0.5) < 1e-6 and 0.5 < depth[0, 3] < 4.0
    assert mr.depth_out(np.array([[0]], np.int16), *mr.plane_parameters(0.5, np.inf, 16))[0, 0] == 0  # w = 0: no depth


def test_plane_sweep_views_project_like_the_cameras():
    """A p + w b, dehomogenised, is where the source camera sees the point at z-depth 1 / w along the reference pixel."""
    from pyslam_amd.prep import plane_sweep_views
    from pyslam_amd.synthetic import trajectory_pose

    K = np.array([[140.0, 0, 79.5], [0, 139.0, 59.5], [0, 0, 1]])
    T_ref, T_a, T_b = (trajectory_pose(i)[0] for i in (150, 144, 138))
    views = plane_sweep_views(K, T_ref, (140.0, 139.0, 79.5, 59.5), np.stack([T_a, T_b]))
    assert views.shape == (2, 3, 4) and views.dtype == np.float32
    rng = np.random.default_rng(0)
    for T_s, m in zip((T_a, T_b), views):
        for _ in range(20):
            x, y, z = rng.uniform(0, 159), rng.uniform(0, 119), rng.uniform(0.5, 5.0)
            X_ref = z * (np.linalg.inv(K) @ np.array([x, y, 1.0]))
            X_src = (T_s @ np.linalg.inv(T_ref) @ np.append(X_ref, 1.0))[:3]
            want = (K @ X_src)[:2] / X_src[2]
            q = m[:, :3].astype(np.float64) @ np.array([x, y, 1.0]) + m[:, 3] / z
            assert np.abs(q[:2] / q[2] - want).max() < 1e-3
    same = plane_sweep_views(K, T_ref, K, T_ref)
    np.testing.assert_allclose(same[0], np.eye(3, 4), atol=1e-6)


def test_ground_truth_figures():
    """The figures that tests/test_gpu_mvs.py asserts on the GPU, measured here with the restatement (which the kernels equal bit
    for bit).  Measured (mvs_cases.TRUTH_MEASURED): valid 0.7723, off by more than a plane step 0.1205, median error 0.335 steps; the
    margins are those of the stereo matcher's ground-truth test."""
    rgb, sources, depth, T_ref, T_src, s = mc.synthetic_triple()
    from pyslam_amd.prep import plane_sweep_views

    views = plane_sweep_views(s.intrinsics, T_ref, s.intrinsics, T_src)
    index, _ = mr.multiview_sgm(rgb, sources, views, **mc.TRUTH_PARAMS)
    valid, off, median = mc.truth_figures(index, depth, mc.TRUTH_PARAMS["min_depth"], mc.TRUTH_PARAMS["max_depth"], mc.TRUTH_PARAMS["num_planes"])
    print(f"valid {valid:.4f}, off by > 1 plane step {off:.4f}, median error {median:.3f} steps")
    assert valid >= mc.TRUTH_MEASURED[0] - 0.05
    assert off <= 1.5 * mc.TRUTH_MEASURED[1]
