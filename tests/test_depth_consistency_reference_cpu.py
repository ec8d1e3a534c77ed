"""The numpy restatement of hv_depth_consistency (tests/depth_consistency_reference.py) on its own: the planted rule edges sit where
they are planted, the random case holds every class at every shape, and on the synthetic room the check does what it is for - it
keeps true depth and removes most of what the plane sweep got wrong.  No GPU; the GPU is held to the restatement bit for bit in
tests/test_gpu_depth_consistency.py."""
import numpy as np
import pytest

from pyslam_amd.prep import consistency_views, plane_sweep_views
from tests import depth_consistency_cases as cc
from tests import depth_consistency_reference as dr
from tests import mvs_cases as mc
from tests import mvs_reference as mr


@pytest.fixture(scope="module")
def room():
    """-> (true depths of TRUTH_POSES, restated plane-sweep depths of TRUTH_POSES, views, back_views of pose 150 to 140 and 130)"""
    s, frames = cc.truth_frames()
    K = s.intrinsics
    raw = [mr.multiview_sgm(rgb, sources, plane_sweep_views(K, T, K, T_src), **mc.TRUTH_PARAMS)[1] for rgb, _, T, sources, T_src in frames]
    views, back_views = consistency_views(K, frames[0][2], K, np.stack([frames[1][2], frames[2][2]]))
    for a in raw:
        a.setflags(write=False)
    return [f[1] for f in frames], raw, views, back_views


@pytest.mark.parametrize("case", cc.planted(), ids=lambda c: c[0])
def test_planted_cases_sit_on_their_edges(case):
    _, depth, sources, views, back_views, kw, check = case
    out, counts, stats, parts = dr.depth_consistency(depth, sources, views, back_views, return_parts=True, **kw)
    check(out, counts, parts)
    assert out.dtype == np.float32 and counts.dtype == np.uint8 and counts.shape == depth.shape + (4,)
    assert stats == (int(parts["valid"].sum()), int((out != 0).sum()), int(counts[..., 0].sum()))


@pytest.mark.parametrize("N", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_random_case_holds_every_class(shape, N):
    depth, sources, views, back_views, *_ = cc.random_case(*shape, N)
    shares = cc.class_shares(depth, sources, views, back_views)
    assert min(shares.values()) >= 0.01, shares
    for bad in cc.BAD_VALUES[1:]:  # (0 is there by construction)
        same = np.isnan(depth) if np.isnan(bad) else depth == np.float32(bad)
        assert same.any() or depth.size < 200, bad
    # the views are inverses of each other: there and back again is the identity on pixels, to rounding
    m, b = views[0].astype(np.float64), back_views[0].astype(np.float64)
    p = np.array([shape[1] / 2.0, shape[0] / 2.0, 1.0])
    q = m[:, :3] @ p + 0.4 * m[:, 3]
    r = b[:, :3] @ (q / q[2]) + (0.4 / q[2]) * b[:, 3]
    np.testing.assert_allclose(r / r[2], p, atol=1e-3)


def test_rules_of_keeping_and_fusing():
    depth, sources, views, back_views, *_ = cc.random_case(37, 83, 3)
    base, counts, _ = dr.depth_consistency(depth, sources, views, back_views, min_consistent=0, max_violations=3, fuse=False)
    valid = dr.is_depth(depth)
    np.testing.assert_array_equal(base, np.where(valid, depth, np.float32(0)))  # nothing asked for: every valid pixel passes unchanged
    assert (counts[~valid] == 0).all() and (counts[..., :3].sum(axis=-1) <= counts[..., 3]).all() and counts[..., 3].max() == 3
    for kw in cc.rule_settings(3):
        out, c, stats = dr.depth_consistency(depth, sources, views, back_views, **kw)
        np.testing.assert_array_equal(c, counts)  # the counts do not depend on C6 and C7
        kept = valid & (counts[..., 0] >= kw["min_consistent"]) & (counts[..., 2] <= kw["max_violations"])
        np.testing.assert_array_equal(out != 0, kept)
        assert stats == (int(valid.sum()), int(kept.sum()), int(counts[..., 0].sum()))
        if not kw["fuse"]:
            np.testing.assert_array_equal(out[kept], depth[kept])
        else:
            alone = kept & (counts[..., 0] == 0)
            np.testing.assert_array_equal(out[alone], depth[alone])  # z / 1
            assert (out[kept & (counts[..., 0] > 0)] != depth[kept & (counts[..., 0] > 0)]).any()


def test_truth_against_truth(room):
    """The true depths of pose 150 against those of poses 140 and 130 with rel_depth_tol = 0.01: measured kept 0.888 of the pixels
    (0.889 are seen by a source), 2 occluded and 24 violated of 19 200 - depth edges, where the nearest source pixel belongs to the
    other surface.  The fused depth stays within the tolerance of the true one: an agreeing view's inverse depth differs by at most
    rel_depth_tol / z, so its depth by at most z tol / (1 - tol), and the mean of such depths with z by no more (measured: 0.0057)."""
    true, _, views, back_views = room
    tol = 0.01
    out, counts, stats = dr.depth_consistency(true[0], true[1:], views, back_views, rel_depth_tol=tol)
    kept, seen = out > 0, counts[..., 3] > 0
    violated, occluded = int((counts[..., 2] > 0).sum()), int((counts[..., 1] > 0).sum())
    deviation = float(np.abs(out[kept].astype(np.float64) / true[0][kept] - 1.0).max())
    print(f"kept {kept.mean():.4f}, seen {seen.mean():.4f}, occluded {occluded}, violated {violated}, largest relative deviation {deviation:.5f}")
    assert kept.mean() >= 0.85
    assert violated <= 0.01 * kept.size
    assert not (kept & ~seen).any()
    np.testing.assert_array_equal(kept, seen & (counts[..., 0] >= 1) & (counts[..., 2] == 0))
    assert deviation <= tol / (1.0 - tol) + 1e-6


def test_check_against_plane_sweep_depth(room):
    """The table of the profile: the plane-sweep depth of pose 150 before the check, after it with fusion and after it without."""
    true, raw, views, back_views = room
    before = cc.depth_figures(raw[0], true[0])
    fused = cc.depth_figures(dr.depth_consistency(raw[0], raw[1:], views, back_views, **cc.TRUTH_CHECK)[0], true[0])
    plain = cc.depth_figures(dr.depth_consistency(raw[0], raw[1:], views, back_views, **{**cc.TRUTH_CHECK, "fuse": False})[0], true[0])
    print("before %.4f %.4f %.4f, fused %.4f %.4f %.4f, not fused %.4f %.4f %.4f" % (before + fused + plain))
    np.testing.assert_allclose(before, mc.TRUTH_MEASURED, atol=1e-3)  # (the index and the depth count a pixel at w <= 0 differently)
    np.testing.assert_allclose(fused, cc.TRUTH_MEASURED, atol=5e-5)
    np.testing.assert_allclose(plain, cc.TRUTH_MEASURED_NOT_FUSED, atol=5e-5)
    # the effect: at most half of the raw share of bad pixels, at least half of the raw valid pixels
    assert fused[1] <= 0.5 * before[1] and plain[1] <= 0.5 * before[1]
    assert fused[0] >= 0.5 * before[0]
    assert fused[2] <= plain[2] <= before[2]
