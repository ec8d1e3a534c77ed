"""CPU: the numpy restatement of the stereo matcher (tests/stereo_reference.py) - pinned by the golden pair, checked on a planted
shift and against the synthetic scene's true disparity, and rule 10 on planted disparities.

Ground truth (tiny_160x120_2cm, baseline 0.11 m, D = 32, defaults otherwise; true disparity 3.0-12.7 px), the committed restatement,
measured with tools/make_golden_stereo.py:
    pose   valid share   off by > 1 px   median error
       0      0.9330        0.0458         0.220 px
     150      0.9151        0.0587         0.211 px
     300      0.9294        0.0357         0.224 px
"""
import numpy as np
import pytest

from tests import stereo_cases as sc
from tests import stereo_reference as sr

# pose -> (valid share, share of valid, co-visible pixels off by more than 1 px) as measured above
MEASURED = {0: (0.9330, 0.0458), 150: (0.9151, 0.0587), 300: (0.9294, 0.0357)}


def test_restatement_reproduces_the_golden():
    left, right, golden = sc.load_golden()
    assert left.shape == (120, 160) and left.dtype == np.uint8 and golden.dtype == np.int16
    disp, depth = sr.stereo_sgm(left, right, **sc.GOLDEN_PARAMS)
    assert depth is None
    np.testing.assert_array_equal(disp, golden)
    assert (golden >= 0).mean() > 0.9 and set(np.unique(golden[golden < 0])) <= {-16}


@pytest.mark.parametrize("paths", [4, 8])
def test_planted_shift(paths):
    k, D = 11, 32
    left, right = sc.planted_shift(24, 96, k, seed=0)
    disp, _ = sr.stereo_sgm(left, right, num_disparities=D, paths=paths)
    inner = disp[:, k + 4:left.shape[1] - 4].astype(np.int32)
    print("invalid", int((inner < 0).sum()), "largest deviation", int(np.abs(inner - 16 * k).max()))
    assert (inner >= 0).all()
    assert np.abs(inner - 16 * k).max() <= 8  # the largest sub-pixel offset rule 8 can produce


@pytest.mark.parametrize("pose", sc.TRUTH_POSES)
def test_ground_truth(pose):
    left, right, depth, _, s = sc.synthetic_pair(pose)
    disp, _ = sr.stereo_sgm(left, right, **sc.GOLDEN_PARAMS)
    valid, off, median = sc.truth_figures(disp, depth, s.fx, sc.BASELINE)
    print(f"pose {pose}: valid {valid:.4f}, off by > 1 px {off:.4f}, median error {median:.3f} px")
    want_valid, want_off = MEASURED[pose]
    assert valid >= want_valid - 0.05
    assert off <= 1.5 * want_off


def test_synthetic_pair_geometry():
    """The right eye is the left one moved by the baseline along the camera's x axis: a pixel's match lies fx b / z to its left."""
    left, right, depth, T_cw, s = sc.synthetic_pair(0)
    assert left.shape == right.shape == (s.height, s.width, 3) and depth.dtype == np.float32
    np.testing.assert_array_equal(T_cw, s.pose(0))
    np.testing.assert_array_equal(left, s[0][1])  # the stream's own frame: nothing existing changes
    true = s.fx * sc.BASELINE / depth
    y, x = 60, 100
    d = int(round(float(true[y, x])))
    assert np.abs(left[y, x].astype(int) - right[y, x - d].astype(int)).max() <= np.abs(left[y, x].astype(int) - right[y, x].astype(int)).max()


def test_depth_follows_rule_10():
    bf = np.float32(14.4375)
    d16 = np.array([[-16, 0, 1, 16, 17, 48, 100, 163, 800, 4095, 32767, -1]], np.int16)
    got = sr.depth_out(d16, bf)
    want = np.zeros(d16.shape, np.float32)
    for i, d in enumerate(d16[0]):
        if d > 0:
            want[0, i] = (bf * np.float32(16.0)) / np.float32(d)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0, 0] == 0 and got[0, 1] == 0 and got[0, -1] == 0 and got[0, 2] == np.float32(231.0)
    # the cuts: results below min_depth, or above a finite max_depth, become 0; a result equal to a cut stays
    cut = sr.depth_out(d16, bf, min_depth=float(want[0, 8]), max_depth=float(want[0, 4]))
    keep = (want >= want[0, 8]) & (want <= want[0, 4])
    np.testing.assert_array_equal(cut, np.where(keep, want, np.float32(0)))
    assert cut[0, 8] == want[0, 8] and cut[0, 4] == want[0, 4] and cut[0, 3] == 0 and cut[0, 9] == 0
    np.testing.assert_array_equal(sr.depth_out(d16, bf, min_depth=0.0, max_depth=np.inf), want)
    # through the whole matcher: depth is rule 10 of the disparity it returns
    left, right = sc.planted_shift()
    disp, depth = sr.stereo_sgm(left, right, num_disparities=32, bf=bf, min_depth=1.0, max_depth=1.4)
    np.testing.assert_array_equal(depth, sr.depth_out(disp, bf, 1.0, 1.4))
    assert (depth[disp < 0] == 0).all() and (depth > 0).any() and (depth[disp > 0] == 0).any()


def test_subpixel_division_truncates_toward_zero():
    """Rule 8 with a negative numerator: C division, not numpy's floor."""
    S = np.array([[[10, 10, 15, 30]]], np.int32)  # d* = 0 is the smallest best d: no offset at the border
    assert sr.subpixel(S, sr.winner(S))[0, 0] == 0
    S = np.array([[[20, 10, 13, 30]]], np.int32)  # d* = 1: den = 13, num = 7 * 16 + 13 = 125, 125 / 26 = 4
    assert sr.subpixel(S, sr.winner(S))[0, 0] == 16 + 4
    S = np.array([[[13, 10, 20, 30]]], np.int32)  # num = -7 * 16 + 13 = -99, -99 / 26 = -3 (floor would give -4)
    assert sr.subpixel(S, sr.winner(S))[0, 0] == 16 - 3
    S = np.array([[[10, 10, 10, 30]]], np.int32)  # a flat minimum: d* = 0
    assert sr.winner(S)[0, 0] == 0
