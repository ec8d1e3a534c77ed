"""CPU: the numpy restatement of hv_orb_detect / hv_match_descriptors (tests/orb_reference.py) held to planted facts, the generated
pattern header against its generator, rigid_from_matches on a planted motion, and the loop facts of the synthetic room on the
restatement chain (profiles/orb_features/README.md lists the measured counts)."""
import os
import re

import numpy as np
import pytest

from pyslam_amd import features as F
from tests import orb_cases as oc
from tests import orb_reference as R
from tools import gen_orb_pattern as gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_lone_dot_is_found_at_its_pixel_and_a_flat_image_has_none():
    kp, desc = R.detect(oc.dot())
    assert kp.tolist() == [[20, 17, 0, 16 * (100 - 20), 0]] and desc.shape == (1, 32)  # m10 = m01 = 0: bin 0
    for value in (0, 90, 255):
        kp, desc = R.detect(np.full((50, 70), value, np.uint8))
        assert kp.shape == (0, 5) and desc.shape == (0, 32)
    assert R.orientation_bin(0, 0) == 0


def test_the_header_is_what_the_generator_gives():
    text = open(os.path.join(ROOT, "pyslam_amd", "csrc", "orb_pattern.h")).read()

    def numbers(name):
        body = re.search(r"\b%s\b[^=]*=\s*\{(.*?)\};" % name, text, flags=re.S).group(1)
        return [int(v) for v in re.findall(r"-?\d+", body)]

    pat = gp.pattern()
    gp.validate(pat, gp.rotated(pat))
    assert int(re.search(r"#define HV_ORB_PATTERN_SEED (\d+)", text).group(1)) == gp.SEED
    assert numbers("hv_orb_pattern") == [v for p in pat for v in p]
    assert numbers("hv_orb_pattern_rotated") == [v for rows in gp.rotated(pat) for p in rows for v in p]
    cx, cy = gp.direction_tables()
    assert numbers("hv_orb_cx") == cx and numbers("hv_orb_cy") == cy
    assert cx[:9] == [1024, 1004, 946, 851, 724, 569, 392, 200, 0] and cy[:9] == cx[8::-1]
    # the restatement reads the same generator
    assert R.PATTERN.tolist() == [list(p) for p in pat] and R.CX.tolist() == cx and R.CY.tolist() == cy


def test_a_quarter_turn_of_the_image_moves_every_bin_by_8():
    n = 65
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:n, 0:n]
    g = np.zeros((n, n))
    for _ in range(25):
        cy, cx, s, a = rng.uniform(0, n), rng.uniform(0, n), rng.uniform(2, 7), rng.uniform(40, 200)
        g += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    g = np.clip(g, 0, 255).astype(np.int32)
    turned = np.rot90(g, k=-1)  # the pixel at (x, y) goes to (n - 1 - y, x): (dx, dy) -> (-dy, dx)
    bins = set()
    for y in range(16, n - 16, 3):
        for x in range(16, n - 16, 3):
            b = R.orientation_bin(*R.moments(g, x, y))
            assert R.orientation_bin(*R.moments(turned, n - 1 - y, x)) == (b + 8) % 32, (x, y)
            bins.add(b)
    assert len(bins) > 8


def test_the_orientation_tie_takes_the_smaller_bin():
    img = oc.orientation_tie()
    y, x = oc.TIE_CENTRE
    m10, m01 = R.moments(R.grey(img), x, y)
    assert (m10, m01) == (2000, 200)
    scores = m10 * R.CX + m01 * R.CY
    assert scores[0] == scores[1] == scores.max() and (scores[2:] < scores[0]).all()  # the tie really occurs
    kp, _ = R.detect(img, levels=1)
    assert kp[(kp[:, 0] == x) & (kp[:, 1] == y)][:, 4].tolist() == [0]


def test_suppression_selection_and_order():
    kp, _ = R.detect(oc.adjacent_pair(), levels=1)
    assert kp[:, :2].tolist() == [[22, 20]]  # F5: of two equal neighbours the earlier one
    kp, _ = R.detect(oc.periodic(), levels=1)
    inner = kp[(kp[:, 0] // 32 == 1) & (kp[:, 1] // 32 == 1)]
    assert inner[:, :2].tolist() == [[x, y] for y in (36, 44) for x in (36, 44, 52, 60)]  # F6: equal scores, the smaller indices
    kp, _ = R.detect(oc.shaped(97, 131, 3, seed=7))
    cells = kp[:, 2] * 1000 + (kp[:, 1] // 32) * 10 + kp[:, 0] // 32
    assert (np.diff(cells) >= 0).all() and set(kp[:, 2].tolist()) == {0, 1}  # F7: level, then cell
    for c in np.unique(cells):
        assert (np.diff(kp[cells == c][:, 3]) <= 0).all()  # then the score, descending
    assert R.capacity(97, 131, 3, 8) == (4 * 5 + 2 * 3) * 8 and len(kp) <= R.capacity(97, 131, 3, 8)


def test_matching_rules_on_planted_sets():
    q, t = oc.descriptor_sets(40, 50, seed=9)
    t[30] = t[7] = q[3]
    index, d1, d2, counts = R.match(q, t)
    assert (d1[0, 3], d2[0, 3], index[0, 3]) == (0, 0, -1)  # duplicates in train: d2 == d1 fails the ratio
    assert R.match(q, t, ratio_percent=0)[0][0, 3] == 7  # ... and the smallest index wins
    q[11] = q[3]
    index = R.match(q, t, ratio_percent=0)[0]
    assert index[0, 3] == 7 and index[0, 11] == -1  # duplicate queries: M4 keeps the smaller query index
    assert R.match(q, t, ratio_percent=0, cross_check=0)[0][0, 11] == 7
    index, d1, d2, counts = R.match(q, t, [0, 1, 1, 50])
    assert (d2[0] == 65535).all() and (d1[1] == 65535).all() and (index[1] == -1).all() and counts[1] == 0
    assert counts.tolist() == (index >= 0).sum(axis=1).tolist()
    zeros, ones = np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8)
    assert R.hamming(zeros, ones).tolist() == [[256]] and R.match(zeros, ones, max_distance=256)[0].tolist() == [[0]]
    assert R.match(zeros, ones, max_distance=255)[0].tolist() == [[-1]]


def test_rigid_from_matches_recovers_a_planted_motion_among_outliers():
    rng = np.random.default_rng(5)
    n = 50
    P = rng.uniform(-1, 1, (n, 3)) + [0, 0, 2.5]
    w = np.array([0.2, -0.3, 0.25])
    angle = np.linalg.norm(w)
    k = w / angle
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx
    T[:3, 3] = (0.3, -0.1, 0.2)
    Q = P @ T[:3, :3].T + T[:3, 3] + 0.003 * rng.standard_normal((n, 3))
    bad = rng.choice(n, 20, replace=False)  # 40 % planted outliers
    Q[bad] += rng.uniform(0.3, 1.0, (20, 3)) * rng.choice([-1, 1], (20, 3))
    got, inliers = F.rigid_from_matches(P, Q, 0.02)
    assert inliers.sum() >= 28 and not inliers[bad].any()
    E = np.linalg.inv(T) @ got
    assert np.linalg.norm(E[:3, 3]) < 0.005 and np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1))) < 0.2
    again, inliers2 = F.rigid_from_matches(P, Q, 0.02)
    assert np.array_equal(got, again) and np.array_equal(inliers, inliers2)  # deterministic
    assert F.rigid_from_matches(P[:2], Q[:2], 0.02)[0] is None


def test_backproject_takes_the_nearest_pixel():
    depth = np.zeros((4, 6), np.float32)
    depth[1, 2], depth[2, 3] = 2.0, np.nan
    pts, valid = F.backproject(np.array([[2.4, 0.6], [1.5, 1.0], [3.0, 2.0], [5.6, 1.0], [-0.6, 0.0], [0.0, 0.0]]), depth, (10.0, 20.0, 2.5, 1.5))
    assert valid.tolist() == [True, True, False, False, False, False]  # (1.5 rounds half up to pixel 2)
    np.testing.assert_allclose(pts[0], [(2.4 - 2.5) / 10 * 2, (0.6 - 1.5) / 20 * 2, 2.0])
    assert not pts[2:].any()


@pytest.fixture(scope="module")
def room():
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD("tiny_160x120_2cm")
    out = {}
    for i in (0, 150, 300, 450, 570, 590):
        depth, rgb, T_cw = s[i]
        kp, desc = R.detect(rgb, **oc.LOOP_FEATURES)
        out[i] = (depth, T_cw, R.level0_xy(kp), desc)
    return s.intrinsics, out


def verify(room, source, target):
    """The appearance chain on the restatement: -> (accepted matches, RANSAC inliers, T_target_source or None)"""
    K, frames = room
    (ds, _, xys, descs), (dt, _, xyt, desct) = frames[source], frames[target]
    index = R.match(descs, desct)[0][0]
    hit = index >= 0
    P, okp = F.backproject(xys[hit], ds, K)
    Q, okq = F.backproject(xyt[index[hit]], dt, K)
    T, inliers = F.rigid_from_matches(P[okp & okq], Q[okp & okq], oc.LOOP_PARAMS["inlier_threshold"])
    return int(hit.sum()), int(inliers.sum()), T


@pytest.mark.parametrize("source", [590, 570])
def test_true_revisits_of_the_room_reach_min_inliers(room, source):
    matches, inliers, T = verify(room, source, 0)
    K, frames = room
    E = np.linalg.inv(frames[0][1] @ np.linalg.inv(frames[source][1])) @ T  # against T_target_source of the ground truth
    print(f"\n({source}, 0): {matches} matches, {inliers} inliers, RANSAC pose off by {np.linalg.norm(E[:3, 3]):.3f} m, "
          f"{np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1))):.2f} deg")
    assert inliers >= oc.LOOP_PARAMS["min_inliers"]


@pytest.mark.parametrize("source", [300, 150, 450])
def test_opposite_views_of_the_room_do_not(room, source):
    matches, inliers, _ = verify(room, source, 0)
    print(f"\n({source}, 0): {matches} matches, {inliers} inliers")
    assert inliers < oc.LOOP_PARAMS["min_inliers"]
