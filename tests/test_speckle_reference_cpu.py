"""No GPU: the two restatements of the speckle filter (tests/speckle_reference.py: flood fill and union-find) agree on every planted
case of tests/speckle_cases.py, the small cases give the answers derived by hand below, and every wrong reading in VARIANTS is told
from the right one by the cases named for it in KILLERS."""
import functools
import os

import numpy as np
import pytest

from tests import speckle_cases as pc
from tests import speckle_reference as pr
from tests.speckle_cases import BASE, INV, K, MD, T_H, T_W

CV2_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speckle_opencv.npz")

# variant -> the cases that must each give another image, labelling or count than the right reading
KILLERS = {
    "connect8": ["checkerboard_s1", f"edges_{2 * T_H + 3}x{2 * T_W + 5}_s5_d16"],
    "seed_diff": ["ramp", f"edges_{2 * T_H + 3}x{2 * T_W + 5}_s5_d16"],
    "link_lt": ["diff_threshold", "ramp", "float_depth"],
    "remove_lt": ["size_threshold", "checkerboard_s1", "one_component_removed"],
    "diff_wraps": ["extremes_d65534"],
    "invalid_links": ["near_invalid", "extremes_d65535"],
    "label_largest": ["snake", "edges_1x7_s1_d16"],
    "size_16bit": ["one_component_full_frame"],
}


@functools.lru_cache(maxsize=None)
def answer(name, variant=None, method="flood"):
    image, params = pc.planted(name)
    return pr.filter_speckles(image, variant=variant, method=method, **params)


def apart(a, b):
    return (not pr.same_bits(a.image, b.image) or not np.array_equal(a.labels, b.labels) or a.stats != b.stats
            or (a.depth is not None and not pr.same_bits(a.depth, b.depth)))


def test_the_planted_list():
    names = [c[0] for c in pc.PLANTED]
    assert len(names) == len(set(names)) == 38 + 18
    for name, image, params in pc.PLANTED:
        assert image.dtype in (np.int16, np.float32) and image.ndim == 2 and image.flags.c_contiguous and not image.flags.writeable
    shapes = {c[1].shape for c in pc.PLANTED if c[0].startswith("edges_")}
    assert shapes == {(1, 1), (1, 7), (7, 1), (T_H - 1, T_W + 1), (2 * T_H + 3, 2 * T_W + 5)}
    assert pc.planted("one_component_full_frame")[0].size > 65535
    assert pc.planted("snake")[0].shape == (3 * T_H, 3 * T_W)


@pytest.mark.parametrize("name", [c[0] for c in pc.PLANTED])
def test_flood_fill_and_union_find_agree(name):
    a, b = answer(name), answer(name, method="union")
    assert pr.same_bits(a.image, b.image) and np.array_equal(a.labels, b.labels) and a.stats == b.stats
    if a.depth is not None:
        assert pr.same_bits(a.depth, b.depth)
    image, params = pc.planted(name)
    # what holds for any input: invalid pixels and only they are labelled -1, a label is the index of a pixel labelled with itself,
    # nothing but the removed pixels changes, and the counts add up
    valid = pr.valid_mask(image, params["new_val"])
    assert np.array_equal(a.labels < 0, ~valid)
    flat = a.labels.ravel()
    assert np.array_equal(flat[flat[flat >= 0]], flat[flat >= 0]) and (flat <= np.arange(flat.size)).all()
    gone = valid & ~pr.valid_mask(a.image, params["new_val"])
    assert pr.same_bits(np.where(gone, 0, a.image).astype(image.dtype), np.where(gone, 0, image).astype(image.dtype))
    s = a.stats
    assert s["valid_pixels"] == valid.sum() and s["removed_pixels"] == gone.sum() and s["components"] == np.unique(flat[flat >= 0]).size
    assert s["removed_components"] <= s["components"] and s["largest"] <= s["valid_pixels"]
    if params["max_speckle_size"] == 0:
        assert s["removed_pixels"] == 0 and pr.same_bits(a.image, image)


def test_hand_derived_answers():
    # one pixel
    for name in ("edges_1x1_s0_d0", "edges_1x1_s1_d0"):
        image, params = pc.planted(name)
        r, v = answer(name), int(image[0, 0] != INV)
        assert pr.stats_tuple(r.stats) == (v, v, v, v * params["max_speckle_size"], v * params["max_speckle_size"])
        assert r.labels[0, 0] == (0 if v else -1)
    # blobs of K go, blobs of K + 1 stay, wherever they lie
    image, where = pc.size_threshold()
    r = answer("size_threshold")
    assert pr.stats_tuple(r.stats) == (4 * (2 * K + 1), 8, K + 1, 4, 4 * K)
    for small, large in where.values():
        assert all(r.image[p] == INV for p in small) and all(r.image[p] == BASE for p in large)
        for blob in (small, large):
            assert {int(r.labels[p]) for p in blob} == {min(y * image.shape[1] + x for y, x in blob)}
    # a difference of exactly MD links, MD + 1 does not
    image, pairs = pc.diff_threshold()
    r = answer("diff_threshold")
    assert pr.stats_tuple(r.stats) == (16, 12, 2, 8, 8)
    for p, q, d in pairs:
        assert (r.labels[p] == r.labels[q]) == (d == MD) and (r.image[p] == INV) == (d != MD) and (r.image[q] == INV) == (d != MD)
    # the ramp is one region though its ends are far apart
    r = answer("ramp")
    n = 2 * T_W + 5
    assert pr.stats_tuple(r.stats) == (n, 1, n, 0, 0) and (r.labels == 0).all() and int(r.image[0, -1]) - int(r.image[0, 0]) == MD * (n - 1)
    # diagonals do not link
    board = pc.checkerboard()
    n = int((board != INV).sum())
    assert pr.stats_tuple(answer("checkerboard_s1").stats) == (n, n, 1, n, n) and (answer("checkerboard_s1").image == INV).all()
    assert pr.stats_tuple(answer("checkerboard_s0").stats) == (n, n, 1, 0, 0) and np.array_equal(answer("checkerboard_s0").image, board)
    # the snake, whole, with one pixel raised and with a step in the middle
    image, path = pc.snake()
    n, half = len(path), len(path) // 2
    assert n == (3 * T_H // 2) * 3 * T_W + 3 * T_H // 2 - 1
    assert pr.stats_tuple(answer("snake").stats) == (n, 1, n, 0, 0)
    # one pixel raised: it is a region of its own between two halves that both stay at max_speckle_size = half - 1
    index = lambda p: p[0] * image.shape[1] + p[1]
    r = answer("snake_raised")
    assert n - half - 1 == half and pr.stats_tuple(r.stats) == (n, 3, half, 1, 1) and r.image[path[half]] == INV
    assert r.labels[path[0]] == 0 and r.labels[path[half]] == index(path[half])
    assert r.labels[path[-1]] == min(index(p) for p in path[half + 1:])
    # a step in the middle: two regions of half and half + 1 pixels, max_speckle_size = half takes the first
    r = answer("snake_step")
    assert pr.stats_tuple(r.stats) == (n, 2, n - half, 1, half) and r.labels[path[half - 1]] == 0 and r.image[path[0]] == INV
    assert r.labels[path[half]] == min(index(p) for p in path[half:]) and r.image[path[half]] == BASE + MD + 1
    # the comb is one region
    c = pc.comb()
    n = int((c != INV).sum())
    assert pr.stats_tuple(answer("comb").stats) == (n, 1, n, 1, n) and (answer("comb").image == INV).all()
    # one region: kept at H W - 1, removed at H W
    n = pc.BIG[0] * pc.BIG[1]
    assert pr.stats_tuple(answer("one_component_kept").stats) == (n, 1, n, 0, 0)
    assert pr.stats_tuple(answer("one_component_removed").stats) == (n, 1, n, 1, n)
    n = pc.FULL_FRAME[0] * pc.FULL_FRAME[1]
    assert pr.stats_tuple(answer("one_component_full_frame").stats) == (n, 1, n, 0, 0)
    # int16 extremes: 65535 is a difference like any other
    r = answer("extremes_d65535")
    assert pr.stats_tuple(r.stats) == (3, 1, 3, 0, 0) and r.labels.tolist() == [[0, 0, -1], [0, -1, -1]]
    r = answer("extremes_d65534")
    assert pr.stats_tuple(r.stats) == (3, 2, 2, 1, 1) and r.labels.tolist() == [[0, 1, -1], [0, -1, -1]]
    assert r.image.tolist() == [[-32768, 0, 0], [5, 0, 0]]
    r = answer("extremes_newval_min")
    assert pr.stats_tuple(r.stats) == (5, 2, 4, 1, 1) and r.labels.tolist() == [[-1, 1, 2], [2, 2, 2]]
    assert r.image.tolist() == [[-32768, -32768, 0], [5, 0, 0]]
    r = answer("near_invalid")
    assert pr.stats_tuple(r.stats) == (2, 2, 1, 2, 2) and r.image.tolist() == [[INV, INV, INV]] and r.labels.tolist() == [[0, -1, 2]]
    # float32: NaN and inf are valid and alone, -0.0 is invalid, the seam pair at exactly max_diff links and the next one does not
    image, params = pc.planted("float_depth")
    r = answer("float_depth")
    for p in ((2, 3), (2, 4), (5, 7), (6, 7), (9, 9), (11, 2)):
        assert r.labels[p] == p[0] * image.shape[1] + p[1] and r.image[p] == 0.0 and not np.signbit(r.image[p])
    for p in ((4, 20), (4, 21), (8, 30)):
        assert r.labels[p] == -1 and np.signbit(r.image[p])  # an invalid pixel keeps its bits
    assert r.labels[1, T_W - 1] == r.labels[1, T_W]
    alone = image.copy()
    alone[:3, :], alone[4:, :] = 0.0, 0.0
    alone[3, :T_W - 1], alone[3, T_W + 1:] = 0.0, 0.0
    assert pr.filter_speckles(alone, 0, 0.25).stats["components"] == 2
    # the companion: zeros exactly where pixels went, every other bit kept
    image, params = pc.planted("companion")
    r = answer("companion")
    gone = (image != INV) & (r.image == INV)
    bits, before = r.depth.view(np.uint32), params["depth"].view(np.uint32)
    assert gone.any() and (bits[gone] == 0).all() and np.array_equal(bits[~gone], before[~gone])
    assert (before[~gone] == pc.NAN_PAYLOAD).any() and (before[~gone] == 0x80000000).any() and (before[gone] == pc.NAN_PAYLOAD).any()


def test_every_wrong_reading_has_its_killers():
    assert set(KILLERS) == set(pr.VARIANTS) and len(pr.VARIANTS) == len(set(pr.VARIANTS)) == 8
    assert all(KILLERS.values())


@pytest.mark.parametrize("variant", pr.VARIANTS)
def test_a_named_case_exposes_the_wrong_reading(variant):
    for name in KILLERS[variant]:
        assert apart(answer(name), answer(name, variant)), f"{variant} is not told apart by {name}"


def test_the_controls():
    """Where a wrong reading cannot show: 8-connectivity on a single row, the strict size rule when nothing is removed."""
    assert not apart(answer("ramp"), answer("ramp", "connect8"))
    assert not apart(answer("checkerboard_s0"), answer("checkerboard_s0", "remove_lt"))
    assert not apart(answer("one_component_kept"), answer("one_component_kept", "size_16bit"))  # below 65536 pixels


@pytest.mark.skipif(not os.path.exists(CV2_FIXTURE), reason="tests/golden/speckle_opencv.npz not generated yet (needs cv2: tools/make_golden_speckle.py)")
def test_restatement_matches_opencv_filter_speckles():
    """PIN of rules S1 - S6 - active once tools/make_golden_speckle.py has run where OpenCV exists: cv2.filterSpeckles' image on
    every planted int16 case equals the restatement's (the GPU is held to the restatement bit for bit)."""
    z = np.load(CV2_FIXTURE)
    seen = 0
    for name, image, params in pc.PLANTED:
        if image.dtype == np.int16:
            np.testing.assert_array_equal(answer(name).image, z[name], err_msg=name)
            seen += 1
    assert seen == len(pc.PLANTED) - 1
