"""No GPU: the wrong readings of the stereo matcher (tests/stereo_reference.py, VARIANTS), its event census (events()) and the
planted pairs (tests/stereo_cases.py, PLANTED) checked against each other - every wrong reading is told apart by a named case,
every event that can happen is reached by a named case - and a measurement of what the inputs of the earlier tests could tell.

WHAT THE EARLIER INPUTS TOLD APART.  Those inputs: textured_pair at the nine stereo_cases.SHAPES (one channel, 8 paths), the golden
pair, the constant pair and planted_shift().  Of the 32 wrong readings they tell 19 from the right one (disparity or depth differs
in some pixel).  The 13 they cannot tell: M(q) over the first row of 16 lanes, M(q) without row 1, 2 or 3, both wrap-around
neighbours, rule 6 searched in d < 16, both tile readings of dR, rule 7 without its x - d* < 0 clause, depth cut at <= min_depth,
and the two grey readings (one channel).  "d* searched in d < 16" differs in 2 pixels in all.  With three channels and 4 paths as
well, as tests/test_gpu_stereo.py runs them, 26 of 32: the grey readings, rule 6 in d < 16 (1 pixel), the d-1 wrap-around at d = 0
(6 pixels of three inputs) and, through a single pixel of the 24x40 D = 64 pair with 4 paths, the three readings of M(q) that lose
a row 0..2 join; M(q) without row 3, the d+1 wrap-around, both tile readings, rule 7's clause and the min_depth cut stay untold.
The planted cases tell all 32 (KILLERS below; test_a_named_case_exposes_the_wrong_reading).

EVENTS, counted by events() on the named case (REACHED below holds the same numbers) and over all 23 planted cases:
    event                       named case               there    cases   in all
    m_row0                      stair_D256               64773      23    180221     (m_*: steps q -> p, summed over the paths)
    m_row1                      stair_D256               28588       8     78219
    m_row2                      stair_D256               13804       8     49827
    m_row3                      stair_D128               12722       8     45130
    m_slot0                     stair_D128               54051      23    243718
    m_slot1                     stair_D128               25321       6     49661
    m_slot2                     stair_D256               20981       5     25690
    m_slot3                     stair_D256               30944       5     34328
    valid_row0                  stair_D256                3040      23     14210
    valid_row1                  stair_D256                2115       8      6959
    valid_row2                  stair_D128                1498       7      5043
    valid_row3                  stair_D128                1310       5      4749
    valid_d_ge_16               stair_D128                5494       8     19288
    valid_d0                    stair_D256                 162      17       504
    valid_dlast                 wide_3x513_D16             461       7      2023
    dstar_tie                   equality_u0                  1      12       236
    dr_tie                      wide_3x257_D16               6      13       235
    dr_from_right_tile          wide_3x513_D256            460       6      4699
    unique_rejects              stair_D256                6214      14     12003
    unique_equality             equality_u0, _u20, _u50  1 each      7         7
    winner_left_of_image        left_of_image_maxdiff1       8       3        19
    lr_diff_eq_max              maxdiff3_9x40                1      21      2931
    lr_diff_eq_max_plus_1       maxdiff3_9x40                1      20       375
    subpixel_negative_inexact   stair_D256                2834      23     12199
    depth_eq_min                depth_cuts_9x40              6       1         6
    depth_eq_max                depth_cuts_9x40              4       1         4

UNREACHED: dr_from_left_tile - no input can reach it.  The left pixel x votes for the right pixel xr = x - d with d >= 0, so the
voter never lies in a tile to the left of the right pixel's; with d <= 255 it lies in the same tile or the next one.  (For the
same reason the readings dr_same_tile and dr_without_right_tile lose the same votes; both names stay, one for each way the merge
of the tiles can be written wrong.)  Rule 8's max(den, 1) is no event: for 0 < d* < D-1 it cannot bind, d* being the smallest
minimiser (test_rule_8_denominator_is_positive_inside)."""
import functools

import numpy as np
import pytest

from tests import stereo_cases as sc
from tests import stereo_reference as sr

# the readings that only change rules 5 to 10: they are run on the right reading's S
AFTER_S = {"winner_first_16", "unique_first_16", "dr_same_tile", "dr_without_right_tile", "winner_tie_largest", "dr_tie_largest", "unique_le",
           "unique_gap0", "unique_gap2", "lr_clamped", "lr_strict", "subpixel_floor", "subpixel_at_ends", "depth_min_le", "depth_max_inf"}

# variant -> the cases that must each give another disparity or depth than the right reading
KILLERS = {
    "m_first_16_lanes": ["stair_D64", "stair_D128", "wide_3x513_D256"],
    "m_without_row1": ["stair_D64", "wide_3x257_D256"],
    "m_without_row2": ["stair_D64", "stair_D128"],
    "m_without_row3": ["stair_D64", "stair_D256"],
    "no_lane_neighbours": ["stair_D128", "wide_3x256_D256", "starts_6x41"],
    "below_wraps_at_0": ["stair_D256", "wide_3x257_D256"],
    "above_wraps_at_top": ["stair_D256"],
    "winner_first_16": ["stair_D64", "wide_3x256_D256"],
    "unique_first_16": ["stair_D128", "wide_3x257_D256"],
    "dr_same_tile": ["wide_3x513_D16", "wide_3x513_D256", "wide_3x257_D256"],
    "dr_without_right_tile": ["wide_3x513_D16", "wide_3x513_D256", "wide_3x257_D256"],
    "diagonal_side_starts_zero": ["starts_41x6", "starts_6x41"],
    "last_starts_dropped": ["starts_41x6", "starts_6x41", "starts_5x43", "starts_9x40", "starts_7x43"],
    "winner_tie_largest": ["equality_u0", "wide_3x257_D16"],
    "dr_tie_largest": ["wide_3x256_D16", "wide_2x257_D256_p1023"],
    "unique_le": ["equality_u0", "equality_u20", "equality_u50"],
    "unique_gap0": ["starts_41x6", "equality_u50"],
    "unique_gap2": ["starts_41x6", "equality_u20"],
    "lr_clamped": ["left_of_image_maxdiff1", "wide_2x257_D256_p1023"],
    "lr_strict": ["maxdiff3_9x40", "left_of_image_maxdiff1"],
    "subpixel_floor": ["starts_9x40", "left_of_image_maxdiff-1"],
    "subpixel_at_ends": ["wide_3x256_D16", "equality_u0"],
    "census_le": ["starts_5x43", "equality_u20"],
    "census_zero_border": ["starts_5x43", "starts_41x6"],
    "census_7x9": ["starts_5x43", "starts_41x6"],
    "cost_0_outside": ["starts_41x6", "left_of_image_maxdiff-1"],
    "cost_clamped_outside": ["starts_41x6", "left_of_image_maxdiff-1"],
    "no_minus_m": ["starts_6x41", "wide_3x256_D16"],
    "grey_no_round": ["stair_D64_rgb"],
    "grey_weight_c0": ["stair_D64_rgb"],
    "depth_min_le": ["depth_cuts_9x40"],
    "depth_max_inf": ["depth_cuts_9x40"],
}

# event -> (the named case, the count events() gives there)
REACHED = {
    "m_row0": ("stair_D256", 64773), "m_row1": ("stair_D256", 28588), "m_row2": ("stair_D256", 13804), "m_row3": ("stair_D128", 12722),
    "m_slot0": ("stair_D128", 54051), "m_slot1": ("stair_D128", 25321), "m_slot2": ("stair_D256", 20981), "m_slot3": ("stair_D256", 30944),
    "valid_row0": ("stair_D256", 3040), "valid_row1": ("stair_D256", 2115), "valid_row2": ("stair_D128", 1498), "valid_row3": ("stair_D128", 1310),
    "valid_d_ge_16": ("stair_D128", 5494), "valid_d0": ("stair_D256", 162), "valid_dlast": ("wide_3x513_D16", 461),
    "dstar_tie": ("equality_u0", 1), "dr_tie": ("wide_3x257_D16", 6), "dr_from_right_tile": ("wide_3x513_D256", 460),
    "unique_rejects": ("stair_D256", 6214), "unique_equality": ("equality_u50", 1), "winner_left_of_image": ("left_of_image_maxdiff1", 8),
    "lr_diff_eq_max": ("maxdiff3_9x40", 1), "lr_diff_eq_max_plus_1": ("maxdiff3_9x40", 1),
    "subpixel_negative_inexact": ("stair_D256", 2834), "depth_eq_min": ("depth_cuts_9x40", 6), "depth_eq_max": ("depth_cuts_9x40", 4),
}
UNREACHED = {"dr_from_left_tile"}  # why: the module docstring


@functools.lru_cache(maxsize=None)
def right_volume_of(name):
    left, right, params = sc.planted(name)
    S = sr.volume(left, right, **params)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def events_of(name):
    left, right, params = sc.planted(name)
    return sr.events(left, right, **params)


def outputs(name, variant):
    left, right, params = sc.planted(name)
    S = right_volume_of(name) if variant is None or variant in AFTER_S else sr.volume(left, right, variant=variant, **params)
    return sr.finish(S, variant=variant, **params)


def pixels_apart(a, b):
    return int(((a[0] != b[0]) | (a[1].view(np.uint32) != b[1].view(np.uint32))).sum())


def test_the_planted_list():
    names = [c[0] for c in sc.PLANTED]
    assert len(names) == len(set(names)) == 23 and set(sc.OWN_PATHS) <= set(names)
    for name, left, right, params in sc.PLANTED:
        assert left.dtype == right.dtype == np.uint8 and left.shape == right.shape and left.flags.c_contiguous and right.flags.c_contiguous
        assert params["paths"] in (4, 8) and 0 < params["p1"] <= params["p2"] <= 1023
    assert {(left.shape[1], p["num_disparities"]) for n, left, _, p in sc.PLANTED if n.startswith("wide_3x")} == {
        (W, D) for W in (256, 257, 513) for D in (16, 256)}
    starts = [left.shape for n, left, _, _ in sc.PLANTED if n.startswith("starts_")]
    assert {W % 4 for _, W in starts} == {(H + W - 1) % 4 for H, W in starts} == {0, 1, 2, 3}
    assert (41, 6) in starts and (6, 41) in starts
    assert sc.planted("stair_D64_rgb")[0].ndim == 3
    bits = int(np.float32(sc.BF_24).view(np.uint32))
    assert float(np.float32(sc.BF_24)) == sc.BF_24 and bits & 1  # a float32 number whose last mantissa bit is set


def test_variant_none_is_the_restatement_of_before():
    """stereo_sgm() is volume() then finish(); the golden pair pins the whole (tests/test_stereo_reference_cpu.py)."""
    left, right, params = sc.planted("starts_9x40")
    disp, depth, S = sr.stereo_sgm(left, right, return_volume=True, **params)
    np.testing.assert_array_equal(S, sr.volume(left, right, **params))
    again = sr.finish(S, **params)
    np.testing.assert_array_equal(disp, again[0])
    np.testing.assert_array_equal(depth.view(np.uint32), again[1].view(np.uint32))


def test_every_wrong_reading_has_its_killers():
    assert set(KILLERS) == set(sr.VARIANTS) and len(sr.VARIANTS) == len(set(sr.VARIANTS)) == 32
    assert all(KILLERS.values())


@pytest.mark.parametrize("variant", sr.VARIANTS)
def test_a_named_case_exposes_the_wrong_reading(variant):
    for name in KILLERS[variant]:
        n = pixels_apart(outputs(name, None), outputs(name, variant))
        print(variant, name, n, "pixels apart")
        assert n > 0, f"{variant} is not told apart by {name}"


def test_the_controls():
    """Without the left-right check the missing clause of rule 7 cannot show; the two tile readings lose the same votes."""
    assert pixels_apart(outputs("left_of_image_maxdiff-1", None), outputs("left_of_image_maxdiff-1", "lr_clamped")) == 0
    for name in ("wide_3x513_D16", "wide_3x513_D256", "stair_D256"):
        S = right_volume_of(name)
        np.testing.assert_array_equal(sr.right_volume(S, "dr_same_tile"), sr.right_volume(S, "dr_without_right_tile"))
    # one tile: nothing to lose
    assert pixels_apart(outputs("wide_3x256_D256", None), outputs("wide_3x256_D256", "dr_same_tile")) == 0


def test_every_event_is_reached_by_a_named_case_or_listed_as_unreached():
    assert set(REACHED) | UNREACHED == set(sr.EVENTS) and not set(REACHED) & UNREACHED
    for event, (name, count) in REACHED.items():
        got = events_of(name)[event]
        print(f"{event:28s}{name:26s}{got}")
        assert got == count > 0, (event, name, got, count)
    for u in (0, 20, 50):
        assert events_of(f"equality_u{u}")["unique_equality"] == 1
    for name in ("left_of_image_maxdiff1", "left_of_image_maxdiff-1"):
        assert events_of(name)["winner_left_of_image"] == 8
    for name, _, _, _ in sc.PLANTED:  # unreachable, not merely unreached
        assert all(events_of(name)[e] == 0 for e in UNREACHED), name


def test_path_start_index_counts_every_start_once():
    """The numbering that last_starts_dropped rests on: every start owns one path, a path's pixels follow each other by (dx, dy)."""
    for H, W in ((5, 7), (7, 5), (1, 4), (4, 1), (6, 6)):
        for dx, dy in sr.DIRECTIONS:
            index, n = sr.path_start_index(H, W, dx, dy)
            assert n == (H if dx else 0) + (W - (1 if dx else 0) if dy else 0)
            assert set(index.ravel().tolist()) == set(range(n)) or (dx and dy and min(H, W) == 1)
            for y in range(H):
                for x in range(W):
                    if 0 <= x - dx < W and 0 <= y - dy < H:
                        assert index[y, x] == index[y - dy, x - dx]
            if dx and dy:  # the side column's starts come first, in y
                np.testing.assert_array_equal(index[:, 0 if dx > 0 else W - 1], np.arange(H))


def test_rule_8_denominator_is_positive_inside():
    """d* is the smallest minimiser: S(d*-1) > S(d*) and S(d*+1) >= S(d*), so max(den, 1) never binds for 0 < d* < D-1 and no
    input can plant it."""
    for name in ("stair_D64", "equality_u0", "wide_3x257_D16"):
        S = right_volume_of(name).astype(np.int64)
        d = sr.winner(S)
        inner = (d > 0) & (d < S.shape[2] - 1)
        take = lambda k: np.take_along_axis(S, np.clip(d + k, 0, S.shape[2] - 1)[..., None], axis=2)[..., 0]
        assert inner.any() and ((take(-1) + take(1) - 2 * take(0))[inner] >= 1).all()


# ---- what the inputs of the earlier tests could tell ------------------------------------------------------------------------------
def earlier_inputs():
    for H, W, D in sc.SHAPES:
        left, right = sc.textured_pair(H, W, 1, seed=H * 1000 + W + D)
        yield left, right, dict(num_disparities=D, bf=14.4375, min_depth=0.5, max_depth=6.0)
    left, right, _ = sc.load_golden()
    yield left, right, dict(bf=14.4375, **sc.GOLDEN_PARAMS)
    flat = np.full((21, 70), 117, np.uint8)
    yield flat, flat, dict(num_disparities=32, bf=14.4375)
    yield sc.planted_shift() + (dict(num_disparities=32, bf=14.4375),)


def test_the_earlier_inputs_cannot_tell_the_work_division_readings():
    """The gap the planted cases close, as a measurement: pixels in which each reading differs from the right one, summed over the
    nine SHAPES, the golden, constant and planted_shift pairs."""
    readings = ("m_first_16_lanes", "m_without_row3", "winner_first_16", "dr_same_tile")
    apart = dict.fromkeys(readings, 0)
    for left, right, params in earlier_inputs():
        S = sr.volume(left, right, **params)
        base = sr.finish(S, **params)
        for v in readings:
            Sv = S if v in AFTER_S else sr.volume(left, right, variant=v, **params)
            apart[v] += pixels_apart(base, sr.finish(Sv, variant=v, **params))
    print(apart)
    assert apart == {"m_first_16_lanes": 0, "m_without_row3": 0, "winner_first_16": 2, "dr_same_tile": 0}
