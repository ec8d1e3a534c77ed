"""No GPU: the restatement of hv_remap and the rectify step (tests/remap_reference.py) and the planted cases (tests/remap_cases.py)
checked against each other - the restatement agrees with oracle/host_prep.py wherever both are defined, every named wrong reading of
the contract is told apart by a named case, the cases hold what they promise - and the refusals of VoxelBlockGrid.remap /
ScalableTSDFVolume.remap that happen before the library is called (tests/recording_lib.py)."""
import math
import warnings

import numpy as np
import pytest

from oracle import host_prep as hp
from pyslam_amd import volumetric as V
from tests import remap_cases as rc
from tests import remap_reference as rr
from tests.recording_lib import volume

F32 = np.float32


# ---- the restatement and oracle/host_prep.py -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted({c.family for c in rc.maps()}))
def test_restatement_equals_host_prep(family):
    """Two restatements written apart; host_prep reaches "non-finite is outside" through numpy's cast of NaN / inf to int64."""
    n = 0
    for c in (c for c in rc.maps() if c.family == family):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # numpy: invalid value encountered in cast
            for kind, C in (("u8", 1), ("u8", 3), ("u8", 4), ("f32_special", 1), ("f32_random", 2), ("i32", 1), ("i32", 3), ("u16", 1)):
                img = rc.image(kind, c.H, c.W, C)
                np.testing.assert_array_equal(rr.remap_nearest(img, c.map_x, c.map_y), hp.remap_nearest(img, c.map_x, c.map_y), err_msg=f"{c.name} {kind} {C}")
            for C in (1, 2, 3, 4):
                img = rc.image("u8", c.H, c.W, C)
                np.testing.assert_array_equal(rr.remap_linear_u8(img, c.map_x, c.map_y), hp.remap_linear_u8(img, c.map_x, c.map_y), err_msg=f"{c.name} u8 {C}")
        n += 1
    assert n > 0


# ---- every wrong reading is exposed by a named case ------------------------------------------------------------------------------
def _nearest(kind, C):
    return lambda c, variant: rr.remap_nearest(rc.image(kind, c.H, c.W, C), c.map_x, c.map_y, variant)


def _linear_u8(C):
    return lambda c, variant: rr.remap_linear_u8(rc.image("u8", c.H, c.W, C), c.map_x, c.map_y, variant)


def _linear_f32(C):
    return lambda c, variant: rr.remap_linear_f32(rc.image("f32_exact", c.H, c.W, C), c.map_x, c.map_y, variant)[0]


def _batch(B, u16):
    return lambda c, variant: np.concatenate([a.reshape(-1).astype(np.float64) for a in rr.rectify_frames(*rc.batch(B, c.H, c.W, u16), c.map_x, c.map_y, variant)])


# variant -> [(case, operation)]: every pair must give another result than the right reading
KILLERS = {
    "half_away": [("nearest_ties_5x7", _nearest("u8", 1)), ("linear_ties_5x7", _linear_u8(3)), ("linear_ties_17x31", _linear_f32(1))],
    "floor": [("nearest_ties_5x7", _nearest("f32_random", 1)), ("linear_ties_t_5x7", _linear_u8(1))],
    "trunc": [("nearest_ties_t_17x31", _nearest("i32", 1)), ("linear_ties_5x7", _linear_u8(1))],
    "c_divmod": [("border_5x7", _linear_u8(3)), ("border_17x31", _linear_f32(2)), ("linear_ties_5x7", _linear_u8(1))],
    "border_replicate": [("border_5x7", _nearest("u8", 1)), ("border_1x9", _linear_u8(1)), ("shift_out_x_5x7", _nearest("i32", 1)),
                         ("border_1x1", _linear_f32(1))],
    "w_swapped": [("fxfy_q1_16x16", _linear_u8(1)), ("fxfy_q2_16x16", _linear_f32(1))],
    "xy_swapped": [("permutation_5x7", _nearest("u8", 1)), ("permutation_17x31", _linear_u8(3)), ("identity_1x9", _nearest("i32", 1))],
    "no_half": [("fxfy_q2_16x16", _linear_u8(3)), ("border_5x7", _batch(1, False))],
    "row_stride_H": [("identity_5x7", _nearest("u8", 1)), ("permutation_17x31", _linear_u8(1)), ("identity_9x1", _nearest("f32_exact", 1))],
    "channel_stride_3": [("identity_5x7", _nearest("u8", 2)), ("permutation_5x7", _nearest("i32", 4)), ("fxfy_q0_16x16", _linear_u8(1)),
                         ("fxfy_q0_16x16", _linear_f32(4))],
    "nan_as_zero": [("nonfinite_5x7", _nearest("u8", 1)), ("nonfinite_17x31", _linear_u8(3)), ("nonfinite_1x1", _nearest("i32", 1)),
                    ("nonfinite_5x7", _batch(2, True))],
    "via_float32": [("identity_5x7", _nearest("i32", 1)), ("permutation_1x1", _nearest("i32", 1))],
    "frame0_colour": [("identity_5x7", _batch(2, True)), ("border_5x7", _batch(5, False))],
    "colour_offset_npx": [("identity_5x7", _batch(2, False)), ("permutation_17x31", _batch(5, True))],
}


def test_every_wrong_reading_has_its_killers():
    assert set(KILLERS) == set(rr.VARIANTS)


@pytest.mark.parametrize("variant", rr.VARIANTS)
def test_a_named_case_exposes_the_wrong_reading(variant):
    for name, op in KILLERS[variant]:
        c = rc.case(name)
        right, wrong = op(c, None), op(c, variant)
        assert right.shape == wrong.shape
        assert not np.array_equal(right, wrong, equal_nan=True), f"{variant} is not told apart by {name}"


def test_uint16_survives_float32_but_not_int16():
    """Every uint16 is a float32 number, so the via_float32 reading cannot show on depth; what can go wrong there is a signed
    16-bit intermediate, and the planted depth images hold values it cannot keep."""
    img = rc.image("u16", 5, 7)
    np.testing.assert_array_equal(rr._through_float32(img), img)
    assert (img > 32767).any() and 65535 in img and 32768 in img
    assert (rc.batch(2, 5, 7, True)[0] > 32767).all()


# ---- the cases keep their promises -----------------------------------------------------------------------------------------------
def cases_of(family):
    return [c for c in rc.maps() if c.family == family]


def test_the_list_of_cases_is_what_the_issue_names():
    assert rc.SHAPES == ((1, 1), (1, 9), (9, 1), (5, 7), (16, 16), (1, 257), (17, 31))
    names = [c.name for c in rc.maps()]
    assert len(names) == len(set(names))
    assert {c.family for c in rc.maps()} == {"identity", "shift", "nearest_ties", "linear_ties", "border", "fxfy", "permutation", "nonfinite",
                                            "int32_edge"}
    assert {(c.H, c.W) for c in rc.maps()} == set(rc.SHAPES)
    assert max(c.H * c.W for c in rc.maps()) == 527


def test_identity_shift_and_permutation():
    for c in cases_of("identity"):
        img = rc.image("i32", c.H, c.W, 2)
        np.testing.assert_array_equal(rr.remap_nearest(img, c.map_x, c.map_y), img)
    for c in cases_of("permutation"):
        flat = (np.rint(c.map_y).astype(int) * c.W + np.rint(c.map_x).astype(int)).ravel()
        assert sorted(flat) == list(range(c.H * c.W))
        assert c.H * c.W < 4 or (flat != np.arange(c.H * c.W)).any()
        img = rc.image("u8", c.H, c.W, 3)  # whole pixels: linear is nearest
        np.testing.assert_array_equal(rr.remap_linear_u8(img, c.map_x, c.map_y), rr.remap_nearest(img, c.map_x, c.map_y))
    for name in ("shift_out_x_5x7", "shift_out_y_5x7"):
        c = rc.case(name)
        assert not rr.remap_nearest(rc.image("u8_white", 5, 7), c.map_x, c.map_y).any()
    c = rc.case("shift_in_5x7")
    img = rc.image("u16", 5, 7)
    out = rr.remap_nearest(img, c.map_x, c.map_y)
    np.testing.assert_array_equal(out[1:, :-1], img[:-1, 1:])
    assert not out[0].any() and not out[:, -1].any()


def test_nearest_ties_tie_on_even_and_odd_on_both_sides():
    seen = set()
    for c in cases_of("nearest_ties"):
        for m, n in ((c.map_x, c.W), (c.map_y, c.H)):
            v = m.astype(np.float64).ravel()
            assert (v - np.floor(v) == 0.5).all()
            k = np.floor(v).astype(int)
            seen |= {("even" if kk % 2 == 0 else "odd", "neg" if kk < 0 else "pos") for kk in k}
            if c.H * c.W >= 8:
                assert {-0.5, -1.5, n - 0.5} <= set(v), c.name
    assert seen == {("even", "neg"), ("odd", "neg"), ("even", "pos"), ("odd", "pos")}
    assert rr.round_coord(F32(-0.5)) == 0 and rr.round_coord(F32(-1.5)) == -2 and rr.round_coord(F32(0.5)) == 0 and rr.round_coord(F32(1.5)) == 2


def test_linear_ties_tie_after_the_float32_multiplication():
    seen = set()
    for c in cases_of("linear_ties"):
        for m in (c.map_x, c.map_y):
            for v in m.ravel():
                s = float(rr.mul32(v))  # the float32 product, exactly
                assert s - math.floor(s) == 0.5, (c.name, v)
                k = math.floor(s)
                seen.add(("even" if k % 2 == 0 else "odd", "neg" if k < 0 else "pos"))
                assert rr.round_coord(rr.mul32(v)) == (k if k % 2 == 0 else k + 1)
    assert seen == {("even", "neg"), ("odd", "neg"), ("even", "pos"), ("odd", "pos")}


def _outside_counts(c):
    """Per pixel: how many of the four taps lie outside the image, and how many of those carry a non-zero weight."""
    iy, ix, fy, fx, ok = rr.linear_taps(c.map_x, c.map_y)
    assert ok.all()
    geo, weighted = np.zeros(len(ix), int), np.zeros(len(ix), int)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        out = ~((ix + dx >= 0) & (ix + dx < c.W) & (iy + dy >= 0) & (iy + dy < c.H))
        w = (fx if dx else 32 - fx) * (fy if dy else 32 - fy)
        geo += out
        weighted += out & (w > 0)
    return geo, weighted


def test_border_cases_blend_one_two_and_three_outside_taps():
    """A 2x2 block of taps against a rectangle has 0, 2, 3 or 4 taps outside, never exactly 1 (and 4 needs a coordinate <= -1, which
    is no border fraction) - so "exactly one outside" is planted as it can occur: one of the taps THAT CARRY WEIGHT is outside (a side
    border at a whole row, fy == 0).  Both counts are held."""
    for name in ("border_17x31", "border_16x16", "border_5x7"):
        geo, weighted = _outside_counts(rc.case(name))
        assert set(geo) == {0, 2, 3} and {0, 1, 2, 3} <= set(weighted), name
    for name in ("border_1x9", "border_9x1", "border_1x257"):  # one row or column: two taps are always outside
        geo, weighted = _outside_counts(rc.case(name))
        assert set(geo) == {2, 3} and (name != "border_1x257" or {0, 1, 2, 3} <= set(weighted)), name
    geo, weighted = _outside_counts(rc.case("border_1x1"))
    assert set(geo) == {3}  # the one pixel is the only tap inside
    for c in cases_of("border"):  # coordinates in (-1, 0) and (W-1, W), on each side
        for m, n in ((c.map_x, c.W), (c.map_y, c.H)):
            if c.H * c.W >= 7:
                assert ((m > -1) & (m < 0)).any() and ((m > n - 1) & (m < n)).any(), c.name
    # 255 blended with the border is not 255; 255 blended with 255 is
    c = rc.case("border_5x7")
    out = rr.remap_linear_u8(rc.image("u8_white", 5, 7), c.map_x, c.map_y).ravel()
    geo, weighted = _outside_counts(c)
    assert (out[weighted == 0] == 255).all() and (out[weighted > 0] < 255).all()


def test_fxfy_cases_hold_every_pair_once_with_every_tap_inside():
    pairs = []
    for c in cases_of("fxfy"):
        iy, ix, fy, fx, ok = rr.linear_taps(c.map_x, c.map_y)
        assert ok.all() and ix.min() >= 0 and ix.max() + 1 < c.W and iy.min() >= 0 and iy.max() + 1 < c.H
        pairs += list(zip(fx.tolist(), fy.tolist()))
        for C in (1, 3):
            assert (rr.remap_linear_u8(rc.image("u8_white", 16, 16, C), c.map_x, c.map_y) == 255).all()  # four taps of 255 give 255
    assert sorted(pairs) == [(a, b) for a in range(32) for b in range(32)]


def test_nonfinite_and_edge_cases_hold_every_value_in_x_in_y_and_in_both():
    for family, values in (("nonfinite", rc.NONFINITE), ("int32_edge", rc.EDGE)):
        for c in cases_of(family):
            if c.H * c.W < 3 * len(values):
                continue
            ix, iy = rc._identity(c.H, c.W)
            for v in values:
                hit = lambda m: np.isnan(m) if v != v else m == F32(v)
                bx, by = hit(c.map_x), hit(c.map_y)
                assert (bx & ~by).any() and (by & ~bx).any() and (bx & by).any(), (c.name, v)
            assert (((c.map_x == ix) | (c.map_y == iy))).sum() > 0
    for v in rc.NONFINITE:
        assert rr.round_coord(F32(v)) is None and rr.round_coord(rr.mul32(v)) is None
    inside32 = [rr.round_coord(rr.mul32(v)) is not None for v in rc.EDGE]
    inside = [rr.round_coord(F32(v)) is not None for v in rc.EDGE]
    assert inside32 == [True, False, True, False, False, False, False, False]
    assert inside == [True, True, True, True, True, False, True, False]
    assert rr.round_coord(rr.mul32(-67108864.0)) == -(1 << 31) and rr.split5(-(1 << 31)) == (-(1 << 26), 0)
    # a non-finite entry gives the border value whatever the other coordinate says
    c = rc.case("nonfinite_5x7")
    bad = ~(np.isfinite(c.map_x) & np.isfinite(c.map_y)) | (np.abs(c.map_x) > 1e9) | (np.abs(c.map_y) > 1e9)
    assert bad.sum() == 15
    for kind in ("u8_white", "u16"):
        out = rr.remap_nearest(rc.image(kind, 5, 7), c.map_x, c.map_y)
        assert not out[bad].any() and (out[~bad] == rc.image(kind, 5, 7)[~bad]).all()
    assert not rr.remap_linear_u8(rc.image("u8_white", 5, 7, 3), c.map_x, c.map_y)[bad].any()
    val, bound = rr.remap_linear_f32(rc.image("f32_special", 5, 7), c.map_x, c.map_y)
    assert (val[bad] == 0).all() and (bound[bad] == 0).all()


def test_images_hold_the_planted_values():
    for H, W in rc.SHAPES:
        if H * W >= 4:
            u8 = rc.image("u8", H, W, 3)
            assert u8.min() == 0 and u8.max() == 255
            i32 = rc.image("i32", H, W)
            assert {(1 << 24) + 1, -1, -(1 << 31)} <= set(i32.ravel().tolist())
            u16 = rc.image("u16", H, W)
            assert {32768, 65535} <= set(u16.ravel().tolist())
            sp = rc.image("f32_special", H, W)
            assert np.isnan(sp).any() and np.isposinf(sp).any() and np.isneginf(sp).any() and (np.signbit(sp) & (sp == 0)).any()
        labels = rc.image("i32", H, W, 2).astype(np.int64)
        assert (labels != labels.astype(F32).astype(np.float64)).any()  # some label is no float32 number, at every shape
    r = np.abs(rc.image("f32_random", 17, 31, 4))
    assert r.min() < 1e-25 and r.max() > 1e25 and (rc.image("f32_random", 17, 31, 4) < 0).any()
    assert int(rc.image("i32", 1, 1)[0, 0]) == (1 << 24) + 1


def test_exact_images_make_float32_equal_float64():
    """Every product and partial sum of the float32 evaluation is computed here in float32, one operation at a time, and equals the
    float64 value: no rounding anywhere, so a contracted (FMA) evaluation gives the same bits."""
    for c in rc.maps():
        img = rc.image("f32_exact", c.H, c.W, 2)
        assert rr.is_exact_image(img)
        iy, ix, fy, fx, ok = rr.linear_taps(c.map_x, c.map_y)
        taps = [rr.fetch(img, iy + dy, ix + dx, ok) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
        gx, gy = (fx * F32(1 / 32)).astype(F32)[:, None], (fy * F32(1 / 32)).astype(F32)[:, None]
        one = F32(1)
        w = [(one - gx) * (one - gy), gx * (one - gy), (one - gx) * gy, gx * gy]
        assert all(x.dtype == F32 for x in w)
        acc = taps[0] * w[0]
        for p, x in zip(taps[1:], w[1:]):
            prod = p * x
            assert prod.dtype == F32 and (prod.astype(np.float64) == p.astype(np.float64) * x.astype(np.float64)).all()
            acc = acc + prod
        val, _ = rr.remap_linear_f32(img, c.map_x, c.map_y)
        assert acc.dtype == F32
        np.testing.assert_array_equal(acc.astype(np.float64).reshape(val.shape), val, err_msg=c.name)
    assert not rr.is_exact_image(rc.image("f32_random", 5, 7)) and not rr.is_exact_image(rc.image("f32_special", 5, 7))


def test_the_bound_holds_for_an_unfused_float32_evaluation():
    """The derived bound, tried on the plain float32 evaluation (numpy: no FMA) of the random images."""
    for c in rc.maps():
        img = rc.image("f32_random", c.H, c.W, 3)
        iy, ix, fy, fx, ok = rr.linear_taps(c.map_x, c.map_y)
        taps = [rr.fetch(img, iy + dy, ix + dx, ok) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
        gx, gy = (fx / 32.0).astype(F32)[:, None], (fy / 32.0).astype(F32)[:, None]
        one = F32(1)
        acc = ((taps[0] * ((one - gx) * (one - gy)) + taps[1] * (gx * (one - gy))) + taps[2] * ((one - gx) * gy)) + taps[3] * (gx * gy)
        val, bound = rr.remap_linear_f32(img, c.map_x, c.map_y)
        assert (np.abs(acc.astype(np.float64).reshape(val.shape) - val) <= bound).all(), c.name


def test_batches_differ_frame_by_frame():
    for B in (1, 2, 5):
        for u16 in (False, True):
            d, c = rc.batch(B, 5, 7, u16)
            assert d.shape == (B, 5, 7) and c.shape == (B, 5, 7, 3) and d.dtype == (np.uint16 if u16 else np.float32)
            m = rc.case("permutation_5x7")
            dr, cr = rr.rectify_frames(d, c, m.map_x, m.map_y)
            for f in range(B):
                np.testing.assert_array_equal(dr[f], rr.remap_nearest(d[f], m.map_x, m.map_y))
                np.testing.assert_array_equal(cr[f], rr.remap_linear_u8(c[f], m.map_x, m.map_y))


# ---- the front's refusals, before the library is called --------------------------------------------------------------------------
def fronts():
    return [volume(V.ScalableTSDFVolume, voxel_length=0.02, sdf_trunc=0.08, res=16), volume(V.VoxelBlockGrid, voxel_size=0.02, block_size=8)]


@pytest.mark.parametrize("linear", [False, True])
def test_maps_of_another_shape_are_refused_before_the_library_is_called(linear):
    H, W = 5, 7
    good = rc.case("identity_5x7")
    for vol in fronts():
        for C in (1, 3):
            img = rc.image("u8", H, W, C)
            for shape in ((H - 1, W), (H, W - 1), (W, H), (H + 1, W + 1), (H * W,), (1, H, W), (H, W, 1)):
                bad = np.zeros(shape, F32)
                for mx, my in ((bad, good.map_y), (good.map_x, bad), (bad, bad)):
                    with pytest.raises(RuntimeError, match=r"remap: map_[xy] has shape .* the image is 5x7"):
                        vol.remap(img, mx, my, linear=linear)
                    assert vol._lib.calls == []
            out = vol.remap(img, good.map_x, good.map_y, linear=linear)  # and the next good call goes through
            assert vol._lib.names() == ["hv_remap"] and out.shape == img.shape
            vol._lib.calls = []


def test_float64_and_uint16_images_are_refused():
    good = rc.case("identity_5x7")
    for vol in fronts():
        for img, name in ((rc.image("f32_exact", 5, 7).astype(np.float64), "float64"), (rc.image("u16", 5, 7), "uint16"),
                          (rc.image("u8", 5, 7).astype(np.int64), "int64")):
            with pytest.raises(RuntimeError, match=f"remap: unsupported image dtype {name}"):
                vol.remap(img, good.map_x, good.map_y)
            assert vol._lib.calls == []
