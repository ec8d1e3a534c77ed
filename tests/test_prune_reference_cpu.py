"""CPU: the numpy restatement of TSDF pruning (tests/prune_reference.py) on hand-built dumps, the metres-to-units conversion of
ScalableTSDFVolume.prune (pyslam_amd.volumetric.unit_range_of_bounds), and the inputs the GPU tests rely on: how many units of the
tests' own stream carry no observed voxel, with and without a de-integration (a test that releases nothing shows nothing)."""
import numpy as np
import pytest

from tests.prune_reference import prune_reference

R3 = 16 ** 3
VOX, TRUNC = 0.02, 0.08


def hand_dump(units):
    """units = [(key, weight of voxel 7)] -> a key-sorted dump; a unit of weight 0 is fresh in every plane."""
    units = sorted(units)
    n = len(units)
    keys = np.array([k for k, _ in units], np.int32).reshape(n, 3)
    t = np.zeros((n, R3), np.float32)
    w = np.zeros((n, R3), np.float32)
    c = np.zeros((n, R3, 3), np.float64)
    for i, (_, weight) in enumerate(units):
        if weight:
            t[i, 7], w[i, 7], c[i, 7] = 0.25 * (i + 1), weight, (10.0 * i, 20.0, 30.0)
    return keys, t, w, c


def assert_rows(after, before, rows):
    for a, b in zip(after, before):
        np.testing.assert_array_equal(a, b[rows])


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_outside_takes_precedence_over_empty():
    dump = hand_dump([((0, 0, 0), 3), ((1, 0, 0), 0), ((5, 0, 0), 0), ((6, 0, 0), 2)])
    after, stats = prune_reference(dump, True, (0, 0, 0), (4, 4, 4))
    assert stats == (4, 2, 1, 1)  # (5,0,0) is empty AND outside: counted as outside
    assert_rows(after, dump, [0])
    after, stats = prune_reference(dump, False, (0, 0, 0), (4, 4, 4))
    assert stats == (4, 2, 0, 2)
    assert_rows(after, dump, [0, 1])


def test_no_criterion_is_a_no_op():
    dump = hand_dump([((0, 0, 0), 0), ((0, 0, 1), 1)])
    after, stats = prune_reference(dump, False, None, None)
    assert stats == (2, 0, 0, 2)
    assert_rows(after, dump, [0, 1])


def test_everything_and_nothing_released():
    dump = hand_dump([((-3, 2, 1), 0), ((0, 0, 0), 0)])
    after, stats = prune_reference(dump, True)
    assert stats == (2, 0, 2, 0) and all(len(x) == 0 for x in after)
    assert after[1].shape == (0, R3) and after[3].shape == (0, R3, 3)
    after, stats = prune_reference(dump, True, (10, 10, 10), (11, 11, 11))
    assert stats == (2, 2, 0, 0)
    full = hand_dump([((-3, 2, 1), 1), ((0, 0, 0), 9)])
    after, stats = prune_reference(full, True, (-3, 0, 0), (0, 2, 1))
    assert stats == (2, 0, 0, 2)
    assert_rows(after, full, [0, 1])
    empty = hand_dump([])
    after, stats = prune_reference(empty, True, (0, 0, 0), (1, 1, 1))
    assert stats == (0, 0, 0, 0)


def test_the_range_is_inclusive_per_axis():
    dump = hand_dump([((x, y, 0), 1) for x in range(-2, 3) for y in range(-2, 3)])
    after, stats = prune_reference(dump, True, (-1, 0, 0), (1, 2, 0))
    assert stats == (25, 25 - 9, 0, 9)
    assert sorted(map(tuple, after[0])) == [(x, y, 0) for x in (-1, 0, 1) for y in (0, 1, 2)]


# ---- metres -> units --------------------------------------------------------------------------------------------------------
def test_unit_range_floors_negative_coordinates():
    from pyslam_amd.volumetric import unit_range_of_bounds

    lo, hi = unit_range_of_bounds(((-0.1, -1.0, 0.1), (0.1, -0.9, 1.1)), 0.0625, 16)  # L = 1.0 exactly
    assert lo.dtype == np.int32 and hi.dtype == np.int32
    assert lo.tolist() == [-1, -1, 0] and hi.tolist() == [0, -1, 1]


def test_a_bound_on_a_unit_face_keeps_the_unit_beyond_it():
    from pyslam_amd.volumetric import unit_range_of_bounds

    # unit k is the half-open box [k L, (k + 1) L): max = 3 L meets unit 3; min = 3 L does not meet unit 2
    lo, hi = unit_range_of_bounds(((0.0, 0.0, 3.0), (3.0, 2.999, 3.0)), 0.0625, 16)
    assert lo.tolist() == [0, 0, 3] and hi.tolist() == [3, 2, 3]
    lo, hi = unit_range_of_bounds(((-2.0, -2.0, -2.0), (-2.0, -2.0, -2.0)), 0.0625, 16)
    assert lo.tolist() == [-2, -2, -2] and hi.tolist() == [-2, -2, -2]


def test_unit_length_that_is_not_representable():
    from pyslam_amd.volumetric import unit_range_of_bounds

    L = np.float64(0.02) * np.float64(16)  # 0.32 is not a binary fraction: the conversion is the float64 quotient, floored
    pts = np.array([-1.0, -0.64, -0.32, -1e-9, 0.0, 0.31999, 0.32, 0.96, 7 * L, 7 * 0.32])
    for x in pts:
        lo, hi = unit_range_of_bounds(((x, x, x), (x, x, x)), 0.02, 16)
        want = int(np.floor(np.float64(x) / L))
        assert lo.tolist() == [want] * 3 and hi.tolist() == [want] * 3, x
    lo, hi = unit_range_of_bounds(((-0.33, 0.0, 0.0), (0.33, 0.31, 0.65)), 0.02, 16)
    assert lo.tolist() == [-2, 0, 0] and hi.tolist() == [1, 0, 2]
    # the default resolution is the volume's 16
    assert [x.tolist() for x in unit_range_of_bounds(((0, 0, 0), (1, 1, 1)), 0.02)] == [[0, 0, 0], [3, 3, 3]]


def test_bad_bounds_raise():
    from pyslam_amd.volumetric import unit_range_of_bounds

    with pytest.raises(ValueError):
        unit_range_of_bounds(((0.0, 0.0, 1.0), (1.0, 1.0, 0.5)), 0.02, 16)  # min > max
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            unit_range_of_bounds(((0.0, 0.0, 0.0), (1.0, bad, 1.0)), 0.02, 16)
        with pytest.raises(ValueError):
            unit_range_of_bounds(((bad, 0.0, 0.0), (1.0, 1.0, 1.0)), 0.02, 16)
    L = 0.32
    with pytest.raises(ValueError):
        unit_range_of_bounds(((0.0, 0.0, 0.0), (0.0, 0.0, (1 << 20) * L)), 0.02, 16)  # unit 2^20 is not a key
    with pytest.raises(ValueError):
        unit_range_of_bounds(((-((1 << 20) + 1) * L, 0.0, 0.0), (0.0, 0.0, 0.0)), 0.02, 16)
    lo, hi = unit_range_of_bounds(((-(1 << 20) * 1.0, 0.0, 0.0), (0.0, 0.0, (1 << 20) * 1.0 - 0.5)), 0.0625, 16)  # the last keys fit
    assert lo[0] == -(1 << 20) and hi[2] == (1 << 20) - 1
    with pytest.raises(ValueError):
        unit_range_of_bounds(((0.0, 0.0), (1.0, 1.0)), 0.02, 16)
    with pytest.raises(ValueError):
        unit_range_of_bounds((0.0, 0.0, 0.0), 0.02, 16)


# ---- the stream the GPU tests fuse -------------------------------------------------------------------------------------------
def test_the_tiny_stream_holds_units_without_an_observed_voxel():
    """oracle.PortTsdf on tiny_160x120_2cm frames 0..47 (2 cm / 8 cm, stride 4): 451 units, 19 of them never updated; after frames
    24..47 are taken out again (tests/deintegrate_reference.py), 85.  The removal's result is the oracle of frames 0..23 wherever
    that holds a unit."""
    from tests.deintegrate_reference import deintegrate_reference, frame_samples
    from tests.test_gpu_tsdf_edges import intrinsic, oracle_of, tiny_frames

    s, frames = tiny_frames(0, 48)
    full = oracle_of(s, frames, VOX, TRUNC).dump()
    after, stats = prune_reference(full, True)
    assert stats == (451, 0, 19, 432)
    assert np.all(after[2].max(axis=1) > 0)
    assert prune_reference(after, True)[1] == (432, 0, 0, 432)

    K = intrinsic(s).as_array()
    samples = [frame_samples(VOX, TRUNC, d, c, K, T) for d, c, T in frames[24:]]
    removed, dstats = deintegrate_reference(full, samples)
    assert dstats[1] == 0 and dstats[3] == 0
    pruned, stats = prune_reference(removed, True)
    assert stats == (451, 0, 85, 366)
    first = prune_reference(oracle_of(s, frames[:24], VOX, TRUNC).dump(), True)[0]
    np.testing.assert_array_equal(pruned[0], first[0])
    np.testing.assert_array_equal(pruned[2], first[2])
