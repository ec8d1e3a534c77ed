"""CPU: the numpy restatement of the TSDF point queries (tests/sample_reference.py) against what the contract in include/hipvol.h
implies, on planted voxel states - and the facts the GPU files (tests/test_gpu_tsdf_sample.py, tests/test_gpu_tsdf_check_frame.py) rest
on: the fragile share of every point set they use is 0.0, and the pulled rectangle of the fused scene is told apart by the
restatement alone.

Bounds of the linear field.  tsdf = (x - X0) / TRUNC is planted as float32 and read back through the import's float32 product and
quotient: at most three roundings of 2^-25 each for |tsdf| < 1.  Trilinear interpolation of a linear field is exact, so the value
inherits at most 3 * 2^-25, the float32 cast of sdf adds one more half ulp: 4 * 2^-25 = 2^-23 of TRUNC, and the bound is twice that,
TRUNC * 2^-22.  A gradient component is a difference of two interpolated values times TRUNC / VOX = 4: 4 * 2 * 3 * 2^-25 plus its own
cast is under 2^-20, the bound twice that, 2^-19.
"""
import re

import numpy as np
import pytest

from tests import planted_states as ps
from tests import sample_cases as sc
from tests import sample_reference as sr

VOX, TRUNC = sc.VOX, sc.TRUNC


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_constants_match_the_header_and_the_binding():
    from pyslam_amd import _lib as L
    from pyslam_amd import volumetric as V

    text = open(L._build.INCLUDE + "/hipvol.h").read()
    header = {name: int(value) for name, value in re.findall(r"#define (HV_(?:SAMPLE|CHECK)_[A-Z_]+) (\d+)", text)}
    assert len(header) == 9
    for name, value in header.items():
        short = name.split("_", 2)[2]
        assert getattr(sr, short) == value and getattr(L, name) == value and getattr(V, name[3:]) == value, name
    assert re.search(r"HV_F32 = 0, HV_F64 = 1", text) and (L.HV_F32, L.HV_F64) == (0, 1)
    assert sr.FRAGILE_BAND == 1e-9


def test_linear_field_is_reproduced_within_the_float32_roundings():
    dump = ps.as_dump(sc.linear_states())
    assert (dump[2] > 0).all() and dump[2].max() <= 7 and len(dump[0]) == 8
    p = sc.linear_points()
    out = sr.sample_points(dump, VOX, TRUNC, p)
    assert (out["status"] == sr.TRILINEAR).all()
    # the points reach across unit borders along every axis
    cell = np.floor(p / VOX - 0.5).astype(np.int64)
    assert all(((cell[:, a] & 15) == 15).any() for a in range(3))
    assert np.abs(out["sdf"].astype(np.float64) - (p[:, 0] - sc.X0)).max() <= sc.LINEAR_SDF_BOUND
    assert np.abs(out["gradient"].astype(np.float64) - [1.0, 0.0, 0.0]).max() <= sc.LINEAR_GRADIENT_BOUND
    np.testing.assert_array_equal(out["weight"], dump[2][sr.rr._Grid(dump).locate(*np.floor(p / VOX).astype(np.int64).T)])


def test_voxel_centres_return_the_voxel():
    """r = 0 on every axis: the interpolation collapses onto corner 0, whatever the other seven hold."""
    states = ps.random_units(np.array([(i, j, k) for i in (-1, 0) for j in (-1, 0) for k in (-1, 0)], np.int64), 31, unobserved=0.0)
    dump = ps.as_dump(states)
    rng = np.random.default_rng(32)
    gi = rng.integers(-15, 15, (4000, 3))  # voxels whose +1 neighbours lie in the block too
    p = (gi + 0.5) * VOX
    exact = (p / np.float64(VOX) - 0.5 == gi).all(axis=1)  # the lattice coordinate the contract computes is the integer itself
    assert exact.sum() > 1000
    p, gi = p[exact], gi[exact]
    out = sr.sample_points(dump, VOX, TRUNC, p)
    assert (out["status"] == sr.TRILINEAR).all() and out["fragile"].all()
    row, word = sr.rr._Grid(dump).locate(*gi.T)
    assert np.array_equal(bits(out["sdf"]), bits((np.float64(TRUNC) * dump[1][row, word].astype(np.float64)).astype(np.float32)))
    assert np.array_equal(bits(out["color"]), bits((dump[3][row, word] / 255.0).astype(np.float32)))
    assert np.array_equal(out["weight"], dump[2][row, word])


def test_status_rules_on_hand_made_cases():
    dump = ps.as_dump(sc.hand_states())
    points, expected = sc.hand_points()
    out = sr.sample_points(dump, VOX, TRUNC, points)
    for (name, _, want), got in zip(sc.HAND_POINTS, out["status"]):
        assert got == want, name
    assert not out["fragile"].any()
    # the alias of a key beyond the rim is held: only the range check keeps those points OUTSIDE
    assert (np.asarray(dump[0]) == ps.RIM_ALIAS).all(axis=1).any()
    zero = out["status"] <= sr.UNOBSERVED
    for name in ("sdf", "gradient", "color", "weight"):
        assert not out[name][zero].any(), name
    names = [n for n, _, _ in sc.HAND_POINTS]
    one = names.index("the one observed voxel of a unit")
    assert out["sdf"][one] == np.float32(np.float64(TRUNC) * np.float64(np.float32(0.25))) and out["weight"][one] == 5
    assert np.array_equal(out["color"][one], (np.array([10.0, 200.0, 77.0]) / 255.0).astype(np.float32)) and not out["gradient"][one].any()
    seven = names.index("seven of eight observed")
    assert not out["gradient"][seven].any() and out["weight"][seven] > 0
    # float32 points are widened first
    p32 = points.astype(np.float32)
    a, b = sr.sample_points(dump, VOX, TRUNC, p32), sr.sample_points(dump, VOX, TRUNC, p32.astype(np.float64))
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)
    # the empty map: every point OUTSIDE
    empty = sr.sample_points(sr_empty(), VOX, TRUNC, points)
    assert not empty["status"].any() and not empty["sdf"].any()


def sr_empty():
    from tests.merge_reference import empty_dump

    return empty_dump()


@pytest.mark.parametrize("threshold", sc.THRESHOLDS)
def test_thresholds_move_the_statuses(threshold):
    dump = ps.as_dump(sc.cluster_states())
    p = sc.cluster_points(4097)
    out = sr.sample_points(dump, VOX, TRUNC, p, threshold)
    assert set(np.unique(out["status"])) == {sr.OUTSIDE, sr.UNOBSERVED, sr.NEAREST, sr.TRILINEAR}
    # the nearest voxel's weight decides OUTSIDE / UNOBSERVED / observed
    row, word = sr.rr._Grid(dump).locate(*np.floor(p / VOX).astype(np.int64).T)
    w = np.where(row >= 0, dump[2][np.maximum(row, 0), word], -1.0)
    assert np.array_equal(out["status"] == sr.OUTSIDE, w < 0)
    assert np.array_equal(out["status"] >= sr.NEAREST, w > threshold)
    assert np.array_equal(out["weight"], np.where(w > threshold, w, 0.0).astype(np.float32))
    if threshold > 0:
        low = sr.sample_points(dump, VOX, TRUNC, p, 0.0)
        assert (out["status"] <= low["status"]).all() and (out["status"] < low["status"]).any()


def test_fragile_share_of_every_point_set_the_gpu_tests_use_is_zero():
    dump = ps.as_dump(sc.cluster_states())
    for n in sc.POINT_COUNTS:
        p = sc.cluster_points(n)
        for q in (p, p.astype(np.float32)):
            assert not sr.sample_points(dump, VOX, TRUNC, q)["fragile"].any(), n
    assert not sr.sample_points(ps.as_dump(sc.hand_states()), VOX, TRUNC, sc.hand_points()[0])["fragile"].any()
    assert not sr.sample_points(ps.as_dump(sc.linear_states()), VOX, TRUNC, sc.linear_points())["fragile"].any()
    seen = np.zeros(5, np.int64)
    for pose in sc.POSES:
        states, T = sc.wall_scene(pose)
        dump = ps.as_dump(states)
        for H, W in sc.IMAGE_SIZES:
            for kind, scale in sc.DEPTH_KINDS:
                out = sr.check_frame(dump, VOX, TRUNC, sc.wall_depth(H, W, kind, scale), sc.intrinsics(H, W), T, scale)
                assert not out["fragile"].any(), (pose, H, W, kind)
                assert out["count"].sum() == H * W and np.array_equal(out["count"], np.bincount(out["cls"].reshape(-1), minlength=5))
                assert not out["sdf"][out["cls"] <= sr.UNKNOWN].any()
                seen += out["count"]
    assert (seen > 100).all(), seen  # every class occurs


def test_class_rule_at_the_tolerance():
    tol = 0.0390625  # 5 * 2^-7: a float32
    up, down = np.nextafter(np.float32(tol), np.float32(1)), np.nextafter(np.float32(tol), np.float32(0))
    sdf = np.array([tol, -tol, up, -up, down, -down, 0.0, 1.0, -1.0, 5.0], np.float32)
    status = np.array([3, 2, 3, 3, 2, 2, 3, 0, 1, 3], np.uint8)
    valid = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 0], bool)
    want = [sr.CONSISTENT, sr.CONSISTENT, sr.IN_FRONT, sr.BEHIND, sr.CONSISTENT, sr.CONSISTENT, sr.CONSISTENT, sr.UNKNOWN, sr.UNKNOWN, sr.INVALID]
    assert sr.classify(sdf, status, valid, tol).tolist() == want
    # the float32 sdf is widened and compared in double: a tolerance between two float32 values splits them
    assert sr.classify(np.array([up, down], np.float32), np.array([3, 3]), np.array([True, True]), float(tol) + 1e-12).tolist() == [sr.IN_FRONT, sr.CONSISTENT]


def test_depth_edge_values():
    states, T = sc.wall_scene("+z")
    depth = np.array([[0.0, np.nan, np.inf, 0.25, 0.5, -np.inf, np.nextafter(np.float32(0.25), np.float32(1)), np.nextafter(np.float32(0.5), np.float32(1))]],
                     np.float32)
    out = sr.check_frame(ps.as_dump(states), VOX, TRUNC, depth, (40.0, 40.0, 3.5, 0.0), T, 1.0, 0.25, 0.5)
    assert (out["cls"][0] == sr.INVALID).tolist() == [True, True, True, True, False, True, False, True]
    assert out["cls"][0, 4] == sr.CONSISTENT  # depth_max exactly is valid: the pixel lies on the front wall


def test_fused_scene_pulled_rectangle_is_told_apart_by_the_restatement():
    """The restatement on the oracle-fused map: of the pulled pixels with valid depth none is CONSISTENT and at least half are
    IN_FRONT; the frame as it was fused is CONSISTENT almost everywhere."""
    from tests.test_gpu_tsdf_edges import frames_of, intrinsic, oracle_of

    s, frames = frames_of("tiny_160x120_2cm", 0, sc.FUSED_FRAMES)
    dump = oracle_of(s, frames, VOX, TRUNC).dump()
    depth, _, T = frames[sc.FUSED_FRAME]
    K = intrinsic(s).as_array()
    before = sr.check_frame(dump, VOX, TRUNC, depth, K, T, 1.0, 0.1, 4.0)
    assert before["count"][sr.CONSISTENT] > 0.95 * (before["count"].sum() - before["count"][sr.INVALID])
    out = sr.check_frame(dump, VOX, TRUNC, sc.pulled(depth), K, T, 1.0, 0.1, 4.0)
    assert not out["fragile"].any() and not before["fragile"].any()
    rect = out["cls"][sc.PULL_RECT]
    valid = int((rect != sr.INVALID).sum())
    assert valid > 1000 and (rect == sr.CONSISTENT).sum() == 0 and (rect == sr.IN_FRONT).sum() >= valid / 2
    outside = np.ones(out["cls"].shape, bool)
    outside[sc.PULL_RECT] = False
    assert np.array_equal(out["cls"][outside], before["cls"][outside])
    cleaned = sc.pulled(depth)
    cleaned[out["cls"] == sr.IN_FRONT] = 0
    assert sr.check_frame(dump, VOX, TRUNC, cleaned, K, T, 1.0, 0.1, 4.0)["count"][sr.IN_FRONT] == 0
