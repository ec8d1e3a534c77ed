"""CPU: the numpy restatement of the point lookup (tests/lookup_reference.py) - (a) the planted cases of tests/lookup_cases.py tell
every wrong reading of the contract (lookup_reference.VARIANTS) from the right one, on states planted in the oracle's C restatement
grids; (b) the restatement is tied to the COMPILED REFERENCE: every voxel its get_voxels(min_count, min_confidence) lists is looked
up at its own listed position with radius 0 and must come back as exactly that row."""
import numpy as np
import pytest

import oracle
from oracle.semantic import PortSemGrid2, RefSemGrid2
from tests import lookup_cases as lc
from tests import lookup_reference as lr
from tests.semantic_helpers import frame_points, semantic_frame

need_ref = pytest.mark.skipif(not oracle.ref_available(), reason="compiled reference not available")
INTR32 = np.array(lc.INTR, np.float32)


def _carve(grid, depth, threshold):
    grid.carve(INTR32, lc.W, lc.H, np.eye(4), lc.DEPTH_MAX, lc.DEPTH_MIN, depth, threshold)


def planted_states(bs):
    """[(case, state)] on the C restatement grids: the plain grid and the voting payload (kind 0)."""
    out = []
    for case in lc.cases(bs):
        plain = oracle.PortGrid(lc.VOXEL, bs)
        lc.run_case(plain, case, False, _carve)
        out.append((case, lr.plain_state(plain.dump())))
        sem = PortSemGrid2(0, lc.VOXEL, bs)
        lc.run_case(sem, case, True, _carve)
        out.append((case, lr.semantic_state(sem.dump())))
    return out


def param_sets(case, state):
    sets = list(case.params)
    if case.conf_voxel is not None and not state["plain"]:
        b, l = lr._index(state, case.bs)[case.conf_voxel]
        conf = np.float32(state["conf"][b, l])
        sets += [(1, float(conf)), (1, float(np.nextafter(conf, np.float32(2.0))))]
    return sets


STATES = {bs: None for bs in lc.BLOCK_SIZES}


def states(bs):
    if STATES[bs] is None:
        STATES[bs] = planted_states(bs)
    return STATES[bs]


@pytest.mark.parametrize("bs", lc.BLOCK_SIZES)
def test_planted_states_hold_what_the_cases_say(bs):
    by_name = {(c.name, s["plain"]): (c, s) for c, s in states(bs)}
    # the carved voxel sits, reset, inside a live block, next to voxels that kept their points
    case, s = by_name[("reset", False)]
    idx = lr._index(s, bs)
    assert (0, 0, 8) not in idx and (1, 0, 8) in idx and (0, 0, 9) in idx and (4, 4, 8) in idx
    assert (np.asarray(s["keys"]) == np.array([0, 0, 8 // bs])).all(1).any()
    # the confidence case's voxel is under 1, its neighbour at 1
    case, s = by_name[("conf_edge", False)]
    idx = lr._index(s, bs)
    assert 0.0 < s["conf"][idx[(2, 2, 2)]] < 1.0 and s["conf"][idx[(3, 2, 2)]] == 1.0
    # the corner voxel's neighbourhood: three of its eight blocks exist
    case, s = by_name[("corner8", True)]
    assert len(s["keys"]) == 3 and case.n_blocks() == 3
    assert by_name[("empty", True)][1]["keys"].shape[0] == 0


@pytest.mark.parametrize("variant", lr.VARIANTS)
def test_every_variant_differs_on_a_planted_case(variant):
    """The cases tell the rules apart: each wrong reading changes at least one answer."""
    differs = []
    for bs in lc.BLOCK_SIZES:
        for case, state in states(bs):
            for dtype in (np.float32, np.float64):
                pts = case.points(dtype)
                for mc, conf in param_sets(case, state):
                    for radius in (0, 1, 2):
                        right = lr.lookup(state, pts, lc.VOXEL, bs, mc, conf, radius)
                        wrong = lr.lookup(state, pts, lc.VOXEL, bs, mc, conf, radius, variant=variant)
                        if lr.same(right, wrong) is not None:
                            differs.append((case.name, bs, np.dtype(dtype).name, radius))
    assert differs, variant


def test_float64_points_that_float32_keys_elsewhere():
    """f32_key_for_f64 needs a float64 point whose float32 rounding crosses a voxel face: one float64 ulp under the face."""
    bs = 8
    g = PortSemGrid2(0, lc.VOXEL, bs)
    below = np.nextafter(0.5, 0.0)
    g.integrate(np.array([[below, 1 / 16, 1 / 16]], np.float64), np.zeros((1, 3), np.float32), np.array([1], np.int32), np.array([1], np.int32), None)
    state = lr.semantic_state(g.dump())
    assert (1, 0, 0) in lr._index(state, bs)  # the float64 integrate keyed it in float64
    pts = np.array([[below, 1 / 16, 1 / 16]], np.float64)
    assert lr.lookup(state, pts, lc.VOXEL, bs)["status"][0] == lr.OWN
    assert lr.lookup(state, pts, lc.VOXEL, bs, variant="f32_key_for_f64")["status"][0] == lr.MISSING
    assert lr.lookup(state, pts.astype(np.float32), lc.VOXEL, bs)["status"][0] == lr.MISSING  # float32(below) == 0.5: voxel 2


def test_results_of_the_cases_are_as_planted():
    """Spot checks of the right rule against the cases' own words (so that the restatement is not only compared with itself)."""
    bs = 8
    by = {(c.name, s["plain"]): (c, s) for c, s in states(bs)}
    case, s = by[("tie", False)]
    r = lr.lookup(s, case.points(np.float64), lc.VOXEL, bs, radius=1)
    assert r["status"][0] == lr.NEAR and r["class_id"][0] == 1 and r["position"][0, 0] == 0.375
    case, s = by[("own_wins", False)]
    r = lr.lookup(s, case.points(np.float32), lc.VOXEL, bs, radius=2)
    assert r["status"][0] == lr.OWN and r["class_id"][0] == 1
    case, s = by[("under_min_count", True)]
    r = lr.lookup(s, case.points(np.float64), lc.VOXEL, bs, min_count=2, radius=1)
    assert r["status"].tolist() == [lr.NEAR, lr.OWN] and r["count"].tolist() == [2, 2]
    case, s = by[("negative", False)]
    r = lr.lookup(s, case.points(np.float64), lc.VOXEL, bs)
    assert r["class_id"][:4].tolist() == [1, 3, 2, 2] and r["status"][-5:].tolist() == [lr.INVALID] * 5
    case, s = by[("key_edge", False)]
    r = lr.lookup(s, case.points(np.float32), lc.VOXEL, bs, radius=1)
    assert r["status"].tolist() == [lr.OWN, lr.NEAR, lr.MISSING, lr.INVALID, lr.OWN, lr.NEAR, lr.MISSING, lr.INVALID]
    r = lr.lookup(s, case.points(np.float64), lc.VOXEL, bs, radius=2)
    assert r["status"].tolist() == [lr.OWN, lr.NEAR, lr.NEAR, lr.INVALID, lr.OWN, lr.NEAR, lr.NEAR, lr.INVALID]
    case, s = by[("reset", True)]
    r = lr.lookup(s, case.points(np.float64), lc.VOXEL, bs, radius=1)
    assert r["status"].tolist() == [lr.NEAR, lr.OWN, lr.OWN, lr.NEAR]
    with pytest.raises(ValueError):
        lr.lookup(s, case.points(np.float64), lc.VOXEL, bs, radius=3)


@need_ref
@pytest.mark.parametrize("kind", (0, 1, 2, 3))
def test_restatement_returns_the_rows_the_compiled_reference_lists(kind):
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD("tiny_160x120_2cm")
    ref = RefSemGrid2(kind, 0.02, 8)
    for i in range(2):
        depth, rgb, T, cls_img, inst_img = semantic_frame(s, i)
        pts, cols, cls, obj, depths = frame_points(depth, rgb, T, cls_img, inst_img, s.intrinsics, 4.0)
        ref.integrate(pts, cols, cls, obj, depths)  # float64 points: keyed in float64, as the float64 lookup keys a listed position
    state = lr.semantic_state(ref.dump())
    for min_count, min_confidence in ((1, 0.0), (2, 0.6), (3, -1.0)):
        rows = ref.get_voxels(min_count, min_confidence)
        assert len(rows[0]) > 100
        got = lr.lookup(state, np.ascontiguousarray(rows[0]), 0.02, 8, min_count, min_confidence, 0)
        assert lr.status_counts(got["status"])[1] == len(rows[0])  # every listed voxel is found as its OWN voxel
        for name, want in zip(("position", "color", "class_id", "object_id", "confidence"), rows):
            assert got[name].dtype == want.dtype and got[name].tobytes() == np.ascontiguousarray(want).tobytes(), name
        # ... and a voxel that is not listed is not found: the restatement finds exactly len(rows) voxels among ALL occupied ones
        every = ref.get_voxels(1, -1.0)
        found = lr.lookup(state, np.ascontiguousarray(every[0]), 0.02, 8, min_count, min_confidence, 0)
        assert lr.status_counts(found["status"])[1] == len(rows[0])


@need_ref
def test_restatement_returns_the_rows_of_the_compiled_plain_grid():
    from oracle import host_prep
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD("tiny_160x120_2cm")
    ref = oracle.RefGrid(0.02, 8)
    depth, rgb, T = s[0]
    pts, cols, _ = host_prep.frame_to_world_f32(depth, rgb, *s.intrinsics, T, 4.0)
    ref.integrate(pts, cols)
    state = lr.plain_state(ref.dump())
    for min_count in (1, 2):
        pos, col = ref.get_voxels(min_count, 0.0)
        assert len(pos) > 100
        got = lr.lookup(state, np.ascontiguousarray(pos), 0.02, 8, min_count, 0.0, 0)  # float32 rows of a float32-keyed grid
        assert lr.status_counts(got["status"])[1] == len(pos)
        assert got["position"].tobytes() == pos.astype(np.float64).tobytes() and got["color"].tobytes() == np.ascontiguousarray(col).tobytes()
