"""CPU: the numpy restatement of the bundle-adjustment contract (tests/bundle_reference.py) checked against itself - its Jacobians
against central differences of its own residual, its Schur-complement solve against a dense solve of the full damped system - and on
the planted problems of tests/bundle_cases.py, whose fairness conditions for the GPU comparison are asserted here; and build_tracks
on planted match lists."""
import numpy as np
import pytest

from pyslam_amd import bundle as B
from tests import bundle_cases as C
from tests import bundle_reference as R

CASES = {c["name"]: c for c in C.all_cases()}
SMALL = sorted(n for n, c in CASES.items() if 6 * len(c["cameras"]) + 3 * len(c["points"]) <= 400)


def measurements(c):
    return np.c_[c["meas"], c["inv_sigma2"]]


@pytest.fixture(scope="module")
def runs():
    return {n: R.optimize(c["cameras"], c["points"], c["idx"], measurements(c), c["active"], c["fixed"], **c["params"]) for n, c in CASES.items()}


def test_the_cases_are_the_shapes_they_claim():
    assert max(len(c["cameras"]) for c in CASES.values()) <= 257 and max(len(c["points"]) for c in CASES.values()) <= 4096
    assert max(len(c["idx"]) for c in CASES.values()) <= 20000
    g = CASES["gather_edges"]
    per_camera = np.bincount(g["idx"][:, 0], minlength=len(g["cameras"]))
    per_point = np.bincount(g["idx"][:, 1], minlength=len(g["points"]))
    assert {1, 63, 64, 65, 129, 1025} <= set(per_camera.tolist())
    assert {0, 1, 2, 17, 65} <= set(per_point.tolist())
    m = CASES["mixed"]
    stereo = np.isfinite(m["meas"][:, 2])
    assert stereo.any() and (~stereo).any() and not stereo[m["idx"][:, 1] == 0].any()
    assert not np.isfinite(CASES["mono_two_fixed"]["meas"][:, 2]).any() and CASES["mono_two_fixed"]["fixed"].sum() == 2
    d = CASES["duplicates"]["idx"]
    assert len(np.unique(d, axis=0)) < len(d)
    i = CASES["inactive"]
    assert not i["active"][i["idx"][:, 0] == 3].any() and not i["active"][i["idx"][:, 1] == 11].any() and i["active"].sum() > 20
    assert CASES["one_free_camera"]["fixed"].sum() == 4 and CASES["pose_only"]["params"]["fixed_points"]
    assert CASES["points_only"]["fixed"].all()
    o = CASES["outliers"]
    assert o["outliers"].sum() == len(o["idx"]) // 10 and np.abs(o["meas"] - C.project(o["truth_cameras"], o["truth_points"], o["idx"], True)[0])[
        o["outliers"]].min() >= 20.0


@pytest.mark.parametrize("name", ["two_cameras", "mixed", "outliers", "behind_at_start"])
def test_jacobians_against_central_differences(name):
    c = CASES[name]
    P, idx, meas = c["params"], c["idx"], measurements(c)
    lin = R.linearise(c["cameras"], c["points"], idx, meas, c["active"], P)
    on, h = lin["on"], 1e-6

    def r_at(cams, pts):
        return R.linearise(cams, pts, idx, meas, on, P)["r"]

    for a in range(6):
        d = np.zeros((len(c["cameras"]), 6))
        d[:, a] = h
        num = (r_at(R.exp(d) @ c["cameras"], c["points"]) - r_at(R.exp(-d) @ c["cameras"], c["points"])) / (2 * h)
        assert np.abs(num - lin["Jc"][:, :, a]).max() <= 1e-6 * max(1.0, np.abs(lin["Jc"]).max())
    for a in range(3):
        d = np.zeros_like(c["points"])
        d[:, a] = h
        num = (r_at(c["cameras"], c["points"] + d) - r_at(c["cameras"], c["points"] - d)) / (2 * h)
        assert np.abs(num - lin["Jp"][:, :, a]).max() <= 1e-6 * max(1.0, np.abs(lin["Jp"]).max())
    # the weight is the derivative of the kernel
    chi2 = lin["chi2"][on]
    for k, e in ((5.991, ~np.isfinite(c["meas"][:, 2])[on]), (7.815, np.isfinite(c["meas"][:, 2])[on])):
        rho = lambda x: np.where(x <= k, x, 2 * np.sqrt(k * x) - k)
        num = (rho(chi2[e] + h) - rho(chi2[e] - h)) / (2 * h)
        np.testing.assert_allclose(lin["w"][on][e], num, rtol=1e-6)
        np.testing.assert_allclose(lin["rho"][on][e], rho(chi2[e]), rtol=1e-14)


@pytest.mark.parametrize("name", SMALL)
def test_schur_solve_against_the_dense_system(name):
    c = CASES[name]
    P = c["params"]
    pf = not P.get("fixed_points", False)
    lin = R.linearise(c["cameras"], c["points"], c["idx"], measurements(c), c["active"], P)
    blk = R.blocks(lin, c["idx"], len(c["cameras"]), len(c["points"]))
    blk["bc"][c["fixed"]] = 0
    if not pf:
        blk["bp"][:] = 0
    for lam in (1e-3, 1.0, 1e3):
        dc, dp, its, res = R.solve_schur(blk, c["idx"], lam, c["fixed"], pf, 1e-13, 500)
        wc, wp, _, _ = R.solve_dense(blk, c["idx"], lam, c["fixed"], pf)
        scale = max(np.abs(wc).max(), np.abs(wp).max(), 1e-300)
        assert np.abs(dc - wc).max() <= 1e-8 * scale and np.abs(dp - wp).max() <= 1e-8 * scale, (name, lam, its, res)
        if not pf:
            assert its <= 1 and not dp.any()


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["exact"]))
def test_exact_data_recover_the_truth(runs, name):
    c, out = CASES[name], runs[name]
    assert out["success"] and out["chi2_final"] <= 1e-12 * max(1.0, out["chi2_initial"])
    seen = np.zeros(len(c["points"]), bool)
    seen[c["idx"][c["active"] & ~out["behind"], 1]] = True
    assert C.pose_error(out["cameras"], c["truth_cameras"]) <= 1e-7
    assert np.abs(out["points"] - c["truth_points"])[seen].max() <= 1e-6
    # the dense solver walks the same path
    dense = R.optimize(c["cameras"], c["points"], c["idx"], measurements(c), c["active"], c["fixed"], solver=R.solve_dense, **c["params"])
    assert dense["success"] and C.pose_error(dense["cameras"], c["truth_cameras"]) <= 1e-7


def test_the_outlier_case_marks_the_planted_observations(runs):
    c, out = CASES["outliers"], runs["outliers"]
    assert out["success"] and np.array_equal(~out["inlier"], c["outliers"])
    # the kernel bounds what an outlier pulls but does not remove it; the second phase of the schedule (bundle.bundle_adjust_two_phase)
    # switches the marked observations off, and the rest are exact data
    second = R.optimize(out["cameras"], out["points"], c["idx"], measurements(c), out["inlier"], c["fixed"], **{**c["params"], "huber": False})
    assert second["success"] and C.pose_error(second["cameras"], c["truth_cameras"]) <= 1e-7


def test_the_depth_rules(runs):
    a = runs["behind_at_start"]
    assert a["behind"].sum() == 1 and a["behind"][-1] and not a["inlier"][-1] and a["chi2"][-1] == 0.0
    t = runs["behind_in_trial"]
    nan_rows = [k for k, r in enumerate(t["trace"]) if r["F_trial"] != r["F_trial"]]
    assert nan_rows and all(not t["trace"][k]["accepted"] and t["trace"][k]["rho"] == 0.0 for k in nan_rows)
    assert not t["behind"].any() and t["success"]
    F = [r["F"] for r in t["trace"]]
    assert all(b <= a_ for a_, b in zip(F, F[1:]))  # never discontinuous: rejected steps leave F where it was


def test_isolated_variables_do_not_move(runs):
    c, out = CASES["inactive"], runs["inactive"]
    assert np.array_equal(out["cameras"][3], c["cameras"][3]) and np.array_equal(out["points"][11], c["points"][11])
    g, out = CASES["gather_edges"], runs["gather_edges"]
    assert np.array_equal(out["points"][1025:], g["points"][1025:]) and np.array_equal(out["cameras"][0], g["cameras"][0])


@pytest.mark.parametrize("name", sorted(CASES))
def test_flag_comparisons_are_fair(runs, name):
    """Every sqrt(chi2) stays 1e-3 from its delta and every gain ratio 1e-3 from 0 on the restatement's own run (a ratio that is 0 by
    rule - a trial that is not a number - is exact on both sides)."""
    c, out = CASES[name], runs[name]
    delta = np.sqrt(np.where(np.isfinite(c["meas"][:, 2]), c["params"]["huber_delta2_stereo"] if "huber_delta2_stereo" in c["params"] else 7.815,
                             c["params"].get("huber_delta2_mono", 5.991)))
    for row in out["trace"]:
        on = row["lin"]["on"]
        assert np.abs(np.sqrt(row["lin"]["chi2"][on]) - delta[on]).min() >= 1e-3
        if row["converged"] not in (R.RESIDUAL, R.GRADIENT) and row["F_trial"] == row["F_trial"] and row["pred"] > 0:
            assert abs(row["rho"]) > 1e-3, (name, row["rho"])
    on = c["active"] & ~out["behind"]
    assert np.abs(np.sqrt(out["chi2"][on]) - delta[on]).min() >= 1e-3


def test_the_room_pipeline_on_the_restatements_lowers_the_trajectory_error():
    """What KeyframeGraphRgbd.bundle_adjust does on the GPU, from the numpy restatements alone (orb_reference for features and matches,
    bundle_reference for the two phases): the figures of profiles/bundle_adjust/README.md."""
    p = C.room_problem()
    first, second, active, mean = C.restated_two_phase(p)
    start = C.trajectory_error(p["start"], p["truth"])
    end = C.trajectory_error(np.linalg.inv(second["cameras"]), p["truth"])
    print(f"room: {len(p['tracks'])} tracks, {len(p['idx'])} observations, {int(active.sum())} active; trajectory error {start:.4f} m -> {end:.4f} m; "
          f"mean chi2 {first['chi2_initial'] / len(p['idx']):.3f} -> {mean:.3f}")
    assert len(p["frames"]) >= 7 and second["success"] and end < start and mean < first["chi2_initial"] / len(p["idx"])
    assert np.array_equal(second["cameras"][0], p["cameras"][0])


# -- build_tracks --------------------------------------------------------------------------------------------------------------------

def pair(a, b, *matches):
    return a, b, np.array(matches, np.int64).reshape(-1, 2)


def test_tracks_follow_a_chain_in_a_fixed_order():
    tracks = B.build_tracks([pair(1, 2, (7, 3)), pair(0, 1, (5, 7), (2, 9)), pair(2, 3, (3, 0))], min_length=2)
    assert [t.tolist() for t in tracks] == [[[0, 2], [1, 9]], [[0, 5], [1, 7], [2, 3], [3, 0]]]
    assert [t.tolist() for t in B.build_tracks([pair(0, 1, (5, 7), (2, 9)), pair(1, 2, (7, 3))], min_length=3)] == [[[0, 5], [1, 7], [2, 3]]]


def test_a_track_with_two_keypoints_of_one_keyframe_is_dropped_whole():
    # keypoint 4 of keyframe 0 and keypoint 6 of keyframe 0 both reach keypoint 1 of keyframe 2
    tracks = B.build_tracks([pair(0, 1, (4, 8)), pair(1, 2, (8, 1)), pair(0, 2, (6, 1)), pair(0, 1, (3, 3))], min_length=2)
    assert [t.tolist() for t in tracks] == [[[0, 3], [1, 3]]]


def test_short_tracks_and_empty_lists():
    assert B.build_tracks([], min_length=2) == []
    assert B.build_tracks([pair(0, 1), pair(1, 2, (0, 0))], min_length=3) == []
    with pytest.raises(ValueError, match="min_length"):
        B.build_tracks([], min_length=1)
