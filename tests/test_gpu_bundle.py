"""GPU: hv_bundle_adjust against its numpy restatement (tests/bundle_reference.py) on the planted problems of tests/bundle_cases.py
(N <= 70, M <= 1 100, O <= 2 100).

The tolerance of the per-quantity comparison is measured, not chosen: the restatement is evaluated once in numpy.longdouble on the
states the call traced, DEV = its largest deviation from the float64 restatement over all cases and quantities (each deviation
relative to the scale bundle_reference.scales gives the quantity), and the GPU is allowed BAR = 8 x DEV, the pose graph's margin, for
the different association inside the small products (the library forms W^T (w s J^T J) W, the restatement (J W)^T (J W) w s).
Measured on an MI355X (profiles/bundle_adjust/README.md):
    DEV (float64 restatement against longdouble)   7.028e-16     BAR = 5.623e-15
    largest GPU deviation                            4.268e-16
Accepted flags and the stopping rule must match exactly; test_bundle_reference_cpu.py keeps every |rho_gain| above 1e-3 and every
sqrt(chi2) 1e-3 from its delta so that this is fair.  rho_gain and the new lambda pass through the conjugate gradients, whose sums
associate differently on the device: both solves end at a preconditioned relative residual of 1e-10 (cg_tolerance of the cases;
cg_max_iterations 300 is not reached: the longest solve of the restatement takes 37 iterations), so the camera step agrees to 1e-10
times the condition number of the preconditioned reduced system, below 37^2 ~ 1.4e3 by the iteration count, 1.4e-7, and the
back-substituted points inherit it; rho_gain = decrease / model decrease is stationary in d at the solution up to 1 - rho_gain, so
1e-5 relative is a safe bound on rho_gain - the pose graph's - and 6e-5 on the new lambda where Nielsen's factor is not clamped
(d lambda / lambda <= 6 d rho); where it is clamped at 1/3, or lambda grows by nu, the new lambda is equal bit for bit."""
import numpy as np
import pytest
import torch

from tests import bundle_cases as C
from tests import bundle_reference as R

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in C.all_cases()}
QUANTITIES = ("r", "chi2", "w", "B", "bc", "C", "bp")
RULES = {0: "max_iterations", 1: "gradient", 2: "step", 3: "decrease", 4: "residual"}
PINHOLE = ("fx", "fy", "cx", "cy", "bf")


class Pinhole:
    def __init__(self, p):
        self.fx, self.fy, self.cx, self.cy = p["fx"], p["fy"], p["cx"], p["cy"]


@pytest.fixture(scope="module")
def vol():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    return ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 12)


def keywords(c):
    p = {k: v for k, v in c["params"].items() if k not in PINHOLE and k not in ("huber", "fixed_points")}
    return dict(bf=c["params"]["bf"], inv_sigma2=c["inv_sigma2"], huber=c["params"].get("huber", True),
                fixed_points=c["params"].get("fixed_points", False), **p)


def call(vol, c, form=lambda a: a, **kw):
    return vol.bundle_adjust(form(c["cameras"]), form(c["points"]), form(c["idx"]), form(c["meas"]), Pinhole(c["params"]),
                             active=form(c["active"]), camera_fixed=form(c["fixed"]), **{**keywords(c), "inv_sigma2": form(c["inv_sigma2"]), **kw})


def measurements(c):
    return np.c_[c["meas"], c["inv_sigma2"]]


@pytest.fixture(scope="module")
def runs(vol):
    """Every case once on the GPU with its trace, the restatement's own run, and per traced state the float64 and longdouble
    restatements with the GPU's linearisation.  -> ({name: dict}, DEV)"""
    out, dev = {}, 0.0
    for name, c in CASES.items():
        gpu = call(vol, c, trace=True)
        N, M, meas, P = len(c["cameras"]), len(c["points"]), measurements(c), c["params"]
        states = []
        for k, row in enumerate(gpu.trace):
            on = c["active"] if k == 0 else c["active"] & ~gpu.behind
            args = (row["cameras"], row["points"], c["idx"], meas, on, P)
            ld, f64 = R.linearise(*args, dtype=np.longdouble), R.linearise(*args)
            bl, b64 = R.blocks(ld, c["idx"], N, M), R.blocks(f64, c["idx"], N, M)
            S = R.scales(ld, bl, row["cameras"], row["points"], c["idx"], meas, {**R.DEFAULTS, **P})
            kw = keywords(c)
            got = vol.bundle_linearise(row["cameras"], row["points"], c["idx"], c["meas"], Pinhole(P), bf=kw["bf"], inv_sigma2=c["inv_sigma2"],
                                       active=on, huber=kw["huber"])
            d_ref, d_gpu = R.deviation({**f64, **b64}, {**ld, **bl}, S), R.deviation(got, {**ld, **bl}, S)
            dev = max(dev, max(d_ref.values()))
            states.append(dict(ref=d_ref, gpu=d_gpu, S=S, ld=ld, got=got, f64=f64))
        ref = R.optimize(c["cameras"], c["points"], c["idx"], meas, c["active"], c["fixed"], **P)
        out[name] = dict(gpu=gpu, ref=ref, states=states)
    worst = max(max(s["gpu"].values()) for r in out.values() for s in r["states"])
    print(f"\nbundle: DEV (float64 restatement against longdouble) = {dev:.3e}, largest GPU deviation = {worst:.3e}, BAR = {8 * dev:.3e}")
    return out, dev


# -- 1. step by step -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_every_iteration_matches_the_restatement(runs, name):
    c = CASES[name]
    all_runs, dev = runs
    run = all_runs[name]
    gpu, bar, P, meas = run["gpu"], 8.0 * dev, c["params"], measurements(c)
    assert 0.0 < dev < 1e-12  # a float64 evaluation: a few units of 2^-53 against its scale
    nu = 2.0
    assert len(gpu.trace) == gpu.iterations >= 1
    for k, (row, st) in enumerate(zip(gpu.trace, run["states"])):
        print(name, k, {q: "%.2e/%.2e" % (st["gpu"][q], st["ref"][q]) for q in QUANTITIES}, "rho %.6f" % row["gain_ratio"])
        for q in QUANTITIES:
            assert st["gpu"][q] <= bar, (name, k, q, st["gpu"][q], bar)
        on = c["active"] if k == 0 else c["active"] & ~gpu.behind
        assert np.array_equal(st["got"]["behind"], st["f64"]["low"])
        # the same state, damping and rule through the restatement's own step
        step = lambda first: R.step(row["cameras"], row["points"], c["idx"], meas, on, c["fixed"], row["lambda_"], nu, first, P)
        *_, lam_new, nu_new, want = step(k == 0)
        if k == 0:
            # lambda_0 = lambda_scale max diag H: a block is a sum of terms, each within BAR of its scale
            slack = max(st["S"]["B"].max(), st["S"]["C"].max())
            assert abs(row["lambda_"] - want["lam"]) <= P.get("lambda_scale", 1e-5) * bar * slack, (row["lambda_"], want["lam"])
            *_, lam_new, nu_new, want = step(False)
        assert row["accepted"] == want["accepted"] and row["converged"] == want["converged"], (name, k, row, want["rho"], want["converged"])
        scale = max(abs(want["F"]), np.abs(st["S"]["chi2"]).sum())
        assert abs(row["chi2"] - want["F"]) <= bar * scale * len(c["idx"]), (name, k, row["chi2"], want["F"])
        assert abs(row["gradient_norm"] - want["gradient"]) <= bar * max(st["S"]["bc"].max(), st["S"]["bp"].max()), (name, k)
        assert (row["chi2_trial"] != row["chi2_trial"]) == (want["F_trial"] != want["F_trial"])  # B4: not-a-number on both sides or on neither
        if want["converged"] in (R.GRADIENT, R.RESIDUAL):
            assert row["lambda_new"] == row["lambda_"]
        else:
            assert abs(row["gain_ratio"] - want["rho"]) <= 1e-5 * max(1.0, abs(want["rho"])), (name, k, row["gain_ratio"], want["rho"])
            clamped = not want["accepted"] or 1.0 - (2.0 * want["rho"] - 1.0) ** 3 < 1.0 / 3.0 - 1e-4
            if clamped:
                assert row["lambda_new"] == lam_new, (name, k, row["lambda_new"], lam_new)
            else:
                assert abs(row["lambda_new"] - lam_new) <= 6e-5 * lam_new, (name, k, row["lambda_new"], lam_new)
        nu = nu_new
    assert gpu.converged == RULES[run["ref"]["converged"]] and gpu.success == run["ref"]["success"]
    assert gpu.iterations == run["ref"]["iterations"]


# -- 2. end results ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["exact"]))
def test_exact_cases_recover_the_truth(runs, name):
    c = CASES[name]
    run = runs[0][name]
    want = C.pose_error(run["ref"]["cameras"], c["truth_cameras"])
    got = C.pose_error(run["gpu"].cameras, c["truth_cameras"])
    seen = np.zeros(len(c["points"]), bool)
    seen[c["idx"][c["active"] & ~run["ref"]["behind"], 1]] = True
    want_p = np.abs(run["ref"]["points"] - c["truth_points"])[seen].max()
    got_p = np.abs(run["gpu"].points - c["truth_points"])[seen].max()
    print(f"{name}: error against the truth, restatement {want:.3e} / {want_p:.3e}, GPU {got:.3e} / {got_p:.3e}")
    assert run["gpu"].success and np.array_equal(run["gpu"].cameras[c["fixed"]], c["cameras"][c["fixed"]])
    assert got <= 8.0 * want and got_p <= 8.0 * want_p, (got, want, got_p, want_p)
    assert run["gpu"].chi2_final <= run["gpu"].chi2_initial


def test_the_outlier_case_marks_the_planted_observations_and_no_others(runs):
    c, gpu = CASES["outliers"], runs[0]["outliers"]["gpu"]
    assert gpu.success and np.array_equal(~gpu.inlier, c["outliers"]) and not gpu.behind.any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_flags_and_chi2_equal_the_restatements(runs, name):
    run = runs[0][name]
    gpu, ref = run["gpu"], run["ref"]
    assert np.array_equal(gpu.behind, ref["behind"]) and np.array_equal(gpu.inlier, ref["inlier"])
    np.testing.assert_allclose(gpu.chi2, ref["chi2"], rtol=1e-6, atol=1e-9 * max(1.0, ref["chi2_initial"]))


def test_isolated_variables_come_back_bit_identical(runs):
    c, gpu = CASES["inactive"], runs[0]["inactive"]["gpu"]
    assert np.array_equal(gpu.cameras[3], c["cameras"][3]) and np.array_equal(gpu.points[11], c["points"][11])
    assert not np.array_equal(gpu.cameras[1], c["cameras"][1])
    g, gpu = CASES["gather_edges"], runs[0]["gather_edges"]["gpu"]
    assert np.array_equal(gpu.points[1025:], g["points"][1025:]) and np.array_equal(gpu.cameras[0], g["cameras"][0])
    p, gpu = CASES["pose_only"], runs[0]["pose_only"]["gpu"]
    assert np.array_equal(gpu.points, p["points"]) and max(r["cg_iterations"] for r in gpu.trace) <= 1
    o, gpu = CASES["points_only"], runs[0]["points_only"]["gpu"]
    assert np.array_equal(gpu.cameras, o["cameras"]) and not np.array_equal(gpu.points, o["points"])


def test_the_depth_rules(runs):
    a = runs[0]["behind_at_start"]["gpu"]
    assert a.behind.sum() == 1 and a.behind[-1] and a.chi2[-1] == 0.0 and a.success
    t = runs[0]["behind_in_trial"]["gpu"]
    nan_rows = [r for r in t.trace if r["chi2_trial"] != r["chi2_trial"]]
    assert nan_rows and all(not r["accepted"] and r["gain_ratio"] == 0.0 for r in nan_rows) and not t.behind.any() and t.success


# -- 3. reproducibility and forms ----------------------------------------------------------------------------------------------------

def host(a):
    return np.asarray(a.cpu()) if torch.is_tensor(a) else np.asarray(a)


def same(a, b):
    for f in ("cameras", "points", "chi2", "behind", "inlier"):
        assert np.array_equal(host(getattr(a, f)), host(getattr(b, f))), f
    for f in ("chi2_initial", "chi2_final", "lambda_", "iterations", "cg_iterations_total", "converged", "success"):
        assert getattr(a, f) == getattr(b, f), f


@pytest.mark.parametrize("name", ["gather_edges", "mixed", "inactive"])
def test_runs_and_operand_forms_are_bitwise_equal(vol, name):
    from pyslam_amd.volumetric import VoxelBlockGrid

    c = CASES[name]
    before = {k: np.array(c[k]) for k in ("cameras", "points", "idx", "meas", "inv_sigma2", "active", "fixed")}
    first = call(vol, c, trace=True)
    again = call(vol, c, trace=True)
    same(first, again)
    for ra, rb in zip(first.trace, again.trace):
        assert all(np.array_equal(ra[k], rb[k], equal_nan=True) for k in ra)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cpu = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    dev_in = {k: cuda(v) for k, v in before.items()}
    dev = vol.bundle_adjust(dev_in["cameras"], dev_in["points"], dev_in["idx"], dev_in["meas"], Pinhole(c["params"]), active=dev_in["active"],
                            camera_fixed=dev_in["fixed"], **{**keywords(c), "inv_sigma2": dev_in["inv_sigma2"]})
    assert torch.is_tensor(dev.cameras) and dev.cameras.is_cuda and dev.points.is_cuda and dev.chi2.is_cuda and dev.inlier.dtype == torch.bool
    same(first, dev)
    same(first, call(vol, c, form=cpu))
    # other dtypes and layouts of the same numbers, and a grid as the context
    other = dict(c, cameras=np.asfortranarray(c["cameras"]), points=np.asfortranarray(c["points"]), idx=c["idx"].astype(np.int64),
                 meas=np.asfortranarray(c["meas"]), active=c["active"].astype(np.uint8), fixed=c["fixed"].astype(np.int64))
    same(first, call(vol, other))
    same(first, call(VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12), c))
    # operands are not written, on either side
    for k, v in before.items():
        assert np.array_equal(c[k], v, equal_nan=True) and np.array_equal(dev_in[k].cpu().numpy(), v, equal_nan=True), k


def test_results_are_ordered_on_torchs_current_stream(vol):
    c = CASES["mixed"]
    want = call(vol, c)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cams = cuda(c["cameras"])
    buf = torch.zeros_like(cams)
    x = torch.full((2048, 2048), 1e-3, device="cuda")
    torch.cuda.synchronize()
    for _ in range(20):  # work the write has to wait behind
        x = (x @ x).clamp_(-1.0, 1.0)
    buf.copy_(cams)
    out = vol.bundle_adjust(buf, cuda(c["points"]), cuda(c["idx"]), cuda(c["meas"]), Pinhole(c["params"]), active=cuda(c["active"]),
                            camera_fixed=cuda(c["fixed"]), **{**keywords(c), "inv_sigma2": cuda(c["inv_sigma2"])})
    doubled = out.cameras * 2.0  # on torch's current stream, no synchronisation in between
    assert np.array_equal(doubled.cpu().numpy(), want.cameras * 2.0)
    assert np.array_equal(buf.cpu().numpy(), c["cameras"])


# -- 4. errors -----------------------------------------------------------------------------------------------------------------------

def test_rejected_inputs_raise_before_any_launch(vol):
    from pyslam_amd import _lib as L

    c = CASES["mixed"]
    N, M, O = len(c["cameras"]), len(c["points"]), len(c["idx"])
    base = dict(cams=c["cameras"], pts=c["points"], fixed=c["fixed"].astype(np.uint8), idx=c["idx"], meas=measurements(c))

    def raw(cams, pts, fixed, idx, meas, n=None, m=None, loc=L.HV_HOST, **fields):
        """The C ABI itself on the caller's own state buffers."""
        prm = L.HvBundleParams()
        vol._lib.hv_bundle_default_params(L.ctypes.byref(prm))
        for k in PINHOLE:
            setattr(prm, k, c["params"][k])
        for k, v in fields.items():
            setattr(prm, k, v)
        res = L.HvBundleResult()
        return vol._lib.hv_bundle_adjust(vol._h, L.ptr(cams), N if n is None else n, L.ptr(pts), M if m is None else m, L.ptr(fixed), L.ptr(idx),
                                         L.ptr(meas), None, len(idx), L.ctypes.byref(prm), None, None, L.ctypes.byref(res), None, None, None, 0, None,
                                         loc)

    def edit(a, index, value):
        b = a.copy()
        b[index] = value
        return b

    scalars = ("n", "m", "fx", "fy", "bf", "lambda_scale", "cg_tolerance", "max_iterations", "cg_max_iterations", "min_depth", "huber_delta2_mono",
               "step_tolerance")
    bad = [("at least one camera and one point", dict(n=0)), ("at least one camera and one point", dict(m=0)),
           ("outside 0..", dict(idx=edit(c["idx"], (2, 0), N))), ("outside 0..", dict(idx=edit(c["idx"], (2, 1), -1))),
           ("outside 0..", dict(idx=edit(c["idx"], (7, 1), M))),
           ("camera 1 is not finite", dict(cams=edit(c["cameras"], (1, 0, 3), np.nan))), ("point 4 is not finite", dict(pts=edit(c["points"], (4, 1), np.inf))),
           ("observation 5 has a pixel", dict(meas=edit(base["meas"], (5, 0), np.nan))), ("observation 6 has a pixel", dict(meas=edit(base["meas"], (6, 1), np.inf))),
           ("bottom row", dict(cams=edit(c["cameras"], (2, 3, 3), 2.0))), ("bottom row", dict(cams=edit(c["cameras"], (2, 3, 0), 1e-300))),
           ("inv_sigma2", dict(meas=edit(base["meas"], (3, 3), 0.0))), ("inv_sigma2", dict(meas=edit(base["meas"], (3, 3), np.nan))),
           ("no camera is fixed", dict(fixed=np.zeros(N, np.uint8))),
           ("fx, fy and bf", dict(fx=0.0)), ("fx, fy and bf", dict(fy=-1.0)), ("fx, fy and bf", dict(bf=0.0)),
           ("lambda_scale", dict(lambda_scale=0.0)), ("tolerance", dict(cg_tolerance=1.0)), ("tolerance", dict(step_tolerance=-1.0)),
           ("max_iterations", dict(max_iterations=0)), ("max_iterations", dict(cg_max_iterations=10001)), ("min_depth", dict(min_depth=-1.0)),
           ("Huber", dict(huber_delta2_mono=0.0))]
    vol.synchronize()
    vol.profile_enable(True)
    vol.profile_read()
    for loc in (L.HV_HOST, L.HV_DEVICE):
        for message, change in bad:
            args = {**{k: v.copy() for k, v in base.items()}, **{k: v for k, v in change.items() if k not in scalars}}
            args = {k: np.ascontiguousarray(v) for k, v in args.items()}
            before = (args["cams"].copy(), args["pts"].copy())
            if loc == L.HV_DEVICE:
                args = {k: torch.from_numpy(v).cuda() for k, v in args.items()}
            with pytest.raises(L.HipVolError, match=message):
                L.check(raw(loc=loc, **args, **{k: v for k, v in change.items() if k in scalars}))
            after = tuple(host(args[k]) for k in ("cams", "pts"))
            assert np.array_equal(after[0], before[0], equal_nan=True) and np.array_equal(after[1], before[1], equal_nan=True), message
    _, launches, _ = vol.profile_read()
    vol.profile_enable(False)
    assert launches == 0, "a refused call queued a launch"
    # not errors: no observation at all; every camera fixed with the points free (the points_only case)
    out = vol.bundle_adjust(c["cameras"], c["points"], np.zeros((0, 2), np.int32), np.zeros((0, 3)), Pinhole(c["params"]), bf=12.0)
    assert out.success and out.iterations == 0 and np.array_equal(out.cameras, c["cameras"]) and np.array_equal(out.points, c["points"])
    assert out.chi2.shape == (0,) and out.converged == "residual"
    out = vol.bundle_adjust(np.zeros((0, 4, 4)), np.zeros((0, 3)), np.zeros((0, 2), np.int32), np.zeros((0, 2)), Pinhole(c["params"]), bf=12.0)
    assert out.success and out.cameras.shape == (0, 4, 4)
    assert call(vol, CASES["points_only"]).success


# -- 5. the map is untouched ---------------------------------------------------------------------------------------------------------

def test_the_map_is_untouched():
    from pyslam_amd.synthetic import SyntheticRGBD
    from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume

    s = SyntheticRGBD("tiny_160x120_2cm")
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    fused = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 12)
    for i in (40, 41):
        depth, rgb, T = s[i]
        fused.integrate(RGBDImage.create_from_color_and_depth(rgb, depth, 1.0, 4.0, False), K, T)
    before, blocks, dirty = fused.dump(), fused.num_blocks(), fused.dirty_keys()
    out = call(fused, CASES["gather_edges"])
    assert out.success
    after = fused.dump()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert fused.num_blocks() == blocks and np.array_equal(fused.dirty_keys(), dirty)


# -- 6. end to end -------------------------------------------------------------------------------------------------------------------

def test_keyframe_graph_bundle_adjusts_the_room():
    """Eight keyframes of the 160x120 room at the truth moved by planted offsets (bundle_cases.ROOM_OFFSETS), node 0 fixed.  The
    library's features and matches equal the restatements' bit for bit (tests/test_gpu_features.py), so the graph poses the same
    problem as bundle_cases.room_problem and the two-phase runs can be compared pose by pose: each outer iteration's step agrees to
    1.4e-7 of its length (the module docstring), the steps are below 0.3, twenty iterations and a factor ten for what a later
    iteration makes of an earlier difference give 1e-5 on every entry of a pose, hence 2e-5 m on the trajectory error."""
    from pyslam_amd.pose_graph import KeyframeGraphRgbd
    from pyslam_amd.volumetric import ScalableTSDFVolume

    p = C.room_problem()
    _, want, active, want_mean = C.restated_two_phase(p)
    vol = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)
    kg = KeyframeGraphRgbd(vol, p["cam"], method="hybrid", T_wc0=p["truth"][0], features=C.ROOM_FEATURES, depth_max=5.0)
    for depth, rgb, _ in p["frames"]:
        kg.add_frame(rgb, depth)
    assert len(kg.graph.poses) == len(p["frames"]) >= 7
    kg.graph._poses = [T.copy() for T in p["start"]]
    result, mean = kg.bundle_adjust(p["bf"], min_length=C.ROOM_MIN_LENGTH, rounds=C.ROOM_ROUNDS, match_params=dict(max_distance=C.ROOM_MATCH["max_distance"], ratio=C.ROOM_MATCH["ratio_percent"] / 100.0,
                                                     cross_check=bool(C.ROOM_MATCH["cross_check"])), **C.ROOM_SOLVE)
    log = kg.bundle_log
    assert np.array_equal(log["index"], p["idx"]) and np.array_equal(log["measurements"], p["meas"], equal_nan=True)
    assert np.array_equal(log["points"], p["points"]) and np.array_equal(log["active"], active)
    start, ref = C.trajectory_error(p["start"], p["truth"]), C.trajectory_error(np.linalg.inv(want["cameras"]), p["truth"])
    got = C.trajectory_error(kg.graph.poses, p["truth"])
    before = float(R.linearise(p["cameras"], p["points"], p["idx"], measurements(p), np.ones(len(p["idx"]), bool), p["params"])["chi2"].mean())
    print(f"room: trajectory error {start:.4f} m at the start, restatement {ref:.4f} m, GPU {got:.4f} m; mean chi2 {before:.3f} -> {mean:.3f}")
    assert result.success and mean < before
    assert np.abs(host(result.cameras) - want["cameras"]).max() <= 1e-5 and abs(got - ref) <= 2e-5
    assert abs(mean - want_mean) <= 1e-4 * want_mean
    assert ref < start
    assert np.array_equal(host(result.cameras)[0], p["cameras"][0])  # node 0 is fixed
