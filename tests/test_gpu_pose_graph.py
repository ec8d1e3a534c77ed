"""GPU: hv_pose_graph_optimize against its numpy restatement (tests/pose_graph_reference.py) on the planted graphs of
tests/pose_graph_cases.py (N <= 257), and the keyframe graph end to end on the synthetic room.

The tolerance of the per-edge comparison is measured, not chosen: the restatement is evaluated once in numpy.longdouble on the states
the call traced, DEV = its largest deviation from the float64 restatement over all cases and quantities (each deviation relative to
the scale pose_graph_reference.scales gives the quantity), and the GPU is allowed BAR = 8 x DEV, the margin being for the different
summation order inside the 6 x 6 products.  Measured on an MI355X (profiles/pose_graph/README.md):
    DEV (float64 restatement against longdouble)   1.206e-15     BAR = 9.652e-15
    largest GPU deviation                            9.599e-16
Accepted flags and the stopping rule must match exactly; test_pose_graph_reference_cpu.py keeps every |rho| above 1e-3 so that this
is fair.  rho and the new lambda pass through the conjugate gradients, whose sums associate differently on the device: both solves
end at a preconditioned relative residual of 1e-10 (cg_tolerance of the cases, cg_max_iterations 1500 is not reached), so d agrees
to 1e-10 times the condition number of the preconditioned system (1.4e4 on the 257-ring, from its 1400 CG iterations), 1.4e-6; rho
= decrease / model decrease is stationary in d at the solution up to 1 - rho, so 1e-5 relative is a safe bound on rho, and 6e-5 on
the new lambda where Nielsen's factor is not clamped (d lambda / lambda <= 6 d rho); where it is clamped at 1/3, or lambda grows by
nu, the new lambda is equal bit for bit."""
import types

import numpy as np
import pytest
import torch

from tests import pose_graph_cases as C
from tests import pose_graph_reference as R

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in C.all_cases()}
QUANTITIES = ("r", "chi2", "l", "M", "g", "b")
RULES = {0: "max_iterations", 1: "gradient", 2: "step", 3: "decrease", 4: "residual"}


@pytest.fixture(scope="module")
def vol():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    return ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 12)


def call(vol, c, poses=None, **kw):
    return vol.optimize_pose_graph(c["poses"] if poses is None else poses, c["nodes"], c["Z"], c["info"], c["uncertain"], **{**c["params"], **kw})


@pytest.fixture(scope="module")
def runs(vol):
    """Every case once on the GPU with its trace, the restatement's own run, and per traced state the float64 and longdouble
    restatements with the GPU's linearisation.  -> ({name: dict}, DEV)"""
    out, dev = {}, 0.0
    for name, c in CASES.items():
        gpu = call(vol, c, trace=True)
        mu = c["params"].get("line_process_weight", 1.0)
        N = len(c["poses"])
        states = []
        for row in gpu.trace:
            args = (row["poses"], c["nodes"], c["Z"], c["info"], c["uncertain"], mu)
            ld = R.linearise(*args, dtype=np.longdouble)
            f64 = R.linearise(*args)
            ld["b"], f64["b"] = R.gradient(ld, c["nodes"], N), R.gradient(f64, c["nodes"], N)
            S = R.scales(ld, c["nodes"], row["poses"], c["Z"], c["info"], mu)
            got = vol.pose_graph_linearise(row["poses"], c["nodes"], c["Z"], c["info"], c["uncertain"], line_process_weight=mu)
            d_ref, d_gpu = R.deviation(f64, ld, S), R.deviation(got, ld, S)
            dev = max(dev, max(d_ref.values()))
            states.append(dict(ref=d_ref, gpu=d_gpu, S=S, ld=ld))
        out[name] = dict(gpu=gpu, ref=R.optimize(c["poses"], c["nodes"], c["Z"], c["info"], c["uncertain"], **c["params"]), states=states)
    worst = max(max(s["gpu"].values()) for r in out.values() for s in r["states"])
    print(f"\npose graph: DEV (float64 restatement against longdouble) = {dev:.3e}, largest GPU deviation = {worst:.3e}, BAR = {8 * dev:.3e}")
    return out, dev


# -- 1. step by step -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_every_iteration_matches_the_restatement(runs, name):
    c = CASES[name]
    all_runs, dev = runs
    run = all_runs[name]
    gpu, bar = run["gpu"], 8.0 * dev
    assert 0.0 < dev < 1e-12  # a float64 evaluation: a few units of 2^-53 against its scale
    nu = 2.0
    assert len(gpu.trace) == gpu.iterations >= 1
    for k, (row, st) in enumerate(zip(gpu.trace, run["states"])):
        print(name, k, {q: "%.2e/%.2e" % (st["gpu"][q], st["ref"][q]) for q in QUANTITIES}, "rho %.6f" % row["gain_ratio"])
        for q in QUANTITIES:
            assert st["gpu"][q] <= bar, (name, k, q, st["gpu"][q], bar)
        # the same state, damping and rule through the restatement's own step
        _, lam_new, nu_new, want = R.step(row["poses"], c["nodes"], c["Z"], c["info"], c["uncertain"], row["lambda_"], nu, k == 0, c["params"])
        if k == 0:
            # lambda_0 = lambda_scale max diag H: a sum of the M_e of a node, each within BAR of its scale
            slack = np.zeros(len(c["poses"]))
            np.add.at(slack, c["nodes"].ravel(), np.repeat(st["S"]["M"].ravel(), 2))
            assert abs(row["lambda_"] - want["lam"]) <= c["params"].get("lambda_scale", 1e-5) * bar * slack.max(), (row["lambda_"], want["lam"])
            _, lam_new, nu_new, want = R.step(row["poses"], c["nodes"], c["Z"], c["info"], c["uncertain"], row["lambda_"], nu, False, c["params"])
        assert row["accepted"] == want["accepted"] and row["converged"] == want["converged"], (name, k, row, want["rho"], want["converged"])
        scale = max(abs(want["F"]), np.abs(st["S"]["chi2"]).sum())
        assert abs(row["chi2"] - want["F"]) <= bar * scale * len(c["nodes"]), (name, k, row["chi2"], want["F"])
        assert abs(row["gradient_norm"] - want["gradient"]) <= bar * st["S"]["b"].max(), (name, k)
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
def test_exact_graphs_recover_the_truth(runs, name):
    c = CASES[name]
    run = runs[0][name]
    fixed = c["params"]["fixed"]
    want = C.aligned_error(run["ref"]["poses"], c["truth"], fixed)
    got = C.aligned_error(run["gpu"].poses, c["truth"], fixed)
    print(f"{name}: error against the truth, restatement {want:.3e}, GPU {got:.3e}")
    assert run["gpu"].success and np.array_equal(run["gpu"].poses[fixed], c["poses"][fixed])
    assert got <= 8.0 * want, (got, want)
    assert run["gpu"].kept.all() and run["gpu"].edges_kept == len(c["nodes"])
    assert run["gpu"].chi2_final <= run["gpu"].chi2_initial


def test_false_chord_is_cut_and_the_poses_are_those_without_it(runs):
    c = CASES["false_chord"]
    with_chord, without = runs[0]["false_chord"], runs[0]["no_chord"]
    gpu = with_chord["gpu"]
    assert gpu.success and not gpu.kept[-1] and gpu.kept[:-1].all() and gpu.edges_kept == len(c["nodes"]) - 1
    assert gpu.line_process[-1] < 0.25 and (gpu.line_process[:65] == 1.0).all()
    np.testing.assert_allclose(gpu.line_process, with_chord["ref"]["l"], rtol=1e-9, atol=0)
    want = C.aligned_error(with_chord["ref"]["poses"], c["truth"], 0)
    got = C.aligned_error(gpu.poses, without["gpu"].poses, 0)
    print(f"false chord: restatement against the truth {want:.3e}, GPU against its run without the chord {got:.3e}")
    assert got <= 8.0 * want


# -- 3. reproducibility and forms ----------------------------------------------------------------------------------------------------

def same(a, b):
    assert np.array_equal(np.asarray(a.poses.cpu() if torch.is_tensor(a.poses) else a.poses), np.asarray(b.poses.cpu() if torch.is_tensor(b.poses) else b.poses))
    lp = [np.asarray(x.line_process.cpu() if torch.is_tensor(x.line_process) else x.line_process) for x in (a, b)]
    assert np.array_equal(lp[0], lp[1])
    for f in ("chi2_initial", "chi2_final", "lambda_", "iterations", "cg_iterations_total", "edges_kept", "converged", "success"):
        assert getattr(a, f) == getattr(b, f), f


@pytest.mark.parametrize("name", ["ring257", "false_chord", "star70"])
def test_runs_and_operand_forms_are_bitwise_equal(vol, name):
    from pyslam_amd.volumetric import VoxelBlockGrid

    c = CASES[name]
    first = call(vol, c, trace=True)
    again = call(vol, c, trace=True)
    same(first, again)
    for ra, rb in zip(first.trace, again.trace):
        assert all(np.array_equal(ra[k], rb[k]) for k in ra)
    cuda = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cpu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    p = c["params"]
    dev = vol.optimize_pose_graph(cuda(c["poses"]), cuda(c["nodes"]), cuda(c["Z"]), cuda(c["info"]), cuda(c["uncertain"]), **p)
    assert torch.is_tensor(dev.poses) and dev.poses.is_cuda and dev.line_process.is_cuda and dev.kept.dtype == torch.bool
    same(first, dev)
    same(first, vol.optimize_pose_graph(cpu(c["poses"]), cpu(c["nodes"]), cpu(c["Z"]), cpu(c["info"]), cpu(c["uncertain"]), **p))
    # other dtypes and layouts of the same numbers, and a grid as the context
    same(first, vol.optimize_pose_graph(np.asfortranarray(c["poses"]), c["nodes"].astype(np.int64), c["Z"],
                                        c["info"], None if c["uncertain"] is None else c["uncertain"].astype(bool), **p))
    same(first, call(VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12), c))
    assert np.array_equal(np.asarray(dev.kept.cpu()), first.kept)


def test_results_are_ordered_on_torchs_current_stream(vol):
    """CUDA operands written by asynchronous torch work just before the call are read after it, and the result tensors can be used
    on torch's current stream right after the call."""
    c = CASES["ring65"]
    want = call(vol, c)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    poses, nodes, Z, info = cuda(c["poses"]), cuda(c["nodes"]), cuda(c["Z"]), cuda(c["info"])
    buf = torch.zeros_like(poses)
    x = torch.full((2048, 2048), 1e-3, device="cuda")
    torch.cuda.synchronize()
    for _ in range(20):  # work the write has to wait behind
        x = (x @ x).clamp_(-1.0, 1.0)
    buf.copy_(poses)
    out = vol.optimize_pose_graph(buf, nodes, Z, info, **c["params"])
    doubled = out.poses * 2.0  # on torch's current stream, no synchronisation in between
    assert np.array_equal(doubled.cpu().numpy(), want.poses * 2.0)
    assert np.array_equal(buf.cpu().numpy(), c["poses"])  # the operand is not written


# -- 4. errors -----------------------------------------------------------------------------------------------------------------------

def test_rejected_inputs_raise_before_any_launch(vol):
    from pyslam_amd import _lib as L

    c = CASES["duplicates"]
    poses, nodes, Z, info = c["poses"], c["nodes"], c["Z"], c["info"]
    N, E = len(poses), len(nodes)

    def raw(poses, nodes, Z, info, unc=None, fixed=0, n=None, loc=L.HV_HOST):
        """The C ABI itself on the caller's own poses buffer."""
        prm = L.HvPoseGraphParams()
        vol._lib.hv_pose_graph_default_params(L.ctypes.byref(prm))
        prm.fixed = fixed
        res = L.HvPoseGraphResult()
        return vol._lib.hv_pose_graph_optimize(vol._h, L.ptr(poses), len(poses) if n is None else n, L.ptr(nodes), L.ptr(Z), L.ptr(info), L.ptr(unc),
                                               len(nodes), L.ctypes.byref(prm), None, L.ctypes.byref(res), None, None, 0, None, loc)

    def edit(a, index, value):
        b = a.copy()
        b[index] = value
        return b

    asym = info.copy()
    asym[3, 1, 2] += 1e-12
    unc_only = np.zeros(E, np.uint8)
    unc_only[[10, 11]] = 1  # node 11 hangs on edges 10 = (10, 11), 11 = (11, 0) and 16 = (11, 4): all three uncertain
    unc_only[16] = 1
    bad = [("need 1 ..", dict(n=0)), ("fixed node", dict(fixed=N)), ("fixed node", dict(fixed=-1)),
           ("outside 0..", dict(nodes=edit(nodes, (2, 1), N))), ("outside 0..", dict(nodes=edit(nodes, (2, 0), -1))),
           ("to itself", dict(nodes=edit(nodes, (5, 1), 5))),
           ("pose 3 is not finite", dict(poses=edit(poses, (3, 0, 3), np.nan))), ("pose 7 is not finite", dict(poses=edit(poses, (7, 1, 1), np.inf))),
           ("bottom row", dict(poses=edit(poses, (2, 3, 3), 2.0))), ("bottom row", dict(poses=edit(poses, (2, 3, 0), 1e-300))),
           ("transformation of edge 4", dict(Z=edit(Z, (4, 2, 3), np.nan))), ("transformation of edge 6", dict(Z=edit(Z, (6, 3, 1), 0.5))),
           ("information matrix of edge 2", dict(info=edit(info, (2, 0, 0), np.inf))), ("not symmetric", dict(info=asym)),
           ("not connected to the fixed node", dict(unc=unc_only)), ("union-find", dict(unc=unc_only))]
    vol.synchronize()
    vol.profile_enable(True)
    vol.profile_read()
    for loc in (L.HV_HOST, L.HV_DEVICE):
        for message, change in bad:
            args = {**dict(poses=poses.copy(), nodes=nodes, Z=Z, info=info), **{k: v for k, v in change.items() if k not in ("n", "fixed")}}
            args = {k: np.ascontiguousarray(v) for k, v in args.items()}
            before = args["poses"].copy()
            if loc == L.HV_DEVICE:
                args = {k: torch.from_numpy(v).cuda() for k, v in args.items()}
            with pytest.raises(L.HipVolError, match=message):
                L.check(raw(loc=loc, **args, **{k: v for k, v in change.items() if k in ("n", "fixed")}))
            after = args["poses"].cpu().numpy() if loc == L.HV_DEVICE else args["poses"]
            assert np.array_equal(after, before, equal_nan=True), message
    _, launches, _ = vol.profile_read()
    vol.profile_enable(False)
    assert launches == 0, "a refused call queued a launch"
    # a graph that hangs together through an uncertain edge alone, in the binding's words
    with pytest.raises(L.HipVolError, match="through certain edges"):
        vol.optimize_pose_graph(poses[:2], [(0, 1)], Z[:1], info[:1], uncertain=[True])
    # not errors: one node and no edge; duplicate and backward edges (the case itself)
    out = vol.optimize_pose_graph(poses[:1], np.zeros((0, 2), np.int32), np.zeros((0, 4, 4)), np.zeros((0, 6, 6)))
    assert out.success and out.iterations == 0 and np.array_equal(out.poses, poses[:1]) and out.line_process.shape == (0,)
    assert call(vol, c).success


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
    out = call(fused, CASES["false_chord"])
    assert out.success
    after = fused.dump()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert fused.num_blocks() == blocks and np.array_equal(fused.dirty_keys(), dirty)


# -- 6. end to end -------------------------------------------------------------------------------------------------------------------

def ate(poses, truth):
    """Absolute trajectory error: the root mean square distance of the camera centres from the truth, both starting at the true first
    pose (no further alignment)."""
    return float(np.sqrt(((poses[:, :3, 3] - truth[:, :3, 3]) ** 2).sum(1).mean()))


def test_keyframe_graph_closes_the_loop_of_the_room():
    """One full orbit of the 160x120 room in 120 frames (3 degrees a frame), every frame a keyframe."""
    from pyslam_amd.pose_graph import KeyframeGraphRgbd
    from pyslam_amd.synthetic import SyntheticRGBD
    from pyslam_amd.volumetric import PinholeCameraIntrinsic, ScalableTSDFVolume

    n = 120
    s = SyntheticRGBD("tiny_160x120_2cm", n_poses=n)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    cam = types.SimpleNamespace(fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, width=s.width, height=s.height)
    frames = [s[i] for i in range(n)]
    truth = np.array([np.linalg.inv(s.pose(i)) for i in range(n)])
    vol = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 14)
    # intensity_weight 0.1: what INTEGRATION section 21 measured as the better weight beyond one-frame baselines
    kg = KeyframeGraphRgbd(vol, cam, method="hybrid", T_wc0=truth[0], depth_max=5.0, intensity_weight=0.1)
    for depth, rgb, _ in frames:
        kg.add_frame(rgb, depth)
    assert kg.lost_nodes == [] and len(kg.graph.poses) == n and len(kg.graph.edges) == n - 1
    before = kg.graph.poses
    old_extrinsics = kg.extrinsics()
    depths, colors = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    vol.integrate_batch(depths, colors, K, old_extrinsics)
    added = kg.close_loops(max_distance=0.4, max_angle=0.5, min_gap=n - 10)
    edges = kg.graph.edges
    ends = [e for e in added if edges[e, 0] >= n - 3 and edges[e, 1] <= 2]
    assert ends, "no loop edge between the ends of the orbit"
    res = kg.optimize(line_process_weight=kg.graph.line_process_weight(0.2), cg_max_iterations=1000)
    assert res.success and all(res.kept[e] for e in ends) and res.kept[:n - 1].all()
    e_before, e_after = ate(before, truth), ate(kg.graph.poses, truth)
    print(f"\nend to end: {len(added)} loop edges, {int(res.kept[n - 1:].sum())} kept, {res.iterations} iterations ({res.converged}), "
          f"chi2 {res.chi2_initial:.4g} -> {res.chi2_final:.4g}, ATE before {e_before * 1e3:.2f} mm, after {e_after * 1e3:.2f} mm, "
          f"ratio {e_after / e_before:.3f}")
    assert e_after < e_before
    # reintegrate_batch's contract, from the graph's output: the map moved to the corrected poses is the map fused at them
    vol.reintegrate_batch(depths, colors, K, old_extrinsics, kg.extrinsics())
    fresh = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 14)
    fresh.integrate_batch(depths, colors, K, kg.extrinsics())
    (km, *moved), (kf, *want) = vol.dump(), fresh.dump()
    index = {tuple(k): i for i, k in enumerate(km)}
    sel = np.array([index[tuple(k)] for k in kf], np.int64)  # KeyError: the fresh map holds a unit the moved one does not
    for a, b, name in zip(moved, want, ("tsdf", "weight", "colour")):
        assert np.array_equal(a[sel].view(np.uint8), b.view(np.uint8)), name
    rest = np.setdiff1d(np.arange(len(km)), sel)  # units only the old poses touched are left in the fresh state, not removed
    assert all(not a[rest].any() for a in moved)
