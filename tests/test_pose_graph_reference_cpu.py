"""CPU: the numpy restatement of hv_pose_graph_optimize (tests/pose_graph_reference.py) held against itself - Log and exp invert each
other across the branches, the analytic Jacobians equal central differences of its own residual, its two inner solvers reach the
same optimum, exact graphs recover the truth, the line process switches the planted false chord off and no accept / reject
decision sits near rounding."""
import numpy as np
import pytest

from tests import pose_graph_cases as C
from tests import pose_graph_reference as R

CASES = {c["name"]: c for c in C.all_cases()}


def run(case, solver=R.solve_pcg):
    return R.optimize(case["poses"], case["nodes"], case["Z"], case["info"], case["uncertain"], solver=solver, **case["params"])


@pytest.fixture(scope="module")
def solved():
    return {name: run(c) for name, c in CASES.items()}


def optimum_bound(case, out_a, out_b=None):
    """How far two states that both satisfy the gradient rule may lie apart: |dx|_2 <= (|b_a|_2 + |b_b|_2) / lambda_min(H) for the
    quadratic model, H the dense matrix of the free nodes at a; doubled for what the model leaves out, plus 1e-12 for rounding."""
    p = case["params"]
    N, fixed = len(case["poses"]), p["fixed"]
    mu = p.get("line_process_weight", 1.0)
    lin = R.linearise(out_a["poses"], case["nodes"], case["Z"], case["info"], case["uncertain"], mu)
    free = np.ones(6 * N, bool)
    free[6 * fixed:6 * fixed + 6] = False
    lam_min = np.linalg.eigvalsh(R.dense_system(lin, case["nodes"], N)[np.ix_(free, free)])[0]
    assert lam_min > 0
    norm = 0.0
    for out in (out_a, out_b):
        if out is not None:
            l2 = R.linearise(out["poses"], case["nodes"], case["Z"], case["info"], case["uncertain"], mu)
            norm += np.linalg.norm(R.gradient(l2, case["nodes"], N, fixed))
    return 2.0 * norm / lam_min + 1e-12


def test_log_inverts_exp_across_the_branches():
    rng = np.random.default_rng(5)
    axes = rng.standard_normal((40, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    # the small-angle branch, the generic one, either side of the near-pi threshold (cos = -0.99 at 3.0001 rad), and pi itself
    for th in (0.0, 1e-12, 9e-9, 1.1e-8, 1e-5, 0.04, 0.06, 1.0, 2.9, 3.0, 3.0003, 3.1, np.pi - 1e-6, np.pi - 1e-10):
        xi = np.concatenate([th * axes, rng.standard_normal((40, 3))], 1)
        T = R.exp(xi)
        back = R.log(T)
        # Log is evaluated from R, whose entries carry eps: the angle comes back to eps / sin-or-sqrt conditioning, 1e-7 at pi
        tol = 1e-12 if th < 3.0 else 2e-7
        assert np.abs(back - xi).max() <= tol, (th, np.abs(back - xi).max())
        assert np.abs(R.exp(back) - T).max() <= 1e-12, th
    # at pi exactly the axis sign is free: exp(Log(T)) = T still holds
    T = R.exp(np.concatenate([np.pi * axes, np.zeros((40, 3))], 1))
    assert np.abs(R.exp(R.log(T)) - T).max() <= 1e-12


@pytest.mark.parametrize("name", ["triangle", "near_pi", "tiny", "wide_information"])
def test_analytic_jacobians_equal_central_differences(name):
    """J_s and J_t = -J_s against central differences of the restatement's own residual under T := exp(d) T.  h = 1e-5: truncation
    h^2 / 6 |r'''| (|r'''| is a few times (1 + |t|)^3 <= 1e2) is below 2e-9, rounding eps |r| / h below 1e-10 - bound 1e-8 times
    max(1, |J|)."""
    c = CASES[name]
    poses, nodes, Z = c["poses"], c["nodes"], c["Z"]
    lin = R.linearise(poses, nodes, Z, c["info"], c["uncertain"], 1.0)
    if name == "near_pi":
        th = np.linalg.norm(lin["r"][:, :3], axis=1)
        assert th.max() > 3.0003  # the near-pi branch of Log is the one differentiated
    if name == "tiny":
        assert np.linalg.norm(lin["r"][:, :3], axis=1).max() < 1e-8
    h = 1e-5
    for e, (s, t) in enumerate(nodes):
        for node, sign in ((s, 1.0), (t, -1.0)):
            J = np.zeros((6, 6))
            for a in range(6):
                d = np.zeros(6)
                d[a] = h
                hi, lo = poses.copy(), poses.copy()
                hi[node] = R.exp(d) @ poses[node]
                lo[node] = R.exp(-d) @ poses[node]
                J[:, a] = (R.residual(hi, nodes[e:e + 1], Z[e:e + 1])[0] - R.residual(lo, nodes[e:e + 1], Z[e:e + 1])[0]) / (2 * h)
            want = sign * lin["J"][e]
            assert np.abs(J - want).max() <= 1e-8 * max(1.0, np.abs(want).max()), (name, e, node, np.abs(J - want).max())


def test_triangle_residual_is_the_planted_xi():
    """With the nodes at the truth the inconsistent loop edge's residual is Log(inv(exp(xi))): the planted xi, negated in omega and
    moved through the rotation in t - checked through exp."""
    c = CASES["triangle"]
    r = R.residual(c["truth"], c["nodes"], c["Z"])
    assert np.abs(r[:2]).max() <= 1e-14
    assert np.abs(R.exp(r[2]) @ R.exp(C.TRIANGLE_XI) - np.eye(4)).max() <= 1e-14


@pytest.mark.parametrize("name", sorted(CASES))
def test_pcg_and_dense_solver_reach_the_same_optimum(solved, name):
    c = CASES[name]
    a, b = solved[name], run(c, R.solve_dense)
    assert a["success"] and b["success"], (a["converged"], b["converged"])
    d = R.log(R.inv(b["poses"]) @ a["poses"])
    assert np.linalg.norm(d) <= optimum_bound(c, a, b), (np.linalg.norm(d), optimum_bound(c, a, b))


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["exact"]))
def test_exact_edges_recover_the_truth(solved, name):
    c = CASES[name]
    out = solved[name]
    assert out["success"]
    fixed = c["params"]["fixed"]
    assert np.array_equal(out["poses"][fixed], c["poses"][fixed])
    assert C.aligned_error(out["poses"], c["truth"], fixed) <= optimum_bound(c, out)
    assert out["kept"].all()


def test_false_chord_is_switched_off_and_the_true_ones_kept(solved):
    out = solved["false_chord"]
    unc = CASES["false_chord"]["uncertain"].astype(bool)
    assert out["l"][-1] < 0.25 and not out["kept"][-1]
    assert (out["l"][unc][:-1] >= 0.25).all() and out["kept"][:-1].all()
    assert (out["l"][~unc] == 1.0).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_decision_sits_near_rounding(solved, name):
    """Every outer iteration that takes an accept / reject decision has |rho| > 1e-3, so the GPU cannot flip one by rounding."""
    rows = [r for r in solved[name]["trace"] if r["converged"] not in (R.GRADIENT, R.RESIDUAL)]
    assert all(abs(r["rho"]) > 1e-3 for r in rows), [r["rho"] for r in rows]
    assert len(solved[name]["trace"]) < 100
