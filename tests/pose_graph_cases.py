"""Planted pose graphs for the pose-graph tests, all built from a seeded ground-truth trajectory.  A case is a dict: name, poses
[N,4,4] (the start), nodes [E,2] int32, Z [E,4,4], info [E,6,6], uncertain [E] uint8 or None, truth [N,4,4] or None, exact (every
edge agrees with truth), params (what the call and the restatement both take)."""
import numpy as np

from tests import pose_graph_reference as R


def trajectory(n, seed, radius=2.0):
    """n camera-to-world poses around a circle with seeded jitter in position and attitude."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        a = 2 * np.pi * i / max(n, 3)
        xi = np.concatenate([[0.0, a, 0.0] + 0.1 * rng.standard_normal(3), [radius * np.cos(a), 0.3 * rng.standard_normal(), radius * np.sin(a)]])
        out.append(R.exp(xi))
    return np.array(out)


def relative(truth, s, t):
    """Z = T_target_source of two world poses."""
    return R.inv(truth[t]) @ truth[s]


def perturbed(truth, seed, fixed, rot=0.02, trans=0.05):
    rng = np.random.default_rng(seed)
    xi = np.concatenate([rot * rng.standard_normal((len(truth), 3)), trans * rng.standard_normal((len(truth), 3))], 1)
    xi[fixed] = 0
    return R.exp(xi) @ truth


def spd(rng, w_scale, t_scale):
    """A symmetric (bitwise) positive definite 6 x 6 whose omega block is w_scale and t block t_scale in size."""
    B = rng.standard_normal((6, 12))
    S = np.diag(np.sqrt([w_scale] * 3 + [t_scale] * 3))
    A = S @ (B @ B.T / 12 + np.eye(6)) @ S
    return (A + A.T) / 2


EXACT = dict(residual_tolerance=1e-16, cg_max_iterations=300, cg_tolerance=1e-10)


def _case(name, truth, start, edges, info, uncertain=None, fixed=0, exact=True, Z=None, **params):
    nodes = np.array(edges, np.int32).reshape(-1, 2)
    Zs = np.array([relative(truth, s, t) for s, t in nodes]) if Z is None else Z
    if np.ndim(info) == 0:
        info = np.tile(float(info) * np.eye(6), (len(nodes), 1, 1))
    return dict(name=name, poses=np.ascontiguousarray(start), nodes=nodes, Z=np.ascontiguousarray(Zs), info=np.ascontiguousarray(info),
                uncertain=None if uncertain is None else np.asarray(uncertain, np.uint8), truth=truth, exact=exact,
                params={**EXACT, "fixed": fixed, **params})


def ring(n, seed, fixed=0, name=None):
    truth = trajectory(n, seed)
    edges = [(i, (i + 1) % n) for i in range(n)]
    return _case(name or f"ring{n}", truth, perturbed(truth, seed + 1, fixed), edges, 100.0, fixed=fixed)


def two_nodes():
    truth = trajectory(2, 11)
    return _case("two_nodes", truth, perturbed(truth, 12, 0, 0.1, 0.2), [(0, 1)], 100.0)


TRIANGLE_XI = np.array([0.03, -0.02, 0.04, 0.05, -0.04, 0.02])


def triangle():
    """Two exact edges and a loop edge that is inconsistent by the known TRIANGLE_XI (a left perturbation of Z)."""
    truth = trajectory(3, 21)
    c = _case("triangle", truth, perturbed(truth, 22, 0), [(0, 1), (1, 2), (2, 0)], 100.0, exact=False)
    c["Z"][2] = R.exp(TRIANGLE_XI) @ c["Z"][2]
    return c


def star():
    """A hub of degree 70: its incidence list is longer than a wave.  Half of the edges point at the hub, half away from it."""
    truth = trajectory(71, 31)
    edges = [(0, i) if i % 2 else (i, 0) for i in range(1, 71)]
    return _case("star70", truth, perturbed(truth, 32, 0), edges, 100.0)


def duplicates():
    truth = trajectory(12, 41)
    edges = [(i, (i + 1) % 12) for i in range(12)] + [(3, 2), (7, 6), (0, 1), (0, 1), (11, 4), (9, 2), (9, 2)]
    return _case("duplicates", truth, perturbed(truth, 42, 0), edges, 100.0)


def false_chord(with_chord=True):
    """A 65-ring (certain), six true uncertain chords and one planted false one, 0.5 m off."""
    truth = trajectory(65, 51)
    ring_edges = [(i, (i + 1) % 65) for i in range(65)]
    chords = [(0, 30), (5, 40), (12, 50), (20, 60), (33, 3), (45, 10)]
    edges = ring_edges + chords + ([(8, 37)] if with_chord else [])
    unc = [0] * 65 + [1] * (len(edges) - 65)
    c = _case("false_chord" if with_chord else "no_chord", truth, perturbed(truth, 52, 0), edges, 100.0, uncertain=unc, exact=not with_chord)
    if with_chord:
        off = np.eye(4)
        off[:3, 3] = (0.3, 0.0, 0.4)
        c["Z"][-1] = off @ c["Z"][-1]
    return c


def near_pi():
    """A chain whose last node starts 3.1 rad off: X of the last edge has a rotation beyond the near-pi threshold (3.0003 rad)."""
    truth = trajectory(3, 61)
    start = truth.copy()
    start[2] = R.exp(np.array([3.1 / np.sqrt(3)] * 3 + [0.1, -0.2, 0.1])) @ truth[2]
    return _case("near_pi", truth, start, [(0, 1), (1, 2)], 100.0)


def tiny():
    """Residuals below the small-angle threshold of Log (|omega| ~ 1e-10)."""
    truth = trajectory(4, 71)
    return _case("tiny", truth, perturbed(truth, 72, 0, 1e-10, 1e-10), [(0, 1), (1, 2), (2, 3), (3, 0)], 100.0, residual_tolerance=0.0,
                 gradient_tolerance=1e-12)


def wide_information():
    """Information matrices whose omega and t blocks are six orders of magnitude apart, as the odometry's are."""
    truth = trajectory(9, 81)
    edges = [(i, (i + 1) % 9) for i in range(9)] + [(0, 4), (6, 2)]
    rng = np.random.default_rng(83)
    info = np.array([spd(rng, 1e6 * (1 + i), 1.0 + 0.1 * i) for i in range(len(edges))])
    return _case("wide_information", truth, perturbed(truth, 82, 0, 0.005, 0.05), edges, info)


def all_cases():
    return [two_nodes(), triangle(), ring(64, 101), ring(65, 103), ring(256, 105), ring(257, 107), star(), duplicates(),
            ring(10, 111, fixed=3, name="fixed3"), ring(9, 113, fixed=8, name="fixed_last"), false_chord(), false_chord(False), near_pi(),
            tiny(), wide_information()]


def aligned_error(poses, truth, fixed):
    """The largest |Log(inv(truth_i) G pose_i)| over the nodes with G = truth_fixed inv(pose_fixed): poses against the truth, aligned at
    the fixed node (rotation in radians and translation in metres, one number)."""
    G = truth[fixed] @ R.inv(poses[fixed])
    return float(np.abs(R.log(R.inv(truth) @ (G @ poses))).max())
