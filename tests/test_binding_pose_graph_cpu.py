"""What optimize_pose_graph and pose_graph_linearise send over the C ABI, pinned against the recording stand-in for the library
(tests/recording_lib.py; no GPU), in the manner of tests/test_binding_odometry_cpu.py; and the bookkeeping of PoseGraph and
KeyframeGraphRgbd on a stub volume with a fake rgbd_odometry."""
import types

import numpy as np
import pytest

from pyslam_amd import _lib as L
from pyslam_amd import volumetric as V
from pyslam_amd import volumetric_semantic as S
from pyslam_amd.pose_graph import KeyframeGraphRgbd, PoseGraph
from tests.recording_lib import ref, volume
from tests.test_binding_calls_cpu import ANY, SKIP, P, REF, covers, expect, host, refused, shaped, tsdf  # noqa: F401 (host: a fixture)

I64 = L.ctypes.c_int64
FIELDS = ("line_process_weight", "edge_prune_threshold", "lambda_scale", "gradient_tolerance", "step_tolerance", "decrease_tolerance",
          "residual_tolerance", "cg_tolerance", "max_iterations", "cg_max_iterations", "fixed", "trace_state")


def graph(n=4, seed=0):
    rng = np.random.default_rng(seed)
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, :3, 3] = rng.random((n, 3))
    edges = np.array([(i, i + 1) for i in range(n - 1)] + [(n - 1, 0)], np.int32)
    Z = np.tile(np.eye(4), (len(edges), 1, 1))
    Z[:, :3, 3] = rng.random((len(edges), 3))
    info = np.tile(np.eye(6), (len(edges), 1, 1)) * 7.0
    unc = np.array([False] * (n - 1) + [True])
    return poses, edges, Z, info, unc


def params(call, index):
    p = ref(call[1][index])
    return {f: getattr(p, f) for f in FIELDS}


def test_structs_mirror_the_header():
    assert [n for n, _ in L.HvPoseGraphParams._fields_] == list(FIELDS)
    assert L.ctypes.sizeof(L.HvPoseGraphParams) == 8 * 8 + 4 * 4
    assert [n for n, _ in L.HvPoseGraphResult._fields_] == ["chi2_initial", "chi2_final", "lambda_", "iterations", "cg_iterations_total",
                                                          "edges_kept", "converged", "success"]
    assert L.ctypes.sizeof(L.HvPoseGraphResult) == 3 * 8 + 5 * 4 + 4
    assert L.HV_POSE_GRAPH_TRACE_STRIDE == 12 and len(V._POSE_GRAPH_TRACE) == 12
    text = open(L.os.path.join(L.os.path.dirname(L.os.path.dirname(L.__file__)), "include", "hipvol.h")).read()
    assert "#define HV_POSE_GRAPH_TRACE_STRIDE 12" in text


@covers("optimize_pose_graph")
def test_defaults_on_every_kind_of_volume(host):
    poses, edges, Z, info, unc = graph()
    before = poses.copy()
    for vol in (tsdf(), volume(V.VoxelBlockGrid, voxel_size=0.05, block_size=8), volume(S.VoxelBlockSemanticGrid, voxel_size=0.05, block_size=8)):
        vol._lib.script("hv_pose_graph_optimize", peek={1: (np.float64, 64)})
        out = vol.optimize_pose_graph(host(poses), host(edges), host(Z), host(info))
        call, = expect(vol, ("hv_pose_graph_optimize", P(out.poses), 4, P(edges), P(Z), P(info), None, 4, REF(L.HvPoseGraphParams),
                             P(out.line_process), REF(L.HvPoseGraphResult), None, None, 0, REF(I64), L.HV_HOST))
        assert params(call, 8) == dict(line_process_weight=1.0, edge_prune_threshold=0.25, lambda_scale=1e-5, gradient_tolerance=1e-6,
                                       step_tolerance=1e-6, decrease_tolerance=1e-6, residual_tolerance=1e-6, cg_tolerance=1e-8,
                                       max_iterations=100, cg_max_iterations=100, fixed=0, trace_state=0)
        # the in / out buffer is the result's own array, filled with the caller's poses; the caller's array is not written
        np.testing.assert_array_equal(vol._lib.peeked[-1][1], before.ravel())
        assert np.array_equal(poses, before) and out.poses is not poses
        shaped(out.poses, (4, 4, 4), np.float64), shaped(out.line_process, (4,), np.float64), shaped(out.kept, (4,), np.bool_)
        assert isinstance(out, V.PoseGraphResult) and out.trace is None and out.success is False and out.converged == "max_iterations"
        assert out.iterations == 0 and out.edges_kept == 0 and out.chi2_final == 0.0


@covers("optimize_pose_graph")
def test_marshals_every_argument_dtype_and_layout(host):
    poses, edges, Z, info, unc = graph(5)
    vol = tsdf()
    vol._lib.script("hv_pose_graph_optimize", 2, peek={3: (np.int32, 10), 4: (np.float64, 80), 5: (np.float64, 180), 6: (np.uint8, 5)})
    wide = np.zeros((5, 4, 8))
    wide[..., ::2] = Z  # a strided operand is sent contiguous
    out = vol.optimize_pose_graph(host(poses.astype(np.float32)), edges.astype(np.int64).tolist(), wide[..., ::2], host(info.astype(np.float32)),
                                  uncertain=unc.tolist(), fixed=3, line_process_weight=4.0, edge_prune_threshold=0.5, max_iterations=7,
                                  lambda_scale=1e-3, gradient_tolerance=1e-7, step_tolerance=1e-8, decrease_tolerance=1e-9,
                                  residual_tolerance=1e-10, cg_max_iterations=9, cg_tolerance=1e-4, trace=True)
    call, = expect(vol, ("hv_pose_graph_optimize", P(out.poses), 5, ANY, ANY, ANY, ANY, 5, REF(L.HvPoseGraphParams), P(out.line_process),
                         REF(L.HvPoseGraphResult), ANY, ANY, 7, REF(I64), L.HV_HOST))
    assert params(call, 8) == dict(line_process_weight=4.0, edge_prune_threshold=0.5, lambda_scale=1e-3, gradient_tolerance=1e-7,
                                   step_tolerance=1e-8, decrease_tolerance=1e-9, residual_tolerance=1e-10, cg_tolerance=1e-4, max_iterations=7,
                                   cg_max_iterations=9, fixed=3, trace_state=1)
    got = vol._lib.peeked[-1]
    np.testing.assert_array_equal(got[3], edges.ravel())
    np.testing.assert_array_equal(got[4], Z.ravel())
    np.testing.assert_array_equal(got[5], info.ravel())
    np.testing.assert_array_equal(got[6], unc.astype(np.uint8))
    # two rows came back (scripted), each with the start poses of its iteration
    assert len(out.trace) == 2 and set(out.trace[0]) == {n for n, _ in V._POSE_GRAPH_TRACE} | {"poses"} and out.trace[1]["poses"].shape == (5, 4, 4)
    # a single node without edges is a legal graph
    vol = tsdf()
    out = vol.optimize_pose_graph(np.eye(4)[None], np.zeros((0, 2), np.int32), np.zeros((0, 4, 4)), np.zeros((0, 6, 6)))
    expect(vol, ("hv_pose_graph_optimize", P(out.poses), 1, SKIP, SKIP, SKIP, None, 0, REF(L.HvPoseGraphParams), SKIP, REF(L.HvPoseGraphResult), None,
                 None, 0, REF(I64), L.HV_HOST))
    assert out.line_process.shape == (0,) and out.kept.shape == (0,)


@covers("optimize_pose_graph")
def test_refusals_come_before_any_call():
    poses, edges, Z, info, unc = graph()
    vol = tsdf()
    call = vol.optimize_pose_graph
    refused(vol, ValueError, "poses must be [N,4,4] with N >= 1, got (4, 16)", call, poses.reshape(4, 16), edges, Z, info)
    refused(vol, ValueError, "poses must be [N,4,4] with N >= 1, got (0, 4, 4)", call, poses[:0], edges, Z, info)
    refused(vol, ValueError, "transformations must be [4,4,4] for 4 edges, got (3, 4, 4)", call, poses, edges, Z[:3], info)
    refused(vol, ValueError, "informations must be [4,6,6] for 4 edges, got (4, 36)", call, poses, edges, Z, info.reshape(4, 36))
    refused(vol, ValueError, "uncertain must be [4], got (3,)", call, poses, edges, Z, info, uncertain=unc[:3])
    refused(vol, ValueError, "fixed must be a node index in 0..3, got 4", call, poses, edges, Z, info, fixed=4)
    refused(vol, ValueError, "fixed must be a node index in 0..3, got -1", call, poses, edges, Z, info, fixed=-1)
    refused(vol, ValueError, "line_process_weight must be positive and finite", call, poses, edges, Z, info, line_process_weight=0.0)
    refused(vol, ValueError, "edge_prune_threshold must be in 0..1", call, poses, edges, Z, info, edge_prune_threshold=1.5)
    refused(vol, ValueError, "max_iterations and cg_max_iterations must be in 1..10000", call, poses, edges, Z, info, max_iterations=0)
    refused(vol, ValueError, "max_iterations and cg_max_iterations must be in 1..10000", call, poses, edges, Z, info, cg_max_iterations=10001)


@covers("pose_graph_linearise")
def test_linearise_call(host):
    poses, edges, Z, info, unc = graph()
    vol = tsdf()
    out = vol.pose_graph_linearise(host(poses), host(edges), host(Z), host(info), uncertain=host(unc), line_process_weight=2.5)
    expect(vol, ("hv_pose_graph_linearise", P(poses), 4, P(edges), P(Z), P(info), ANY, 4, 2.5, P(out["r"]), P(out["chi2"]), P(out["l"]),
                 P(out["M"]), P(out["g"]), P(out["b"]), L.HV_HOST))
    shaped(out["r"], (4, 6), np.float64), shaped(out["M"], (4, 6, 6), np.float64), shaped(out["b"], (4, 6), np.float64)
    refused(vol, ValueError, "the graph has no edge", vol.pose_graph_linearise, poses, edges[:0], Z[:0], info[:0])


# -- PoseGraph and KeyframeGraphRgbd on a stub ---------------------------------------------------------------------------------

H, W = 6, 20
CAM = types.SimpleNamespace(fx=30.0, fy=31.0, cx=9.5, cy=2.5, width=W, height=H)


class StubVolume:
    """rgbd_odometry and optimize_pose_graph that record their operands and answer with scripted results."""

    def __init__(self, results=()):
        self.calls, self.results, self.optimized = [], list(results), []

    def rgbd_odometry(self, source_depth, target_depth, intrinsic, **kw):
        self.calls.append((source_depth, target_depth, intrinsic, kw))
        return self.results.pop(0)

    def optimize_pose_graph(self, poses, edges, transformations, informations, uncertain, **kw):
        self.optimized.append((poses, edges, transformations, informations, uncertain, kw))
        moved = poses.copy()
        moved[:, 0, 3] += 1.0
        return V.PoseGraphResult(moved, np.ones(len(edges)), np.ones(len(edges), bool), 2.0, 1.0, 0.1, 3, 9, len(edges), "gradient", True, None)


def result(T, success=True, info=None, fitness=0.9):
    return V.OdometryResult(T, fitness, 0.001, np.eye(6) * 50.0 if info is None else info, success, (1, 1, 1), 0, 100, 110)


def step(tx, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, 0, s, tx], [0, 1, 0, 0.0], [-s, 0, c, 0.01], [0, 0, 0, 1.0]])


def test_pose_graph_holds_plain_arrays_and_inverts_for_extrinsics():
    g = PoseGraph()
    T = [step(0.1 * i, 10.0 * i) for i in range(3)]
    assert [g.add_node(t) for t in T] == [0, 1, 2]
    info = np.arange(36.0).reshape(6, 6)
    assert g.add_edge(1, 0, T[1], info) == 0 and g.add_edge(2, 0, T[2], np.eye(6), uncertain=True) == 1
    assert g.poses.shape == (3, 4, 4) and g.edges.dtype == np.int32 and g.edges.tolist() == [[1, 0], [2, 0]]
    assert g.uncertain.tolist() == [False, True] and g.transformations.shape == (2, 4, 4)
    assert np.array_equal(g.informations[0], (info + info.T) / 2) and np.array_equal(g.informations[0], g.informations[0].T)
    ext = g.extrinsics()
    assert ext.shape == (3, 4, 4) and max(np.abs(ext[i] @ T[i] - np.eye(4)).max() for i in range(3)) <= 1e-15
    for bad in ((0, 0), (3, 0), (-1, 1)):
        with pytest.raises(ValueError, match="bad node pair"):
            g.add_edge(*bad, np.eye(4), np.eye(6))
    with pytest.raises(ValueError, match="must be 4x4"):
        g.add_node(np.eye(3))
    vol = StubVolume()
    res = g.optimize(vol, fixed=1, line_process_weight=3.0)
    poses, edges, Z, infos, unc, kw = vol.optimized[0]
    assert kw == dict(fixed=1, line_process_weight=3.0) and unc.tolist() == [False, True] and edges.tolist() == [[1, 0], [2, 0]]
    assert res is g.last_result and np.array_equal(g.poses, res.poses) and g.poses[0, 0, 3] == T[0][0, 3] + 1.0
    empty = PoseGraph()
    assert empty.poses.shape == (0, 4, 4) and empty.edges.shape == (0, 2) and empty.informations.shape == (0, 6, 6)


def test_keyframe_graph_nodes_edges_and_the_lost_frame():
    T1, T3 = step(0.1, 5.0), step(0.3, -3.0)
    info1 = np.diag([1e4, 2e4, 3e4, 10.0, 20.0, 30.0])
    vol = StubVolume([result(T1, info=info1), result(step(9.0, 0.0), success=False), result(T3)])
    T0 = step(1.0, 30.0)
    kg = KeyframeGraphRgbd(vol, CAM, method="hybrid", keep_on_device=False, T_wc0=T0, lost_information=0.5, iterations=(4, 2))
    depth = [np.full((H, W), 1.0 + i, np.float32) for i in range(4)]
    color = [np.full((H, W, 3), i, np.uint8) for i in range(4)]
    assert [kg.add_frame(color[i], depth[i]) for i in range(4)] == [0, 1, 2, 3]
    g = kg.graph
    assert np.array_equal(g.poses[0], T0) and np.array_equal(g.poses[1], T0 @ T1)
    assert np.array_equal(g.poses[2], T0 @ T1) and kg.lost_nodes == [2]  # the lost frame sits at the previous keyframe's pose
    assert np.array_equal(g.poses[3], (T0 @ T1) @ T3) and not kg.lost and kg.frames == 4
    # one certain edge (new, previous) per frame after the first; the lost one carries the identity and the stated low information
    assert g.edges.tolist() == [[1, 0], [2, 1], [3, 2]] and not g.uncertain.any()
    assert np.array_equal(g.transformations[0], T1) and np.array_equal(g.informations[0], info1)
    assert np.array_equal(g.transformations[1], np.eye(4)) and np.array_equal(g.informations[1], 0.5 * np.eye(6))
    # each frame is the SOURCE against the previous keyframe as TARGET from an identity start
    for k, (sd, td, K, kw) in enumerate(vol.calls):
        assert sd is depth[k + 1] and td is depth[k] and kw["source_color"] is color[k + 1] and kw["target_color"] is color[k]
        assert kw["init"] is None and kw["iterations"] == (4, 2) and list(K.as_array()) == [30.0, 31.0, 9.5, 2.5]
    # the keyframes' images stay (host arrays without keep_on_device)
    assert all(kg.keyframes[i][0] is depth[i] and kg.keyframes[i][1] is color[i] for i in range(4))
    ext = kg.extrinsics()
    assert max(np.abs(ext[i] @ g.poses[i] - np.eye(4)).max() for i in range(4)) <= 1e-15
    # keyframe_every = 2 drops every other frame; point_to_plane keeps no colour
    vol = StubVolume([result(T1)])
    kg = KeyframeGraphRgbd(vol, CAM, method="point_to_plane", keyframe_every=2, keep_on_device=False)
    assert [kg.add_frame(None, depth[i]) for i in range(3)] == [0, None, 1] and len(vol.calls) == 1
    assert vol.calls[0][0] is depth[2] and vol.calls[0][1] is depth[0] and vol.calls[0][3]["source_color"] is None
    with pytest.raises(ValueError, match="method must be one of"):
        KeyframeGraphRgbd(vol, CAM, method="icp")
    with pytest.raises(ValueError, match="keyframe_every"):
        KeyframeGraphRgbd(vol, CAM, keyframe_every=0)
    with pytest.raises(ValueError, match="needs the colour image"):
        KeyframeGraphRgbd(vol, CAM, keep_on_device=False).add_frame(None, depth[0])


def test_close_loops_selects_by_distance_angle_and_gap_and_passes_the_estimate():
    """Eight keyframes on a circle that comes back to its start: node 7 ends 0.05 m and 2 degrees from node 0."""
    n = 8
    truth = [np.eye(4)]
    for i in range(1, n):
        a = 2 * np.pi * i / n
        T = step(0.0, np.degrees(a) if i < n - 1 else 2.0)
        T[:3, 3] = (np.sin(a), 0.0, 1.0 - np.cos(a)) if i < n - 1 else (0.05, 0.0, 0.0)
        truth.append(T)
    rel = [np.linalg.inv(truth[i - 1]) @ truth[i] for i in range(1, n)]
    Zloop = step(0.04, 1.5)
    vol = StubVolume([result(r) for r in rel])
    kg = KeyframeGraphRgbd(vol, CAM, method="point_to_plane", keep_on_device=False)
    depth = [np.full((H, W), 1.0 + i, np.float32) for i in range(n)]
    for d in depth:
        kg.add_frame(None, d)
    assert max(np.abs(kg.graph.poses[i] - truth[i]).max() for i in range(n)) <= 1e-12
    # distance: node 1 is 0.77 m from node 0 and from node 2; only (7, 0) is within 0.3 m.  gap: with min_gap 8 nothing is left
    cand = kg.candidates(0.3, 0.5, 2)
    assert [(j, i) for j, i, _ in cand] == [(7, 0)]
    assert kg.candidates(0.3, 0.5, 8) == [] and kg.candidates(0.3, np.radians(1.0), 2) == []  # gap; angle (2 degrees apart)
    assert [(j, i) for j, i, _ in kg.candidates(0.8, 1.0, 1)] == [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (6, 5), (7, 0), (7, 1)]
    del vol.calls[:]
    # a failed alignment adds nothing; a success becomes an uncertain edge (j, i) with the result's transformation and information
    vol.results = [result(Zloop, success=False)]
    assert kg.close_loops(0.3, 0.5, 2) == [] and len(kg.graph.edges) == n - 1
    vol.results = [result(Zloop, info=np.eye(6) * 3.0)]
    assert kg.close_loops(0.3, 0.5, 2) == [n - 1]
    g = kg.graph
    assert g.edges[-1].tolist() == [7, 0] and g.uncertain.tolist() == [False] * (n - 1) + [True]
    assert np.array_equal(g.transformations[-1], Zloop) and np.array_equal(g.informations[-1], np.eye(6) * 3.0)
    for sd, td, K, kw in vol.calls:
        assert sd is depth[7] and td is depth[0]
        assert np.abs(kw["init"] - np.linalg.inv(truth[0]) @ truth[7]).max() <= 1e-12  # T_target_source by the current estimate
    vol.results = [result(Zloop, fitness=0.2)]
    assert kg.close_loops(0.3, 0.5, 2, min_fitness=0.5) == []
    with pytest.raises(ValueError, match="min_gap"):
        kg.close_loops(min_gap=0)
    kg.optimize(fixed=0)
    assert vol.optimized[0][5] == dict(fixed=0) and kg.graph.poses[2, 0, 3] == truth[2][0, 3] + 1.0
