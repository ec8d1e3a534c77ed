"""GPU: KeyframeGraphRgbd.close_loops_by_appearance on the noisy 160x120 room.  Seven keyframes - four at the start of the orbit,
three from its end (tests/orb_cases.LOOP_FRAMES) - so that the odometry across the jump leaves the later nodes far from the truth:
the pose gate of close_loops cannot pair them with the first nodes, the appearance chain does, and every edge it adds is held to
the ground truth within twice what the numpy restatements of the same chain measured (orb_cases.LOOP_WORST_*)."""
import numpy as np
import pytest

from tests import odometry_reference as orf
from tests import orb_cases as oc

pytestmark = pytest.mark.gpu


def test_appearance_closes_the_loop_the_pose_gate_cannot():
    from pyslam_amd.pose_graph import KeyframeGraphRgbd
    from pyslam_amd.volumetric import ScalableTSDFVolume

    K, frames, cam = oc.loop_frames()
    truth = np.array([np.linalg.inv(f[2]) for f in frames])  # T_wc
    vol = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)
    try:
        kg = KeyframeGraphRgbd(vol, cam, method="hybrid", T_wc0=truth[0], features=oc.LOOP_FEATURES, **oc.LOOP_ODOMETRY)
        for depth, rgb, _ in frames:
            kg.add_frame(rgb, depth)
        n = len(frames)
        assert len(kg.features) == n and len(kg.graph.edges) == n - 1
        late, early = (4, 5, 6), (0, 1)
        # the jump from frame 18 to frame 570 leaves the late nodes far from the truth ...
        poses = kg.graph.poses
        off = [orf.pose_error(poses[j], truth[j]) for j in late]
        print("\nlate nodes off the truth by", ", ".join("%.2f m / %.1f deg" % e for e in off))
        assert min(e[0] for e in off) > 0.3  # further than the max_distance of close_loops (0.3 m by default)
        # ... so the pose gate pairs no late node with an early one correctly
        for e in kg.close_loops(min_gap=oc.LOOP_PARAMS["min_gap"]):
            j, i = kg.graph.edges[e]
            if j in late and i in early:
                err = orf.pose_error(kg.graph.transformations[e], np.linalg.inv(truth[i]) @ truth[j])
                assert err[0] > oc.LOOP_TOLERANCE_FACTOR * oc.LOOP_WORST_TRANSLATION_M, (j, i, err)
        kg = KeyframeGraphRgbd(vol, cam, method="hybrid", T_wc0=truth[0], features=oc.LOOP_FEATURES, **oc.LOOP_ODOMETRY)
        for depth, rgb, _ in frames:
            kg.add_frame(rgb, depth)
        before = len(kg.graph.edges)
        added = kg.close_loops_by_appearance(**oc.LOOP_PARAMS)
        edges, uncertain, T = kg.graph.edges, kg.graph.uncertain, kg.graph.transformations
        assert added == list(range(before, len(edges))) and uncertain[added].all() and not uncertain[:before].any()
        pairs = [tuple(int(v) for v in edges[e]) for e in added]
        assert any(j in late and i in early for j, i in pairs), pairs
        # no edge whose RANSAC stage the restatement chain would not also accept
        accepted = {(r["j"], r["i"]) for r in oc.restated_loops(K, frames) if r["accepted"]}
        assert set(pairs) <= accepted, (pairs, accepted)
        assert [(r[0], r[1]) for r in kg.appearance_log if r[5] is not None] == pairs
        # every added edge against the ground truth
        for e, (j, i) in zip(added, pairs):
            t_err, r_err = orf.pose_error(T[e], np.linalg.inv(truth[i]) @ truth[j])
            print("edge (%d, %d): off the truth by %.4f m, %.3f deg" % (j, i, t_err, r_err))
            assert t_err <= oc.LOOP_TOLERANCE_FACTOR * oc.LOOP_WORST_TRANSLATION_M, (j, i, t_err)
            assert r_err <= oc.LOOP_TOLERANCE_FACTOR * oc.LOOP_WORST_ROTATION_DEG, (j, i, r_err)
        assert kg.close_loops_by_appearance(**oc.LOOP_PARAMS) == []  # pairs that already share an edge are skipped
    finally:
        vol.close()
