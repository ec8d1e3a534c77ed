"""Pose-graph optimisation on its own: _Volume.optimize_pose_graph on rings with chords at N = 256, 2 048 and 16 384 nodes, E = 3 N
(the ring and chords to the 7th and 31st node on), poses perturbed, edges exact, default parameters (100 CG iterations at the most
per outer iteration), at most MAX_ITERATIONS outer iterations.  Beside it, in the same run, the numpy restatement's own host solve
(tests/pose_graph_reference.py) of ONE outer iteration from the same start: its PCG, and its dense solve where the matrix fits
(N <= 2 048).  Reported, not asserted.

Prints one JSON line; per N:
  iterations, converged, cg_iterations_total, chi2_initial, chi2_final      of the GPU call
  kernel_ms_per_iteration   the call's brackets (one per outer iteration: 7 + 4 cg_max_iterations launches), median over the
                            iterations of REPEATS calls after WARMUP
  wall_ms_per_iteration     wall time of the call on device tensors over its outer iterations (median over the calls)
  launches_per_iteration    7 + 4 cg_max_iterations
  host_pcg_ms, host_dense_ms   one outer iteration of the restatement with either inner solver (dense: null beyond 2 048 nodes)
  host_pcg_over_gpu_wall, host_dense_over_gpu_wall   the ratios"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyslam_amd.volumetric import ScalableTSDFVolume  # noqa: E402
from tests import pose_graph_cases as C  # noqa: E402
from tests import pose_graph_reference as R  # noqa: E402

SIZES = (256, 2048, 16384)
CHORDS = (7, 31)
WARMUP, REPEATS = 1, 5
MAX_ITERATIONS = 10
DENSE_LIMIT = 2048


def graph(n, seed=0):
    truth = C.trajectory(n, seed)
    edges = np.array([(i, (i + k) % n) for k in (1,) + CHORDS for i in range(n)], np.int32)
    Z = R.inv(truth[edges[:, 1]]) @ truth[edges[:, 0]]
    info = np.tile(100.0 * np.eye(6), (len(edges), 1, 1))
    return C.perturbed(truth, seed + 1, 0), edges, np.ascontiguousarray(Z), info


def main():
    assert torch.cuda.is_available(), "bench_pose_graph needs a GPU"
    vol = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)
    out = {"metric": "pose_graph", "repeats": REPEATS, "warmup": WARMUP, "max_iterations": MAX_ITERATIONS, "sizes": {}}
    for n in SIZES:
        poses, edges, Z, info = graph(n)
        dev = [torch.from_numpy(a).cuda() for a in (poses, edges, Z, info)]
        kernel, wall, res = [], [], None
        for rep in range(WARMUP + REPEATS):
            vol.synchronize()
            vol.profile_enable(True)
            vol.profile_read()
            t0 = time.perf_counter()
            res = vol.optimize_pose_graph(*dev, max_iterations=MAX_ITERATIONS)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ms = vol.profile_launches()
            vol.profile_enable(False)
            if rep >= WARMUP:
                kernel += [float(x) for x in ms[:res.iterations]]  # the last bracket is the final weights' launch
                wall.append((t1 - t0) * 1e3 / res.iterations)
        t0 = time.perf_counter()
        R.step(poses, edges, Z, info, None, 0.0, 2.0, True, {})
        pcg_ms = (time.perf_counter() - t0) * 1e3
        dense_ms = None
        if n <= DENSE_LIMIT:
            t0 = time.perf_counter()
            R.step(poses, edges, Z, info, None, 0.0, 2.0, True, {}, solver=R.solve_dense)
            dense_ms = (time.perf_counter() - t0) * 1e3
        w = float(np.median(wall))
        out["sizes"][str(n)] = {
            "edges": len(edges), "iterations": res.iterations, "converged": res.converged, "cg_iterations_total": res.cg_iterations_total,
            "chi2_initial": res.chi2_initial, "chi2_final": res.chi2_final, "kernel_ms_per_iteration": round(float(np.median(kernel)), 3),
            "wall_ms_per_iteration": round(w, 3), "launches_per_iteration": 7 + 4 * 100, "host_pcg_ms": round(pcg_ms, 1),
            "host_dense_ms": None if dense_ms is None else round(dense_ms, 1), "host_pcg_over_gpu_wall": round(pcg_ms / w, 2),
            "host_dense_over_gpu_wall": None if dense_ms is None else round(dense_ms / w, 2)}
    vol.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
