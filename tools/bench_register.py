"""Map-to-map registration on its own: ScalableTSDFVolume.register_volume() between two overlapping halves of the map 512 frames of
the synthetic 640x480 / 5 mm stream build, held in different frames as tools/bench_merge.py holds them: the destination holds
frames 0..319 in the frame p' = X p (X: 23 deg about (0.3, 1, 0.2), translation (0.31, -0.12, 0.23) m), the source frames 192..511
in the stream's own frame, so the true T_dst_src is X.  The initial guess is X with an error of one voxel and 0.5 deg about the
centre of the source's units.  Timed with HIP events on the destination's stream around the call and with the host clock (the call
waits for the GPU), after a warm-up call; for scale, integrate_volume of the same pair with the refined transform into a twin of
the destination.  Reported, not asserted.

Prints one JSON line:
  source_units, destination_units
  candidates, inliers, fitness, inlier_rmse_mm, success, iterations
  ms, wall_ms            one call, all iterations (median of 5)
  ms_per_iteration       ms / iterations (the collect pass included)
  one_iteration_ms       a call capped at one iteration (collect + one linearise + one solve), median of 5
  init_error_mm / _deg, error_mm / _deg      pose error before and after, the translation taken at the centre of the source's units
  merge_ms               integrate_volume(source, refined transform) into a twin of the destination"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pyslam_amd.volumetric import PinholeCameraIntrinsic, ScalableTSDFVolume  # noqa: E402
from tools.bench_merge import generic_transform  # noqa: E402

N_MAP, BATCH = 512, 64
DST_FRAMES, SRC_FRAMES = (0, 320), (192, 512)


def rodrigues(axis, degrees, translation):
    k = np.asarray(axis, np.float64)
    k /= np.linalg.norm(k)
    a = np.radians(degrees)
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * Kx + (1.0 - np.cos(a)) * (Kx @ Kx)
    T[:3, 3] = translation
    return T


def pose_error(T, T_ref, centre):
    D = np.linalg.inv(T_ref) @ T
    cos = np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(D[:3, :3] @ centre + D[:3, 3] - centre)), float(np.degrees(np.arccos(cos)))


def main():
    assert torch.cuda.is_available(), "bench_register needs a GPU"
    s, depth, rgb, T = bench.load_frames("synthetic_640x480_5mm", N_MAP)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    dd, rr = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
    T = np.ascontiguousarray(T, dtype=np.float64)
    X = generic_transform()
    T_moved = np.ascontiguousarray(T @ np.linalg.inv(X))
    stream = torch.cuda.Stream()

    def fused(poses, lo, hi):
        vol = ScalableTSDFVolume(bench.VOXEL, bench.SDF_TRUNC, max_blocks=1 << 17)
        vol.set_stream(stream.cuda_stream)
        for k in range(lo // BATCH, hi // BATCH):
            sl = slice(BATCH * k, BATCH * k + BATCH)
            vol.integrate_batch(dd[sl], rr[sl], K, poses[sl], depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)
        vol.synchronize()
        return vol

    def timed(vol, fn):
        vol.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out

    dst, src = fused(T_moved, *DST_FRAMES), fused(T, *SRC_FRAMES)
    keys = src.unit_keys().astype(np.int64)
    centre = (keys.min(0) + keys.max(0) + 1) * 0.5 * 16 * bench.VOXEL
    wrong = rodrigues((-0.4, 0.5, 1.0), 0.5, np.array([1.0, -0.7, 0.5]) / np.linalg.norm([1.0, -0.7, 0.5]) * bench.VOXEL)
    wrong[:3, 3] += centre - wrong[:3, :3] @ centre  # about the centre
    init = X @ wrong

    dst.register_volume(src, init)  # warm-up: code objects loaded, allocator primed
    runs = [timed(dst, lambda: dst.register_volume(src, init)) for _ in range(5)]
    ones = [timed(dst, lambda: dst.register_volume(src, init, max_iterations=1)) for _ in range(5)]
    ms, wall = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
    res = runs[-1][2]
    e0, e1 = pose_error(init, X, centre), pose_error(res.transformation, X, centre)

    twin = fused(T_moved, *DST_FRAMES)
    warm = fused(T_moved, *DST_FRAMES)
    warm.integrate_volume(src, res.transformation)
    merge_ms, _, st = timed(twin, lambda: twin.integrate_volume(src, res.transformation))

    print(json.dumps({"tool": "bench_register", "width": s.width, "height": s.height, "voxel": bench.VOXEL, "map_frames": N_MAP,
                      "source_units": src.num_blocks(), "destination_units": dst.num_blocks(), "candidates": res.candidates, "inliers": res.inliers,
                      "fitness": round(res.fitness, 4), "inlier_rmse_mm": round(res.inlier_rmse * 1e3, 4), "success": res.success,
                      "iterations": res.iterations, "ms": round(ms, 3), "wall_ms": round(wall, 3),
                      "ms_per_iteration": round(ms / max(res.iterations, 1), 3), "one_iteration_ms": round(float(np.median([r[0] for r in ones])), 3),
                      "init_error_mm": round(e0[0] * 1e3, 4), "init_error_deg": round(e0[1], 5), "error_mm": round(e1[0] * 1e3, 4),
                      "error_deg": round(e1[1], 5), "merge_ms": round(merge_ms, 3), "merge_voxels_updated": st.voxels_updated}))


if __name__ == "__main__":
    main()
