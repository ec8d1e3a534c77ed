"""Ray casting on its own: kernel and wall time of ScalableTSDFVolume.ray_cast on the volume ten 32-frame batches of the synthetic
640x480 / 5 mm stream build (~24 k units), and how close the rendered depth comes to the input depth at input keyframe poses.

Prints one JSON line:
  kernel_ms         mean device time of one 640x480 cast (profile_enable / profile_read brackets), all attributes
  wall_ms_host      mean wall time of a cast into host arrays (kernel + device-to-host copies)
  wall_ms_device    mean wall time of a cast into torch CUDA tensors, ended by a synchronise
  rays_per_s        pixels / kernel time
  hit_frac          mean fraction of pixels that hit a surface over the timed casts
  depth_err_*_m     median / p95 |rendered - input depth| at 8 input keyframe poses, pixels valid in both
The kernel is a latency-bound gather (hash probes and voxel reads along each ray); its time is not a fraction of any roofline.
Do NOT run under rocprofv3 on a box without cached frames: the frame generator's worker processes inherit the profiler."""
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

N_FRAMES, BATCH, CASTS, WARMUP, QUALITY_POSES = 320, 32, 50, 5, 8
DEPTH_MIN, DEPTH_MAX, WEIGHT_THRESHOLD = 0.1, bench.DEPTH_TRUNC, 3.0


def main():
    assert torch.cuda.is_available(), "bench_raycast needs a GPU"
    s, depth, rgb, T = bench.load_frames("synthetic_640x480_5mm", N_FRAMES)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    dd, rr = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
    vol = ScalableTSDFVolume(bench.VOXEL, bench.SDF_TRUNC, max_blocks=1 << 17)
    for k in range(N_FRAMES // BATCH):
        sl = slice(BATCH * k, BATCH * k + BATCH)
        vol.integrate_batch(dd[sl], rr[sl], K, T[sl], depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)
    vol.synchronize()
    units = vol.num_blocks()
    poses = [T[(i * 6) % N_FRAMES] for i in range(CASTS)]

    def cast(i, device):
        return vol.ray_cast(K, poses[i % CASTS], DEPTH_MIN, DEPTH_MAX, WEIGHT_THRESHOLD, device=device)

    for i in range(WARMUP):
        cast(i, False)
        cast(i, True)
    torch.cuda.synchronize()

    vol.profile_enable(True)
    hits = []
    for i in range(CASTS):
        out = cast(i, True)
        hits.append(out["mask"].float().mean().item())
    kernel_ms_total, launches, _ = vol.profile_read()
    vol.profile_enable(False)

    t0 = time.perf_counter()
    for i in range(CASTS):
        cast(i, False)
    wall_host = (time.perf_counter() - t0) * 1e3 / CASTS
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(CASTS):
        cast(i, True)
    torch.cuda.synchronize()
    wall_dev = (time.perf_counter() - t0) * 1e3 / CASTS

    errs = []
    for j in range(QUALITY_POSES):
        f = (j * N_FRAMES) // QUALITY_POSES
        out = vol.ray_cast(K, T[f], DEPTH_MIN, DEPTH_MAX, WEIGHT_THRESHOLD, render_attributes=("depth", "mask"))
        ok = out["mask"] & (depth[f] > 0) & (depth[f] < bench.DEPTH_TRUNC)
        errs.append(np.abs(out["depth"][ok] - depth[f][ok]))
    errs = np.concatenate(errs)
    kernel_ms = kernel_ms_total / max(launches, 1)
    print(json.dumps({
        "tool": "bench_raycast", "width": s.width, "height": s.height, "voxel": bench.VOXEL, "units": units, "casts": CASTS,
        "launches": launches, "kernel_ms": round(kernel_ms, 4), "wall_ms_host": round(wall_host, 3), "wall_ms_device": round(wall_dev, 3),
        "rays_per_s": round(s.width * s.height / (kernel_ms * 1e-3), 1), "hit_frac": round(float(np.mean(hits)), 4),
        "depth_err_median_m": round(float(np.median(errs)), 6), "depth_err_p95_m": round(float(np.percentile(errs, 95)), 6),
        "quality_pixels": int(errs.size),
    }))


if __name__ == "__main__":
    main()
