"""The plane-sweep matcher on its own: _Volume.multiview_sgm at 752x480 (euroc_752x480_10mm), D = 128, for N = 1, 2 and 4 source
views and paths 8 and 4, on synthetic keyframes (a reference pose with earlier poses as sources), beside _Volume.stereo_sgm at the
same shape in the same run.  Reported, not asserted.

Prints one JSON line; "stereo" per paths variant and "mvs" per (N, paths) variant:
  stages_ms        kernel time of the call's brackets (medians over REPEATS calls after WARMUP): stereo [census, paths, winner,
                   finish], mvs [census, cost, paths, winner, finish]
  kernel_ms        their sum;  kernel_ms_spread: [min, max]
  device_wall_ms   wall time of one call on device tensors into device tensors, ended by a synchronise
  valid_share      share of pixels with a result
and per mvs variant paths_vs_stereo / winner_vs_stereo: the stage's kernel time over stereo_sgm's at the same number of paths.

--cache FILE.npz: keep the rendered images there (rendering is host-side numpy, about 0.5 s per image)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyslam_amd.prep import plane_sweep_views  # noqa: E402
from pyslam_amd.synthetic import SyntheticRGBD  # noqa: E402
from pyslam_amd.volumetric import ScalableTSDFVolume  # noqa: E402

CONFIG, BASELINE, D = "euroc_752x480_10mm", 0.11, 128
REF_POSE, POSE_STEP, MAX_SOURCES, MIN_DEPTH = 150, 5, 4, 0.8
REPEATS, WARMUP = 15, 3


def keyframes(s, cache):
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return z["rgb"], z["T"], z["right"]
    frames = [s[REF_POSE - POSE_STEP * k] for k in range(MAX_SOURCES + 1)]
    rgb, T = np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames])
    right = s.stereo(REF_POSE, BASELINE)[1]
    if cache:
        np.savez(cache, rgb=rgb, T=T, right=right)
    return rgb, T, right


def timed_calls(vol, call):
    """WARMUP + REPEATS calls, each between two synchronisations -> ([REPEATS, brackets] kernel ms, [REPEATS] wall ms, last result)"""
    stages, walls, result = [], [], None
    for rep in range(WARMUP + REPEATS):
        vol.synchronize()
        torch.cuda.synchronize()
        vol.profile_enable(True)
        t0 = time.perf_counter()
        result = call()
        vol.synchronize()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        per_stage = [float(x) for x in vol.profile_launches()]
        vol.profile_read()
        vol.profile_enable(False)
        if rep >= WARMUP:
            stages.append(per_stage)
            walls.append(wall)
    return np.asarray(stages, np.float64), walls, result


def summary(stages, walls, valid):
    total = stages.sum(axis=1)
    return {"stages_ms": [round(float(x), 3) for x in np.median(stages, axis=0)], "kernel_ms": round(float(np.median(total)), 3),
            "kernel_ms_spread": [round(float(total.min()), 3), round(float(total.max()), 3)],
            "device_wall_ms": round(float(np.median(walls)), 3), "valid_share": round(float(valid), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mvs needs a GPU"
    s = SyntheticRGBD(CONFIG, noise=False, invalid_frac=0.0)
    rgb, T, right = keyframes(s, args.cache)
    vol = ScalableTSDFVolume(s.voxel, 0.04, max_blocks=1 << 10)
    d_rgb, d_right = torch.from_numpy(rgb).cuda(), torch.from_numpy(right).cuda()
    views = plane_sweep_views(s.intrinsics, T[0], s.intrinsics, T[1:])
    out = {"metric": "mvs_sgm", "config": CONFIG, "height": s.height, "width": s.width, "num_planes": D, "min_depth": MIN_DEPTH,
           "pose_step": POSE_STEP, "repeats": REPEATS, "warmup": WARMUP, "stereo": {}, "mvs": {}}
    for paths in (8, 4):
        st, walls, (disp, _) = timed_calls(vol, lambda: vol.stereo_sgm(d_rgb[0], d_right, num_disparities=D, paths=paths, bf=float(s.fx * BASELINE)))
        out["stereo"][f"paths{paths}"] = summary(st, walls, (disp >= 0).float().mean().item())
        base = np.median(st, axis=0)
        for N in (1, 2, 4):
            st, walls, (index, _) = timed_calls(vol, lambda: vol.multiview_sgm(d_rgb[0], d_rgb[1:1 + N], views[:N], min_depth=MIN_DEPTH, num_planes=D,
                                                                                 paths=paths))
            row = summary(st, walls, (index >= 0).float().mean().item())
            med = np.median(st, axis=0)
            row["scratch_bytes"] = s.height * s.width * (3 * D + 8 * (1 + N) + 2)
            row["paths_vs_stereo"], row["winner_vs_stereo"] = round(float(med[2] / base[1]), 3), round(float(med[3] / base[2]), 3)
            out["mvs"][f"n{N}_paths{paths}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
