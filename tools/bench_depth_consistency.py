"""The cross-view consistency check on its own: _Volume.filter_depth_consistency at 752x480 (euroc_752x480_10mm) for N = 1, 2 and 4
source views, beside the _Volume.multiview_sgm call that makes the depth it checks, at the same shape in the same run.  The depth maps
are plane-sweep depths of synthetic keyframes: the reference pose and the N poses before it, each matched against its own two
earlier poses.  Reported, not asserted.

Prints one JSON line; per N:
  kernel_ms        kernel time of the call's bracket (median over REPEATS calls after WARMUP);  kernel_ms_spread: [min, max]
  device_wall_ms   wall time of one call on device tensors into device tensors (depth and counts), ended by a synchronise
  kernel_with_stats_ms, device_wall_with_stats_ms   the same with stats=True: the kernel then adds its counts with one atomic per
                   wave, and the call waits for the stream and copies the three counters back
  mvs_kernel_ms    the kernels of multiview_sgm with the same N sources (num_planes = 128, 8 paths), and mvs_device_wall_ms
  share_of_mvs     kernel_ms / mvs_kernel_ms
  bytes_moved      H W (12 + 4 N): the reference depth in, depth and counts out, one gathered float per view
  valid_in, kept   share of pixels with a depth before and after the check;  mean_agree: agreeing views per valid pixel

--cache FILE.npz: keep the rendered images there (rendering is host-side numpy, about 0.5 s per image)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyslam_amd.prep import consistency_views  # noqa: E402
from pyslam_amd.synthetic import SyntheticRGBD  # noqa: E402
from pyslam_amd.volumetric import ScalableTSDFVolume  # noqa: E402
from tools.bench_mvs import REPEATS, WARMUP, timed_calls  # noqa: E402

CONFIG, D = "euroc_752x480_10mm", 128
REF_POSE, POSE_STEP, MAX_SOURCES, MIN_DEPTH = 150, 5, 4, 0.8
MATCH_SOURCES = 2  # each keyframe's own depth comes from the two poses before it


def keyframes(s, cache):
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return z["rgb"], z["T"]
    frames = [s[REF_POSE - POSE_STEP * k] for k in range(MAX_SOURCES + MATCH_SOURCES + 1)]
    rgb, T = np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames])
    if cache:
        np.savez(cache, rgb=rgb, T=T)
    return rgb, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_consistency needs a GPU"
    s = SyntheticRGBD(CONFIG, noise=False, invalid_frac=0.0)
    rgb, T = keyframes(s, args.cache)
    vol = ScalableTSDFVolume(s.voxel, 0.04, max_blocks=1 << 10)
    d_rgb = torch.from_numpy(rgb).cuda()
    K = s.intrinsics
    mvs = dict(intrinsic=K, min_depth=MIN_DEPTH, num_planes=D, index=False)
    raw = torch.stack([vol.multiview_sgm(d_rgb[k], d_rgb[k + 1:k + 1 + MATCH_SOURCES], T_ref=T[k], T_sources=T[k + 1:k + 1 + MATCH_SOURCES], **mvs)[1]
                       for k in range(MAX_SOURCES + 1)])
    vol.synchronize()
    step = (1.0 / MIN_DEPTH) / (D - 1)
    out = {"metric": "depth_consistency", "config": CONFIG, "height": s.height, "width": s.width, "num_planes": D, "min_depth": MIN_DEPTH,
           "pose_step": POSE_STEP, "inv_depth_tol": round(step, 6), "repeats": REPEATS, "warmup": WARMUP, "check": {}}
    for N in (1, 2, 4):
        views, back_views = consistency_views(K, T[0], K, T[1:1 + N])
        st, walls, (depth, counts, stats) = timed_calls(vol, lambda: vol.filter_depth_consistency(
            raw[0], raw[1:1 + N], views, back_views, inv_depth_tol=step, rel_depth_tol=0.0, counts=True, stats=True))
        bst, bare, _ = timed_calls(vol, lambda: vol.filter_depth_consistency(raw[0], raw[1:1 + N], views, back_views, inv_depth_tol=step,
                                                                             rel_depth_tol=0.0, counts=True))
        mst, mwalls, _ = timed_calls(vol, lambda: vol.multiview_sgm(d_rgb[0], d_rgb[1:1 + N], T_ref=T[0], T_sources=T[1:1 + N], **mvs))
        kernel, with_stats, mvs_kernel = bst.sum(axis=1), st.sum(axis=1), mst.sum(axis=1)
        npx = s.height * s.width
        out["check"][f"n{N}"] = {
            "kernel_ms": round(float(np.median(kernel)), 4), "kernel_ms_spread": [round(float(kernel.min()), 4), round(float(kernel.max()), 4)],
            "device_wall_ms": round(float(np.median(bare)), 3), "kernel_with_stats_ms": round(float(np.median(with_stats)), 4),
            "device_wall_with_stats_ms": round(float(np.median(walls)), 3),
            "mvs_kernel_ms": round(float(np.median(mvs_kernel)), 3), "mvs_device_wall_ms": round(float(np.median(mwalls)), 3),
            "share_of_mvs": round(float(np.median(kernel) / np.median(mvs_kernel)), 4), "bytes_moved": npx * (12 + 4 * N),
            "valid_in": round(stats.valid_pixels / npx, 4), "kept": round(stats.kept_pixels / npx, 4),
            "mean_agree": round(stats.agree_sum / max(stats.valid_pixels, 1), 3)}
        assert int((depth > 0).sum().item()) == stats.kept_pixels and tuple(counts.shape) == (s.height, s.width, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
