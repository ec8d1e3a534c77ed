"""Frame-to-frame odometry on its own: _Volume.rgbd_odometry at 640x480 (synthetic_640x480_5mm) and 752x480 (euroc_752x480_10mm),
iterations (10, 5, 4), depth only and hybrid, beside ScalableTSDFVolume.track_frame_to_model on the same source frame and schedule
against a map fused from the frames around it, in the same run.  Reported, not asserted.

Prints one JSON line; per shape and method:
  kernel_ms             kernel time of the call's brackets (median over REPEATS calls after WARMUP), split into pyramids_ms (source
                        and target), model_ms (the k_odometry_model launches, one per level) and solve_ms (linearise + solve)
  device_wall_ms        wall time of one call on device tensors, ended by a synchronise
  track_kernel_ms       the tracker's brackets on the same frame: track_pyramid_ms, track_model_ms (ray casts, hybrid also the
                        record launches), track_solve_ms; track_device_wall_ms
  share_of_track        kernel_ms / track_kernel_ms
  model_bytes           what the model kernels of the three levels read and write: 17 B per pixel depth only (z in; normal, mask out),
                        37 B hybrid (also intensity in, record out); model_gbps = model_bytes / model_ms
  error_m, error_deg    against the ground-truth relative pose (the pair is TARGET, SOURCE = frames 40, 44)
and once per run copy_gbps: a device-to-device copy of 256 MiB (read + write bytes over its time).

--cache FILE.npz: keep the rendered frames there (rendering is host-side numpy)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyslam_amd.synthetic import SyntheticRGBD  # noqa: E402
from pyslam_amd.volumetric import PinholeCameraIntrinsic, ScalableTSDFVolume  # noqa: E402
from tools.bench_mvs import REPEATS, WARMUP, timed_calls  # noqa: E402

CONFIGS = ("synthetic_640x480_5mm", "euroc_752x480_10mm")
ITERATIONS = (10, 5, 4)
TARGET, SOURCE = 40, 44
MAP_FRAMES = range(36, 44)  # the map the tracker is measured against: eight frames before the source


def frames_of(config, cache):
    path = f"{cache}.{config}.npz" if cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        return z["depth"], z["rgb"], z["T"]
    s = SyntheticRGBD(config)
    fr = [s[i] for i in list(MAP_FRAMES) + [SOURCE]]
    depth, rgb, T = (np.stack([f[k] for f in fr]) for k in range(3))
    if path:
        np.savez(path, depth=depth, rgb=rgb, T=T)
    return depth, rgb, T


def copy_rate():
    a = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    times = []
    for rep in range(WARMUP + REPEATS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        b.copy_(a)
        t1.record()
        torch.cuda.synchronize()
        if rep >= WARMUP:
            times.append(t0.elapsed_time(t1))
    return 2 * a.numel() / (np.median(times) * 1e-3) / 1e9


def pose_error(T_a, T_b):
    D = T_a @ np.linalg.inv(T_b)
    c = np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(D[:3, 3])), float(np.degrees(np.arccos(c)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rgbd_odometry needs a GPU"
    nl, steps = len(ITERATIONS), sum(ITERATIONS)
    out = {"metric": "rgbd_odometry", "iterations": list(ITERATIONS), "pair": [TARGET, SOURCE], "repeats": REPEATS, "warmup": WARMUP,
           "copy_gbps": round(copy_rate(), 1), "shapes": {}}
    for config in CONFIGS:
        s = SyntheticRGBD(config)
        depth, rgb, T = frames_of(config, args.cache)
        K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
        d_depth, d_rgb = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
        vol = ScalableTSDFVolume(s.voxel, 8 * s.voxel, max_blocks=1 << 16)
        n_map = len(MAP_FRAMES)
        vol.integrate_batch(d_depth[:n_map], d_rgb[:n_map], K, T[:n_map], depth_scale=1.0, depth_trunc=4.0)
        vol.synchronize()
        ti, si = TARGET - MAP_FRAMES[0], n_map  # the target is one of the map's frames, the source the frame after them
        true = T[ti] @ np.linalg.inv(T[si])
        npx = sum((s.height >> l) * (s.width >> l) for l in range(nl))
        shape = {}
        for method in ("depth_only", "hybrid"):
            hybrid = method == "hybrid"
            okw = dict(source_color=d_rgb[si], target_color=d_rgb[ti]) if hybrid else {}
            tkw = dict(color=d_rgb[si]) if hybrid else {}
            st, walls, res = timed_calls(vol, lambda: vol.rgbd_odometry(d_depth[si], d_depth[ti], K, iterations=ITERATIONS, **okw))
            tst, twalls, tres = timed_calls(vol, lambda: vol.track_frame_to_model(d_depth[si], K, T[ti], iterations=ITERATIONS, **tkw))
            assert st.shape[1] == 3 * nl + 2 * steps, st.shape  # source + target pyramids, one model launch per level, the steps
            pyramids, model, solve = st[:, :2 * nl].sum(axis=1), st[:, 2 * nl:3 * nl].sum(axis=1), st[:, 3 * nl:].sum(axis=1)
            t_pyr, t_model, t_solve = tst[:, :nl].sum(axis=1), tst[:, nl:tst.shape[1] - 2 * steps].sum(axis=1), tst[:, -2 * steps:].sum(axis=1)
            kernel, t_kernel = st.sum(axis=1), tst.sum(axis=1)
            model_bytes = npx * (37 if hybrid else 17)
            em, ed = pose_error(res.transformation, true)
            tm, td = pose_error(tres.transformation, T[si])
            med = lambda x: round(float(np.median(x)), 4)
            shape[method] = {
                "kernel_ms": med(kernel), "kernel_ms_spread": [round(float(kernel.min()), 4), round(float(kernel.max()), 4)],
                "pyramids_ms": med(pyramids), "model_ms": med(model), "solve_ms": med(solve), "device_wall_ms": round(float(np.median(walls)), 3),
                "track_kernel_ms": med(t_kernel), "track_pyramid_ms": med(t_pyr), "track_model_ms": med(t_model), "track_solve_ms": med(t_solve),
                "track_device_wall_ms": round(float(np.median(twalls)), 3), "share_of_track": round(float(np.median(kernel) / np.median(t_kernel)), 4),
                "model_bytes": model_bytes, "model_gbps": round(model_bytes / (float(np.median(model)) * 1e-3) / 1e9, 1),
                "success": bool(res.success), "iterations_run": list(res.iterations), "error_m": round(em, 6), "error_deg": round(ed, 5),
                "track_success": bool(tres.success), "track_iterations_run": list(tres.iterations), "track_error_m": round(tm, 6),
                "track_error_deg": round(td, 5)}
        out["shapes"][f"{s.width}x{s.height}"] = shape
        vol.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
