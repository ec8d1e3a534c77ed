"""Frame-to-model tracking on its own: device and wall time of ScalableTSDFVolume.track_frame_to_model at 640x480 with
iterations (10, 5, 4) on the volume ten 32-frame batches of the synthetic 640x480 / 5 mm stream build (~24 k units), and the pose
error it reaches from perturbed starts.

Prints one JSON line:
  device_ms          mean summed device time of one call (profile_enable / profile_read brackets around every launch)
  cast_ms            of which the three model ray casts
  pyramid_ms         of which the source pyramid
  track_ms           of which the linearise + solve steps (every queued step, also those that return at once)
  wall_ms            mean wall time of a call from a host depth frame (staging, launches, result read-back)
  iterations_mean    mean linearisations run per level (level 0 first)
  pose_err_*         max / median distance (m) and angle (deg) to the true pose over the timed calls
The steps are latency-bound (a 640x480 linearisation reads ~6 MB); their time is not a fraction of any roofline.
--color: the hybrid call (color = the frame's image, intensity_weight 0.01, intensity_huber_delta 0.1) timed beside the depth-only
call in the same run, the two alternating call by call: the line gains "color" with the same fields plus prep_ms (the model
preparation launches), and "weight_sweep": the pose errors of the same starts at intensity_weight 0.001, 0.01 and 0.1.
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
from tests import track_reference as tr  # noqa: E402

N_FRAMES, BATCH, CALLS, WARMUP = 320, 32, 40, 5
ITERATIONS = (10, 5, 4)
WEIGHT, DELTA_I, SWEEP = 0.01, 0.1, (0.001, 0.01, 0.1)


def perturbed(T_cw, k):
    """A start 2 cm / 1 deg off the true pose, in a direction that turns with k."""
    a = 2.4 * k
    xi = np.array([np.cos(a), np.sin(a), 0.5, -np.sin(a), 0.5, np.cos(a)])
    xi[:3] *= np.radians(1.0) / np.linalg.norm(xi[:3])
    xi[3:] *= 0.02 / np.linalg.norm(xi[3:])
    return np.linalg.inv(np.linalg.inv(T_cw) @ tr.exp_twist(xi))


def main():
    assert torch.cuda.is_available(), "bench_track needs a GPU"
    s, depth, rgb, T = bench.load_frames("synthetic_640x480_5mm", N_FRAMES)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    dd, rr = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
    vol = ScalableTSDFVolume(bench.VOXEL, bench.SDF_TRUNC, max_blocks=1 << 17)
    for k in range(N_FRAMES // BATCH):
        sl = slice(BATCH * k, BATCH * k + BATCH)
        vol.integrate_batch(dd[sl], rr[sl], K, T[sl], depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)
    vol.synchronize()
    units = vol.num_blocks()
    frames = [(i * 7) % N_FRAMES for i in range(CALLS)]
    starts = [perturbed(T[f], i) for i, f in enumerate(frames)]

    with_color = "--color" in sys.argv[1:]

    def call(i, weight=None):
        if weight is None:
            return vol.track_frame_to_model(depth[frames[i]], K, starts[i], iterations=ITERATIONS)
        return vol.track_frame_to_model(depth[frames[i]], K, starts[i], iterations=ITERATIONS, color=rgb[frames[i]],
                                        intensity_weight=weight, intensity_huber_delta=DELTA_I)

    modes = [None, WEIGHT] if with_color else [None]
    for i in range(WARMUP):
        for w in modes:
            call(i, w)
    torch.cuda.synchronize()

    nl = len(ITERATIONS)
    # launches of a call in order: pyramid levels, per level the cast (hybrid: and the model preparation), linearise + solve per step
    vol.profile_enable(True)
    vol.profile_read()  # (reset)
    split = {w: dict(pyramid=0.0, cast=0.0, prep=0.0, steps=0.0) for w in modes}
    for i in range(CALLS):
        for w in modes:  # alternating: both see the same state of the box
            call(i, w)
            ms = vol.profile_launches()
            vol.profile_read()  # (reset)
            per_level = 1 if w is None else 2
            assert len(ms) == nl + per_level * nl + 2 * sum(ITERATIONS), (len(ms), w)
            model = ms[nl:nl + per_level * nl]
            split[w]["pyramid"] += float(ms[:nl].sum())
            split[w]["cast"] += float(model[::per_level].sum())
            split[w]["prep"] += float(model[1::per_level].sum()) if w is not None else 0.0
            split[w]["steps"] += float(ms[nl + per_level * nl:].sum())
    vol.profile_enable(False)

    def report(w):
        t0 = time.perf_counter()
        outs = [call(i, w) for i in range(CALLS)]
        wall = (time.perf_counter() - t0) * 1e3 / CALLS
        errs = np.array([tr.pose_error(o.transformation, T[f]) for o, f in zip(outs, frames)])
        iters = np.mean([o.iterations for o in outs], axis=0)
        sp = split[w]
        out = {"device_ms": round(sum(sp.values()) / CALLS, 4), "cast_ms": round(sp["cast"] / CALLS, 4),
               "pyramid_ms": round(sp["pyramid"] / CALLS, 4), "track_ms": round(sp["steps"] / CALLS, 4), "wall_ms": round(wall, 3),
               "iterations_mean": [round(float(x), 2) for x in iters], "success_frac": float(np.mean([o.success for o in outs]))}
        out.update(pose_errors(errs))
        if w is not None:
            out.update(prep_ms=round(sp["prep"] / CALLS, 4), intensity_weight=w, intensity_huber_delta=DELTA_I,
                       photometric_frac=round(float(np.mean([o.photometric_inliers / max(o.inliers, 1) for o in outs])), 4),
                       intensity_rmse_mean=round(float(np.mean([o.intensity_rmse for o in outs])), 5))
        return out

    line = {"tool": "bench_track", "width": s.width, "height": s.height, "voxel": bench.VOXEL, "units": units, "calls": CALLS,
            "iterations": list(ITERATIONS)}
    line.update(report(None))
    if with_color:
        line["color"] = report(WEIGHT)
        sweep = []
        for w in SWEEP:
            outs = [call(i, w) for i in range(CALLS)]
            errs = np.array([tr.pose_error(o.transformation, T[f]) for o, f in zip(outs, frames)])
            sweep.append(dict({"intensity_weight": w, "success_frac": float(np.mean([o.success for o in outs]))}, **pose_errors(errs)))
        line["weight_sweep"] = sweep
    print(json.dumps(line))


def pose_errors(errs):
    return {"pose_err_max_m": round(float(errs[:, 0].max()), 7), "pose_err_median_m": round(float(np.median(errs[:, 0])), 7),
            "pose_err_max_deg": round(float(errs[:, 1].max()), 6), "pose_err_median_deg": round(float(np.median(errs[:, 1])), 6)}


if __name__ == "__main__":
    main()
