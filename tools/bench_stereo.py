"""The stereo matcher on its own and in the stereo dense flow: _Volume.stereo_sgm at 752x480 (euroc_752x480_10mm), D = 128, paths 8
and 4, on synthetic stereo pairs (SyntheticRGBD.stereo, baseline 0.11 m).  Reported, not asserted.

Prints one JSON line; per variant ("paths8", "paths4"):
  stages_ms        kernel time of the call's four brackets [census, paths, winner, finish] (medians over REPEATS calls after WARMUP)
  kernel_ms        their sum;  kernel_ms_spread: [min, max]
  device_wall_ms   wall time of one call on device tensors into device tensors, ended by a synchronise
  valid_share      share of pixels with a disparity (first pair)
  flow_kf_per_s    keyframes per second of: pair (host uint8) -> upload -> stereo_sgm -> shadow filter -> TSDF integrate at 10 mm,
                   N_KEYFRAMES keyframes, best of FLOW_REPEATS passes on a fresh volume
and "stub_net": the same flow with DepthEstimatorStereoTorch on make_stub_stereo_net() in the matcher's place (a 5x5 convolution
whose disparity has nothing to do with the scene: the figure the stereo configuration was quoted with before).

--profile-calls N: nothing but N calls at paths 8 on one pair, for a counter pass (rocprofv3 --pmc ... --kernel-trace).
--cache FILE.npz: keep the rendered pairs there (rendering is host-side numpy, about 0.5 s per pair)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyslam_amd.depth_estimation import DepthEstimatorStereoTorch, make_stub_stereo_net  # noqa: E402
from pyslam_amd.synthetic import SyntheticRGBD  # noqa: E402
from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume  # noqa: E402

CONFIG, BASELINE, D = "euroc_752x480_10mm", 0.11, 128
N_KEYFRAMES, POSE_STEP, REPEATS, WARMUP, FLOW_REPEATS = 8, 10, 15, 3, 3
SDF_TRUNC, DEPTH_TRUNC = 0.04, 4.0


def pairs(s, n, cache):
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return z["left"], z["right"], z["T"]
    out = [s.stereo(POSE_STEP * i, BASELINE) for i in range(n)]
    left, right, T = np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[3] for o in out])
    if cache:
        np.savez(cache, left=left, right=right, T=T)
    return left, right, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile-calls", type=int, default=0)
    ap.add_argument("--cache", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stereo needs a GPU"
    s = SyntheticRGBD(CONFIG, noise=False, invalid_frac=0.0)
    left, right, T = pairs(s, 1 if args.profile_calls else N_KEYFRAMES, args.cache)
    bf = float(s.fx * BASELINE)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    vol = ScalableTSDFVolume(s.voxel, SDF_TRUNC, max_blocks=1 << 15)
    dl, dr = torch.from_numpy(left[0]).cuda(), torch.from_numpy(right[0]).cuda()
    if args.profile_calls:
        for _ in range(args.profile_calls):
            vol.stereo_sgm(dl, dr, num_disparities=D, paths=8, bf=bf)
        vol.synchronize()
        torch.cuda.synchronize()
        return
    med = lambda a: round(float(np.median(a)), 3)
    out = {"metric": "stereo_sgm", "config": CONFIG, "height": s.height, "width": s.width, "num_disparities": D, "baseline_m": BASELINE,
           "scratch_bytes": s.height * s.width * (2 * D + 22), "repeats": REPEATS, "warmup": WARMUP, "keyframes": N_KEYFRAMES}

    def flow(depth_of):
        best = 0.0
        for _ in range(FLOW_REPEATS):
            v = ScalableTSDFVolume(s.voxel, SDF_TRUNC, max_blocks=1 << 15)
            depth_of(v, left[0], right[0])  # (scratch and caches of the fresh volume)
            v.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(N_KEYFRAMES):
                depth = v.filter_shadow_points(depth_of(v, left[k], right[k]))
                v.integrate(RGBDImage(torch.from_numpy(left[k]).cuda(), depth, 1.0, DEPTH_TRUNC), K, T[k])
            v.synchronize()
            torch.cuda.synchronize()
            best = max(best, N_KEYFRAMES / (time.perf_counter() - t0))
            units = int(v.num_blocks())
            v.close()
        return round(best, 2), units

    for name, paths in (("paths8", 8), ("paths4", 4)):
        stages, walls = [], []
        for rep in range(WARMUP + REPEATS):
            vol.synchronize()
            torch.cuda.synchronize()
            vol.profile_enable(True)
            t0 = time.perf_counter()
            disp, depth = vol.stereo_sgm(dl, dr, num_disparities=D, paths=paths, bf=bf)
            vol.synchronize()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            per_stage = [float(x) for x in vol.profile_launches()]
            vol.profile_read()
            vol.profile_enable(False)
            if rep >= WARMUP:
                stages.append(per_stage)
                walls.append(wall)
        st = np.asarray(stages, np.float64)
        kf, units = flow(lambda v, a, b: v.stereo_sgm(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), num_disparities=D, paths=paths, bf=bf)[1])
        out[name] = {"stages_ms": [round(float(x), 3) for x in np.median(st, axis=0)], "kernel_ms": med(st.sum(axis=1)),
                     "kernel_ms_spread": [round(float(st.sum(axis=1).min()), 3), round(float(st.sum(axis=1).max()), 3)],
                     "device_wall_ms": med(walls), "device_wall_ms_spread": [round(min(walls), 3), round(max(walls), 3)],
                     "valid_share": round(float((disp >= 0).float().mean().item()), 4), "flow_kf_per_s": kf, "flow_units": units}
    cam = type("Camera", (), {"bf": bf})()
    stub = DepthEstimatorStereoTorch(make_stub_stereo_net(), cam, "cuda", keep_on_device=True)
    kf, units = flow(lambda v, a, b: stub.infer(a, b)[0])
    out["stub_net"] = {"flow_kf_per_s": kf, "flow_units": units}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
