"""The stereo matcher on its own and in the stereo dense flow: _Volume.stereo_sgm at 752x480 (euroc_752x480_10mm), D = 128, paths 8
and 4, on synthetic stereo pairs (SyntheticRGBD.stereo, baseline 0.11 m).  Reported, not asserted.

Prints one JSON line; per variant ("paths8", "paths4"):
  stages_ms        kernel time of the call's four brackets [census, paths, winner, finish] (medians over REPEATS calls after WARMUP)
  kernel_ms        their sum;  kernel_ms_spread: [min, max]
  device_wall_ms   wall time of one call on device tensors into device tensors, ended by a synchronise
  valid_share      share of pixels with a disparity (first pair)
  flow_kf_per_s    keyframes per second of: pair (host uint8) -> upload -> stereo_sgm -> shadow filter -> TSDF integrate at 10 mm,
                   N_KEYFRAMES keyframes, best of FLOW_REPEATS passes on a fresh volume
  with_filter      the same call with speckle_window_size = 50, speckle_range = 1 (the reference's values): stages_ms (the four brackets
                   of the matcher, then the filter's four [local, cross, flatten, apply]), kernel_ms, filter_kernel_ms, filter_share (of
                   the matcher's kernel time in the same calls), device_wall_ms, flow_kf_per_s
  host_wall_ms / with_filter.host_wall_ms   wall time of one call on host arrays into host arrays
"filter": hv_filter_speckles alone at 50 / 1 (device tensors, kernel time of its four brackets): "matcher_output" on the disparity
of the first pair (paths 8), "all_equal" on a constant image - one region, the contention case of the size count.
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


def timed_calls(vol, call):
    """WARMUP + REPEATS calls, each between two synchronisations -> {"stages": [REPEATS, brackets] kernel ms, "walls": [REPEATS] ms}"""
    stages, walls = [], []
    for rep in range(WARMUP + REPEATS):
        vol.synchronize()
        torch.cuda.synchronize()
        vol.profile_enable(True)
        t0 = time.perf_counter()
        call()
        vol.synchronize()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        per_stage = [float(x) for x in vol.profile_launches()]
        vol.profile_read()
        vol.profile_enable(False)
        if rep >= WARMUP:
            stages.append(per_stage)
            walls.append(wall)
    return {"stages": np.asarray(stages, np.float64), "walls": walls}


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
        filtered = timed_calls(vol, lambda: vol.stereo_sgm(dl, dr, num_disparities=D, paths=paths, bf=bf, speckle_window_size=50, speckle_range=1))
        fst = filtered["stages"]
        host = timed_calls(vol, lambda: vol.stereo_sgm(left[0], right[0], num_disparities=D, paths=paths, bf=bf))
        host_filtered = timed_calls(vol, lambda: vol.stereo_sgm(left[0], right[0], num_disparities=D, paths=paths, bf=bf, speckle_window_size=50,
                                                                 speckle_range=1))
        kf_f, units_f = flow(lambda v, a, b: v.stereo_sgm(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), num_disparities=D, paths=paths,
                                                          bf=bf, speckle_window_size=50, speckle_range=1)[1])
        with_filter = {"stages_ms": [round(float(x), 3) for x in np.median(fst, axis=0)], "kernel_ms": med(fst.sum(axis=1)),
                       "filter_kernel_ms": med(fst[:, 4:].sum(axis=1)),
                       "filter_share": round(float(np.median(fst[:, 4:].sum(axis=1) / fst[:, :4].sum(axis=1))), 4),
                       "device_wall_ms": med(filtered["walls"]), "host_wall_ms": med(host_filtered["walls"]), "flow_kf_per_s": kf_f,
                       "flow_units": units_f}
        kf, units = flow(lambda v, a, b: v.stereo_sgm(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), num_disparities=D, paths=paths, bf=bf)[1])
        out[name] = {"stages_ms": [round(float(x), 3) for x in np.median(st, axis=0)], "kernel_ms": med(st.sum(axis=1)),
                     "kernel_ms_spread": [round(float(st.sum(axis=1).min()), 3), round(float(st.sum(axis=1).max()), 3)],
                     "device_wall_ms": med(walls), "device_wall_ms_spread": [round(min(walls), 3), round(max(walls), 3)],
                     "valid_share": round(float((disp >= 0).float().mean().item()), 4), "flow_kf_per_s": kf, "flow_units": units,
                     "host_wall_ms": med(host["walls"]), "with_filter": with_filter}
    disp8 = vol.stereo_sgm(dl, dr, num_disparities=D, paths=8, bf=bf)[0]
    out["filter"] = {}
    for name, image in (("matcher_output", disp8), ("all_equal", torch.full_like(disp8, 160))):
        t = timed_calls(vol, lambda: vol.filter_speckles(image, 50, 16))["stages"]
        out["filter"][name] = {"stages_ms": [round(float(x), 4) for x in np.median(t, axis=0)], "kernel_ms": round(float(np.median(t.sum(axis=1))), 4),
                               "kernel_ms_spread": [round(float(t.sum(axis=1).min()), 4), round(float(t.sum(axis=1).max()), 4)]}
    cam = type("Camera", (), {"bf": bf})()
    stub = DepthEstimatorStereoTorch(make_stub_stereo_net(), cam, "cuda", keep_on_device=True)
    kf, units = flow(lambda v, a, b: stub.infer(a, b)[0])
    out["stub_net"] = {"flow_kf_per_s": kf, "flow_units": units}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
