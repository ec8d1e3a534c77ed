"""Features, matching and the appearance loop step on their own: _Volume.detect_features at 640x480 and 752x480 with 3 levels,
_Volume.match_features of 1000 queries against 1, 64 and 512 segments of 1000 descriptors, and one
KeyframeGraphRgbd.close_loops_by_appearance step on the seven keyframes of tests/orb_cases.  Reported, not asserted.

Writes profiles/orb_features/bench_features.json and prints the same JSON line:
  detect[WxH]     keypoints, stages_ms = kernel time of the call's four brackets [grey + pyramid, segment test, select + scan, describe]
                  (medians over REPEATS calls after WARMUP), kernel_ms their sum, device_wall_ms of a call on a device tensor
  match[S]        pairs = 1000 x S x 1000 (x2 with the cross-check pass: pairs_computed), kernel_ms of the call's one bracket,
                  pairs_per_s = pairs_computed / kernel time, and its share of valu_bound_pairs_per_s
  valu_bound_pairs_per_s   256 CUs x 4 SIMDs x 32 lanes x CLOCK_HZ / 16 VALU operations per pair (8 xor, 8 accumulating popcounts)
  loop_step       wall_ms of one close_loops_by_appearance call (seven 160x120 keyframes on the device, features already kept), the
                  pairs it verified and the edges it added"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyslam_amd.pose_graph import KeyframeGraphRgbd  # noqa: E402
from pyslam_amd.synthetic import SyntheticRGBD  # noqa: E402
from pyslam_amd.volumetric import ScalableTSDFVolume  # noqa: E402
from tests import orb_cases as oc  # noqa: E402

WARMUP, REPEATS = 3, 15
CLOCK_HZ = 2.4e9
VALU_BOUND = 256 * 4 * 32 * CLOCK_HZ / 16
OUT = os.path.join(ROOT, "profiles", "orb_features", "bench_features.json")


def timed_calls(vol, call):
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
    return np.asarray(stages, np.float64), walls


def main():
    assert torch.cuda.is_available(), "bench_features needs a GPU"
    vol = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)
    med = lambda a: round(float(np.median(a)), 4)  # noqa: E731
    out = {"metric": "orb_features", "repeats": REPEATS, "warmup": WARMUP, "clock_hz": CLOCK_HZ, "valu_bound_pairs_per_s": VALU_BOUND,
           "detect": {}, "match": {}}
    for config in ("synthetic_640x480_5mm", "euroc_752x480_10mm"):
        s = SyntheticRGBD(config, noise=False, invalid_frac=0.0)
        rgb = torch.from_numpy(np.ascontiguousarray(s[0][1])).cuda()
        n = int(vol.detect_features(rgb, levels=3).keypoints.shape[0])
        st, walls = timed_calls(vol, lambda: vol.detect_features(rgb, levels=3))
        out["detect"]["%dx%d" % (s.width, s.height)] = {"keypoints": n, "stages_ms": [med(st[:, k]) for k in range(st.shape[1])],
                                                        "kernel_ms": med(st.sum(axis=1)), "device_wall_ms": med(walls)}
    rng = np.random.default_rng(0)
    q = torch.from_numpy(rng.integers(0, 256, (1000, 32), dtype=np.uint8)).cuda()
    for S in (1, 64, 512):
        t = torch.from_numpy(rng.integers(0, 256, (1000 * S, 32), dtype=np.uint8)).cuda()
        seg = np.arange(S + 1, dtype=np.int32) * 1000
        st, walls = timed_calls(vol, lambda: vol.match_features(q, t, segments=seg))
        ms = float(np.median(st.sum(axis=1)))
        pairs = 1000 * 1000 * S
        out["match"][str(S)] = {"pairs": pairs, "pairs_computed": 2 * pairs, "kernel_ms": round(ms, 4), "device_wall_ms": med(walls),
                                "pairs_per_s": 2 * pairs / (ms * 1e-3), "share_of_valu_bound": round(2 * pairs / (ms * 1e-3) / VALU_BOUND, 4)}
    K, frames, cam = oc.loop_frames()
    walls, log, added = [], [], []
    for _ in range(1 + 3):
        kg = KeyframeGraphRgbd(vol, cam, method="hybrid", T_wc0=np.linalg.inv(frames[0][2]), features=oc.LOOP_FEATURES, **oc.LOOP_ODOMETRY)
        for depth, rgb, _ in frames:
            kg.add_frame(rgb, depth)
        vol.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        added = kg.close_loops_by_appearance(**oc.LOOP_PARAMS)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        log = kg.appearance_log
    out["loop_step"] = {"keyframes": len(frames), "wall_ms": med(walls[1:]), "pairs_verified": len(log), "edges_added": len(added)}
    vol.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    line = json.dumps(out)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
