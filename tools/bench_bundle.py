"""Bundle adjustment on its own: _Volume.bundle_adjust on planted problems (tests/bundle_cases.planted_problem) at a local shape (20
cameras, 2 000 points, 10 000 observations) and a global one (500 / 50 000 / 300 000), device operands, at most MAX_ITERATIONS outer
iterations.  Reported, not asserted; no target is claimed.

Writes profiles/bundle_adjust/bench_bundle.json and prints it as one JSON line; per shape:
  iterations, converged, cg_iterations_total, chi2_initial, chi2_final      of the call with the default CG stopping rule
  wall_ms_per_iteration, kernel_ms_per_iteration   wall time and the call's own brackets per outer iteration (medians)
  cg_iteration_us           one CG iteration (direction, pass 1, pass 2, update): the difference of two calls of ONE outer iteration
                            with cg_tolerance = 0 and CG_LONG / CG_SHORT inner iterations, over their difference
  pass_points_us, pass_cams_us, pass_*_gbps   with --kernel-stats FILE (the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats`
                            run of this tool with --shape global), on that shape's row: the mean time of k_bd_schur_points / k_bd_schur_cams and the bytes they stream per
                            call over it - per observation q (24) + A (48) + list entry (4) + index pair (8), pass 2 also the point's
                            y (24); per point (C + lambda I)^-1 (48), y (24), row (4); per camera B (168), p and q (96), row (4)
  copy_gbps                 a device-to-device copy of COPY_MB in the same run (read + write bytes over the time)"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyslam_amd.volumetric import ScalableTSDFVolume  # noqa: E402
from tests import bundle_cases as C  # noqa: E402

SHAPES = {"local": (20, 2000, 10000), "global": (500, 50000, 300000)}
WARMUP, REPEATS = 1, 5
MAX_ITERATIONS = 10
CG_SHORT, CG_LONG = 20, 120
COPY_MB = 256


class Pinhole:
    fx, fy, cx, cy = (C.PINHOLE[k] for k in ("fx", "fy", "cx", "cy"))


def copy_rate():
    n = COPY_MB << 20
    a, b = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    b.copy_(a)
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        b.copy_(a)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return 2 * n / float(np.median(t)) / 1e9


def pass_bytes(N, M, O):
    return {"k_bd_schur_points": O * 84 + M * 76, "k_bd_schur_cams": O * 108 + N * 268}


def kernel_means(path):
    """{kernel name: mean microseconds} of a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in ("k_bd_schur_points", "k_bd_schur_cams"):
                if k in name:
                    out[k] = float(row["AverageNs"]) / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--shape", default=None, choices=sorted(SHAPES))
    ap.add_argument("--stats-shape", default="global", choices=sorted(SHAPES), help="the shape the profiled run of --kernel-stats was made with")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bundle needs a GPU"
    vol = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)
    out = {"metric": "bundle_adjust", "repeats": REPEATS, "warmup": WARMUP, "max_iterations": MAX_ITERATIONS, "copy_gbps": round(copy_rate(), 1),
           "shapes": {}}
    for name, (N, M, O) in SHAPES.items():
        if args.shape not in (None, name):
            continue
        c = C.planted_problem(N, M, O)
        O = len(c["idx"])
        dev = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("cameras", "points", "idx", "meas", "inv_sigma2", "fixed")}

        def call(**kw):
            vol.synchronize()
            vol.profile_enable(True)
            vol.profile_read()
            t0 = time.perf_counter()
            res = vol.bundle_adjust(dev["cameras"], dev["points"], dev["idx"], dev["meas"], Pinhole, bf=C.PINHOLE["bf"], inv_sigma2=dev["inv_sigma2"],
                                    camera_fixed=dev["fixed"], **kw)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            ms = vol.profile_launches()
            vol.profile_enable(False)
            return res, wall, [float(x) for x in ms[:res.iterations]]

        kernel, wall, res = [], [], None
        for rep in range(WARMUP + REPEATS):
            res, w, ms = call(max_iterations=MAX_ITERATIONS)
            if rep >= WARMUP:
                kernel += ms
                wall.append(w / res.iterations)
        cg = {}
        for n in (CG_SHORT, CG_LONG):
            t = [call(max_iterations=1, cg_tolerance=0.0, cg_max_iterations=n)[2][0] for _ in range(WARMUP + REPEATS)][WARMUP:]
            cg[n] = float(np.median(t))
        row = {"cameras": N, "points": M, "observations": O, "iterations": res.iterations, "converged": res.converged,
               "cg_iterations_total": res.cg_iterations_total, "chi2_initial": res.chi2_initial, "chi2_final": res.chi2_final,
               "wall_ms_per_iteration": round(float(np.median(wall)), 3), "kernel_ms_per_iteration": round(float(np.median(kernel)), 3),
               "cg_iteration_us": round((cg[CG_LONG] - cg[CG_SHORT]) * 1e3 / (CG_LONG - CG_SHORT), 2)}
        out["shapes"][name] = row
    if args.kernel_stats:
        out["kernel_stats_note"] = ("means over every launch of a profiled run with --shape " + args.stats_shape + ", the launches that return at "
                                    "once because the CG has ended included: the times are lower bounds of a working launch, the rates upper bounds")
        means = kernel_means(args.kernel_stats)
        for name, row in out["shapes"].items():
            if name != args.stats_shape:
                continue
            for k, us in means.items():
                short = "pass_points" if k.endswith("points") else "pass_cams"
                row[short + "_us"] = round(us, 2)
                row[short + "_gbps"] = round(pass_bytes(row["cameras"], row["points"], row["observations"])[k] / us / 1e3, 1)
    vol.close()
    path = os.path.join(ROOT, "profiles", "bundle_adjust", "bench_bundle.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
