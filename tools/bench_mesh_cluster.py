"""The simplified mesh on its own: ScalableTSDFVolume.extract_simplified_mesh at cell 2, 4, 8 and 16 beside extract_triangle_mesh, on
the map 512 frames of the synthetic 640x480 / 5 mm stream build.  Reported, not asserted.

A TICK here is what an output tick of a running reconstruction is: one keyframe fused (so the contents changed and nothing cached
is valid; the per-unit masks and the classification are updated where that keyframe wrote), then one extraction.  Every measured
call is preceded by its own keyframe, the five variants and the three destinations are interleaved inside a repeat, and the figures
are medians over REPEATS repeats after WARMUP.

Prints one JSON line; per variant ("full", "cell2", "cell4", "cell8", "cell16"):
  vertices, triangles
  kernel_ms            the sum of the call's bracketed launches;  stages_ms: each bracket - full mesh: [masks + classification + scan,
                       vertices + triangles]; simplified: [masks + classification + scan, cells + scan, cluster vertices, candidate
                       count + scan, candidates + two sorts + flags + scan, compaction]
  device_wall_ms       wall time of the call into torch tensors on the volume's GPU (float64), ended by a synchronise
  host_f32_wall_ms     wall time into host float32 arrays;  host_f64_wall_ms: into host float64 arrays
  bytes_f32 / bytes_f64   bytes handed over (vertices + colours + triangles)
and "kernel_ms_spread" / "..._wall_ms_spread": [min, max] over the repeats."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume  # noqa: E402

N_MAP, BATCH, REPEATS, WARMUP = 512, 64, 9, 3
VARIANTS = (("full", 0), ("cell2", 2), ("cell4", 4), ("cell8", 8), ("cell16", 16))
MODES = (("device", dict(device=True)), ("host_f32", dict(dtype=np.float32)), ("host_f64", dict()))


def main():
    assert torch.cuda.is_available(), "bench_mesh_cluster needs a GPU"
    s, depth, rgb, T = bench.load_frames("synthetic_640x480_5mm", N_MAP)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    dd, rr = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
    T = np.ascontiguousarray(T, dtype=np.float64)
    vol = ScalableTSDFVolume(bench.VOXEL, bench.SDF_TRUNC, max_blocks=1 << 17)
    for k in range(N_MAP // BATCH):
        sl = slice(BATCH * k, BATCH * k + BATCH)
        vol.integrate_batch(dd[sl], rr[sl], K, T[sl], depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)
    vol.synchronize()
    tick = [0]

    def one_tick(cell, kw):
        i = tick[0] % N_MAP
        tick[0] += 1
        vol.integrate(RGBDImage(rr[i], dd[i], 1.0, bench.DEPTH_TRUNC), K, T[i])
        vol.synchronize()
        torch.cuda.synchronize()
        vol.profile_enable(True)
        t0 = time.perf_counter()
        m = vol.extract_simplified_mesh(cell=cell, **kw) if cell else vol.extract_triangle_mesh(**kw)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        stages = [float(x) for x in vol.profile_launches()]
        kernel = vol.profile_read()[0]
        vol.profile_enable(False)
        return m, wall, kernel, stages

    rows = {(v, m): [] for v, _ in VARIANTS for m, _ in MODES}
    kernels = {v: [] for v, _ in VARIANTS}
    stages = {v: [] for v, _ in VARIANTS}
    sizes = {}
    for rep in range(WARMUP + REPEATS):
        for name, cell in VARIANTS:
            for mode, kw in MODES:
                m, wall, kernel, per_stage = one_tick(cell, kw)
                if rep >= WARMUP:
                    rows[(name, mode)].append(wall)
                    kernels[name].append(kernel)
                    stages[name].append(per_stage)
                sizes[name] = (len(m.vertices), len(m.triangles))
                del m
    med = lambda a: round(float(np.median(a)), 3)
    spread = lambda a: [round(float(np.min(a)), 3), round(float(np.max(a)), 3)]
    out = {"metric": "mesh_cluster", "units": int(vol.num_blocks()), "frames": N_MAP, "repeats": REPEATS, "warmup": WARMUP}
    for name, _ in VARIANTS:
        nv, nt = sizes[name]
        r = {"vertices": nv, "triangles": nt, "kernel_ms": med(kernels[name]), "kernel_ms_spread": spread(kernels[name]),
             "stages_ms": [round(float(x), 3) for x in np.median(np.asarray(stages[name], np.float64), axis=0)],
             "bytes_f32": nv * 24 + nt * 12, "bytes_f64": nv * 48 + nt * 12}
        for mode, _ in MODES:
            r[mode + "_wall_ms"] = med(rows[(name, mode)])
            r[mode + "_wall_ms_spread"] = spread(rows[(name, mode)])
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
