"""Point lookups on their own: lookup_points of the voting and the probabilistic semantic grid at the vertices of the TSDF map's mesh -
the labelled-surface recipe of INTEGRATION section 15 - device in, device out.  Reported, not asserted.

The TSDF map is fused from N_MAP frames of the synthetic 640x480 / 5 mm stream (bench.py's stream and voxel size); the two grids
(2 cm voxels, 8^3 blocks) take every KEY_STRIDE-th of those frames as a keyframe with its class / instance images.  The points are the
vertices of extract_triangle_mesh(device=True), float64, in the extraction's order (spatially coherent, not sorted).

Prints one JSON line:
  units, vertices             of the TSDF map and its mesh
  keyframes, blocks           fed to each grid / blocks each grid holds
  per grid (voting, probabilistic) and radius (0, 1):
    kernel_ms                 mean device time of one lookup_points over all vertices (profile_enable / profile_read brackets)
    wall_ms                   mean wall time of such a call on the torch CUDA tensor, ended by a synchronise
    points_per_s              vertices / kernel_ms
    status_share              share of the vertices per status (missing, own, near, invalid)
  label_mesh_wall_ms          label_mesh(mesh, radius=1) on the voting grid, wall time ended by a synchronise"""
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
from pyslam_amd.volumetric_semantic import VoxelBlockSemanticGrid, VoxelBlockSemanticProbabilisticGrid  # noqa: E402

N_MAP, BATCH, KEY_STRIDE, GRID_VOXEL, CALLS, WARMUP = 128, 64, 8, 0.02, 20, 3


def main():
    assert torch.cuda.is_available(), "bench_lookup needs a GPU"
    s, depth, rgb, T = bench.load_frames("synthetic_640x480_5mm", N_MAP)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    dd, rr = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
    T = np.ascontiguousarray(T, dtype=np.float64)
    vol = ScalableTSDFVolume(bench.VOXEL, bench.SDF_TRUNC, max_blocks=1 << 17)
    for k in range(N_MAP // BATCH):
        sl = slice(BATCH * k, BATCH * k + BATCH)
        vol.integrate_batch(dd[sl], rr[sl], K, T[sl], depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)
    vol.synchronize()
    mesh = vol.extract_triangle_mesh(device=True)
    points = mesh.vertices.contiguous()
    n = int(points.shape[0])

    keyframes = list(range(0, N_MAP, KEY_STRIDE))
    grids = {"voting": VoxelBlockSemanticGrid(GRID_VOXEL, 8, max_blocks=1 << 15, max_points=s.width * s.height),
             "probabilistic": VoxelBlockSemanticProbabilisticGrid(GRID_VOXEL, 8, max_blocks=1 << 15, max_points=s.width * s.height)}
    for i in keyframes:
        lab = torch.from_numpy(np.ascontiguousarray(s.labels(i), dtype=np.int32)).cuda()
        for g in grids.values():
            g.integrate_rgbd(dd[i], rr[i], *s.intrinsics, T[i], class_ids_image=lab, object_ids_image=lab % 3, max_depth=bench.DEPTH_TRUNC)
    out = {"tool": "bench_lookup", "tsdf_voxel": bench.VOXEL, "grid_voxel": GRID_VOXEL, "frames": N_MAP, "units": vol.num_blocks(), "vertices": n,
           "keyframes": len(keyframes), "width": s.width, "height": s.height}

    def kernel_ms(g, fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        g.profile_enable(True)
        for _ in range(CALLS):
            fn()
        total, launches, _ = g.profile_read()
        g.profile_enable(False)
        return total / max(launches, 1)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / CALLS

    for name, g in grids.items():
        g.synchronize()
        out[name] = {"blocks": g.num_blocks()}
        for radius in (0, 1):
            fn = lambda: g.lookup_points(points, radius=radius)  # noqa: E731
            k = kernel_ms(g, fn)
            w = wall_ms(fn)
            st = g.lookup_points(points, radius=radius, stats=True).stats
            out[name][f"radius{radius}"] = {"kernel_ms": round(k, 4), "wall_ms": round(w, 3), "points_per_s": round(n / (k * 1e-3), 1),
                                            "status_share": [round(x / float(n), 4) for x in (st.missing, st.own, st.near, st.invalid)]}
    out["label_mesh_wall_ms"] = round(wall_ms(lambda: grids["voting"].label_mesh(mesh, radius=1)), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
