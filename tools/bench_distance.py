"""The distance field on its own: ScalableTSDFVolume.distance_field on the map 512 frames of the synthetic 640x480 / 5 mm stream
build, over a 256 x 256 x 128 box of voxels centred at the camera's mid-trajectory position with R = 100 voxels (0.5 m), against the
only route a caller had before: dump() the whole pool to the host and run a distance transform there (tests/distance_reference.py,
the contract's restatement) - that one on a 64^3 box at R = 32, small enough to finish.  Reported, not asserted.

Prints one JSON line:
  units, box_origin, box_shape, radius, cells
  stats                       unknown, free, inside, sites, far cells of the box
  classify_ms, scan_x_ms, pass_y_ms, pass_z_ms    median device time per kernel over CALLS calls (profile brackets, device outputs)
  total_kernel_ms             their sum;  cells_per_s = cells / total_kernel_ms
  wall_ms_device              median wall time of a call with device=True, ended by a synchronise; wall_ms_host: numpy outputs
  classify_bytes              counted: per held brick the weight and tsdf planes (32 KiB) and 2 KiB per held face neighbour, plus 5
                              bytes written per cell (class, seed); classify_bytes_per_s = that over classify_ms
  pass_bytes                  counted traffic of the three passes: 16 + 8 + (4 read, 1 class read, 4 + 4 written) bytes per cell
  small_*                     the old route on the small box: dump_s, numpy_s, the library's wall time for the same box, and whether
                              the two agree bit for bit"""
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

N_MAP, BATCH, SHAPE, RADIUS, CALLS, WARMUP = 512, 64, (256, 256, 128), 100, 20, 3
SMALL_SHAPE, SMALL_RADIUS = (64, 64, 64), 32
OUTPUTS = ("distance", "dist2", "cls")


def bounds_of(origin, shape, voxel):
    """World bounds whose voxel box is exactly origin + [0, shape)."""
    origin = np.asarray(origin, np.float64)
    return (origin + 0.5) * voxel, (origin + np.asarray(shape) - 0.5) * voxel


def main():
    assert torch.cuda.is_available(), "bench_distance needs a GPU"
    s, depth, rgb, T = bench.load_frames("synthetic_640x480_5mm", N_MAP)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    dd, rr = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
    T = np.ascontiguousarray(T, dtype=np.float64)
    vol = ScalableTSDFVolume(bench.VOXEL, bench.SDF_TRUNC, max_blocks=1 << 17)
    for k in range(N_MAP // BATCH):
        sl = slice(BATCH * k, BATCH * k + BATCH)
        vol.integrate_batch(dd[sl], rr[sl], K, T[sl], depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)
    vol.synchronize()
    units = vol.num_blocks()

    T_mid = T[N_MAP // 2]
    camera = -T_mid[:3, :3].T @ T_mid[:3, 3]
    origin = np.floor(camera / bench.VOXEL).astype(np.int64) - np.asarray(SHAPE) // 2
    bounds = bounds_of(origin, SHAPE, bench.VOXEL)
    reach = RADIUS * bench.VOXEL - 1e-9
    cells = int(np.prod(SHAPE))

    def call(device):
        return vol.distance_field(bounds, reach, pad=False, outputs=OUTPUTS, device=device)

    for _ in range(WARMUP):
        field = call(True)
    torch.cuda.synchronize()
    assert field.shape == SHAPE and field.origin.tolist() == origin.tolist() and field.radius == RADIUS
    vol.profile_enable(True)
    for _ in range(CALLS):
        call(True)
    per_launch = np.asarray(vol.profile_launches(), np.float64).reshape(CALLS, 4)
    vol.profile_read()
    vol.profile_enable(False)
    kernel_ms = np.median(per_launch, axis=0)
    total_ms = float(np.median(per_launch.sum(axis=1)))

    def wall_ms(device, calls):
        times = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(device)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times))

    wall_dev, wall_host = wall_ms(True, CALLS), wall_ms(False, 5)

    # what classify must move: the held bricks of the box and their held face neighbours
    held = {tuple(k) for k in vol.unit_keys().tolist()}
    u0, u1 = origin >> 4, (origin + np.asarray(SHAPE) - 1) >> 4
    bricks = held_bricks = held_faces = 0
    for ux in range(int(u0[0]), int(u1[0]) + 1):
        for uy in range(int(u0[1]), int(u1[1]) + 1):
            for uz in range(int(u0[2]), int(u1[2]) + 1):
                bricks += 1
                if (ux, uy, uz) in held:
                    held_bricks += 1
                    held_faces += sum((ux + dx, uy + dy, uz + dz) in held
                                      for dx, dy, dz in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)))
    classify_bytes = held_bricks * 32768 + held_faces * 2048 + cells * 5
    pass_bytes = cells * (16 + 8 + 13)

    # the old route on a small box, once
    from tests import distance_reference as dr

    small_origin = np.floor(camera / bench.VOXEL).astype(np.int64) - np.asarray(SMALL_SHAPE) // 2
    small_bounds = bounds_of(small_origin, SMALL_SHAPE, bench.VOXEL)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    small = vol.distance_field(small_bounds, SMALL_RADIUS * bench.VOXEL - 1e-9, pad=False, outputs=OUTPUTS)
    small_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    dump = vol.dump()
    dump_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = dr.distance_field(dump, bench.VOXEL, small_origin, SMALL_SHAPE, SMALL_RADIUS)
    numpy_s = time.perf_counter() - t0
    equal = all(np.array_equal(np.ascontiguousarray(getattr(small, name)).view(np.uint8), np.ascontiguousarray(ref[name]).view(np.uint8)) for name in OUTPUTS) \
        and small.stats.as_tuple() == ref["stats"]

    print(json.dumps({
        "tool": "bench_distance", "voxel": bench.VOXEL, "units": units, "box_origin": origin.tolist(), "box_shape": list(SHAPE),
        "radius": RADIUS, "cells": cells, "stats": list(field.stats.as_tuple()),
        "classify_ms": round(float(kernel_ms[0]), 4), "scan_x_ms": round(float(kernel_ms[1]), 4), "pass_y_ms": round(float(kernel_ms[2]), 4),
        "pass_z_ms": round(float(kernel_ms[3]), 4), "total_kernel_ms": round(total_ms, 4), "cells_per_s": round(cells / (total_ms * 1e-3), 1),
        "wall_ms_device": round(wall_dev, 3), "wall_ms_host": round(wall_host, 3),
        "bricks": bricks, "held_bricks": held_bricks, "classify_bytes": classify_bytes,
        "classify_bytes_per_s": round(classify_bytes / (float(kernel_ms[0]) * 1e-3), 1),
        "pass_bytes": pass_bytes, "pass_bytes_per_s": round(pass_bytes / (float(kernel_ms[1:].sum()) * 1e-3), 1),
        "small_shape": list(SMALL_SHAPE), "small_radius": SMALL_RADIUS, "small_library_s": round(small_s, 4), "small_dump_s": round(dump_s, 3),
        "small_numpy_s": round(numpy_s, 3), "dump_bytes": int(sum(a.nbytes for a in dump)), "small_equal_to_numpy": bool(equal),
    }))


if __name__ == "__main__":
    main()
