"""Cleaning the map on its own: ScalableTSDFVolume.surface_components and remove_small_components on the map 512 frames of the
synthetic 640x480 / 5 mm stream build, next to one full extract_triangle_mesh tick of the same map and to the route a caller had
before on the host: scipy.ndimage.label (3 x 3 x 3 structure) over the dense box of the same sites.  Reported, not asserted.

Every repeat starts from the same map: it is packed once on the device and unpacked into the emptied volume before each repeat, so
the removal always has its floaters to remove and the extraction is always a full one (no per-unit cache survives an unpack).  The
four measurements are interleaved inside a repeat; the figures are medians over REPEATS repeats after WARMUP.

Prints one JSON line:
  units, sites, components, largest, min_sites, margin
  label_device_ms / label_wall_ms     surface_components(sites=True, device=True): the sum of its bracketed launches (both calls of the
                                      count-then-fill pair; the three radix sorts are one bracket) / wall time ended by a synchronise
  label_kernels_ms                    the launches of the fill call, by name
  remove_device_ms / remove_wall_ms   remove_small_components(min_sites), the same two ways;  remove_kernels_ms by name;  remove_stats
  extract_wall_ms                     extract_triangle_mesh(device=True) of the restored map;  triangles
  scipy_label_s                       ndimage.label on the dense bool box of the sites (host; LABEL_REPEATS repeats), box_shape,
                                      scipy_components and whether that count equals the library's"""
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

N_MAP, BATCH, REPEATS, WARMUP, LABEL_REPEATS, MIN_SITES = 512, 64, 7, 2, 3, 200
MAX_LABEL_CELLS = 600_000_000  # the dense box is one byte per cell going in and four coming out
COUNT_CALL = ("sites", "scan", "local", "cross", "flatten", "init", "sizes", "table")
FILL_CALL = ("sites", "scan", "local", "cross", "flatten", "init", "sizes_boxes", "seed_y", "seed_z", "sorts", "table", "list")
REMOVE_CALL = ("sites", "scan", "local", "cross", "flatten", "init", "sizes", "table", "small", "reset")


def main():
    assert torch.cuda.is_available(), "bench_components needs a GPU"
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
    packed = vol.pack(device=True)
    margin = min(16, int(np.ceil(bench.SDF_TRUNC / bench.VOXEL)))

    def restore():
        vol.reset()
        vol.unpack(packed)
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def profiled(fn, launches):
        vol.profile_enable(True)
        out, wall = timed(fn)
        per = np.asarray(vol.profile_launches(), np.float64)
        vol.profile_read()
        vol.profile_enable(False)
        assert len(per) == launches, (len(per), launches)
        return out, wall, per

    rows = {"label_wall": [], "label_dev": [], "label_k": [], "remove_wall": [], "remove_dev": [], "remove_k": [], "extract_wall": [], "scipy": []}
    comps = stats = mesh = None
    box_shape, scipy_components = None, None
    for rep in range(WARMUP + REPEATS):
        restore()
        mesh, t_extract = timed(lambda: vol.extract_triangle_mesh(device=True))
        comps, t_label, k_label = profiled(lambda: vol.surface_components(sites=True, device=True), len(COUNT_CALL) + len(FILL_CALL))
        t_scipy = None
        if WARMUP <= rep < WARMUP + LABEL_REPEATS and len(comps) > 0:
            from scipy import ndimage

            idx = comps.site_index.cpu().numpy().astype(np.int64)
            lo = idx.min(axis=0)
            box_shape = (idx.max(axis=0) - lo + 1).tolist()
            if int(np.prod(box_shape)) <= MAX_LABEL_CELLS:
                grid = np.zeros(box_shape, bool)
                grid[tuple((idx - lo).T)] = True
                t0 = time.perf_counter()
                _, scipy_components = ndimage.label(grid, structure=np.ones((3, 3, 3)))
                t_scipy = time.perf_counter() - t0
                del grid
        stats, t_remove, k_remove = profiled(lambda: vol.remove_small_components(MIN_SITES), len(REMOVE_CALL))
        if rep < WARMUP:
            continue
        rows["extract_wall"].append(t_extract)
        rows["label_wall"].append(t_label)
        rows["label_dev"].append(k_label.sum())
        rows["label_k"].append(k_label[len(COUNT_CALL):])
        rows["remove_wall"].append(t_remove)
        rows["remove_dev"].append(k_remove.sum())
        rows["remove_k"].append(k_remove)
        if t_scipy is not None:
            rows["scipy"].append(t_scipy)

    med = lambda a: float(np.median(np.asarray(a, np.float64), axis=0)) if np.ndim(a) == 1 else np.median(np.asarray(a, np.float64), axis=0)
    print(json.dumps({
        "tool": "bench_components", "voxel": bench.VOXEL, "units": units, "sites": comps.stats.sites, "components": comps.stats.components,
        "largest": comps.stats.largest, "min_sites": MIN_SITES, "margin": margin, "repeats": REPEATS,
        "label_device_ms": round(med(rows["label_dev"]), 4), "label_wall_ms": round(med(rows["label_wall"]), 3),
        "label_kernels_ms": {n: round(float(v), 4) for n, v in zip(FILL_CALL, med(rows["label_k"]))},
        "remove_device_ms": round(med(rows["remove_dev"]), 4), "remove_wall_ms": round(med(rows["remove_wall"]), 3),
        "remove_kernels_ms": {n: round(float(v), 4) for n, v in zip(REMOVE_CALL, med(rows["remove_k"]))},
        "remove_stats": stats._asdict(),
        "extract_wall_ms": round(med(rows["extract_wall"]), 3), "triangles": int(mesh.triangles.shape[0]),
        "scipy_label_s": round(med(rows["scipy"]), 3) if rows["scipy"] else None, "box_shape": box_shape,
        "scipy_components": None if scipy_components is None else int(scipy_components),
        "scipy_count_equal": None if scipy_components is None else bool(int(scipy_components) == comps.stats.components),
    }))


if __name__ == "__main__":
    main()
