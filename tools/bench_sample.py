"""Point queries on their own: ScalableTSDFVolume.sample_points and check_frame on the map 512 frames of the synthetic 640x480 / 5 mm
stream build, against the only route a caller had for the same values before: dump() the whole pool to the host and interpolate in
numpy (tests/sample_reference.py, the contract's restatement).  Reported, not asserted.

Prints one JSON line:
  units                       of the map
  points                      queried: surface points of the map (extract_point_cloud), each moved by up to +-sdf_trunc / 2 per axis
  status_share                share of the points per status (outside, unobserved, nearest, trilinear)
  sample_kernel_ms            mean device time of one sample_points over the points (profile_enable / profile_read brackets): sdf,
                              gradient, weight and status, no colour; sample_color_kernel_ms: with colour as well
  sample_wall_ms_device       mean wall time of such a call on a torch CUDA tensor, ended by a synchronise; ..._host: numpy in, numpy out
  points_per_s                points / sample_kernel_ms
  check_kernel_ms             mean device time of one 640x480 check_frame over input keyframes at their poses; check_wall_ms_device /
                              check_wall_ms_host: wall time with the depth on the GPU / on the host (the call waits for the counts)
  check_counts                mean pixels per class over those frames (invalid, unknown, consistent, in_front, behind)
  dump_s, numpy_s             the old route, once: dump() of the whole map, then the numpy interpolation of the same points
  dump_bytes                  what dump() brings to the host
  equal_to_numpy              the two routes agree bit for bit on every output"""
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

N_MAP, BATCH, N_POINTS, CALLS, WARMUP, FRAMES = 512, 64, 1 << 20, 20, 3, 16


def main():
    assert torch.cuda.is_available(), "bench_sample needs a GPU"
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

    surface = vol.extract_point_cloud(device=True).points
    g = torch.Generator(device="cuda").manual_seed(1)
    pick = torch.randint(0, surface.shape[0], (N_POINTS,), generator=g, device="cuda")
    jitter = (torch.rand((N_POINTS, 3), generator=g, device="cuda", dtype=torch.float64) - 0.5) * bench.SDF_TRUNC
    points = (surface[pick].to(torch.float64) + jitter).contiguous()
    points_host = points.cpu().numpy()
    frames = [(i * N_MAP) // FRAMES for i in range(FRAMES)]

    def kernel_ms(fn, calls):
        for i in range(WARMUP):
            fn(i)
        torch.cuda.synchronize()
        vol.profile_enable(True)
        for i in range(calls):
            fn(i)
        total, launches, _ = vol.profile_read()
        vol.profile_enable(False)
        return total / max(launches, 1)

    def wall_ms(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(calls):
            fn(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    k_plain = kernel_ms(lambda i: vol.sample_points(points, gradient=True, color=False), CALLS)
    k_color = kernel_ms(lambda i: vol.sample_points(points, gradient=True, color=True), CALLS)
    w_dev = wall_ms(lambda i: vol.sample_points(points, gradient=True, color=False), CALLS)
    w_host = wall_ms(lambda i: vol.sample_points(points_host, gradient=True, color=False), 5)
    res = vol.sample_points(points_host, gradient=True, color=True)
    share = np.bincount(res.status, minlength=4) / float(N_POINTS)

    def check(i, device):
        f = frames[i % FRAMES]
        return vol.check_frame(dd[f] if device else depth[f], K, T[f], depth_max=bench.DEPTH_TRUNC)

    k_check = kernel_ms(lambda i: check(i, True), FRAMES)
    w_check_dev = wall_ms(lambda i: check(i, True), FRAMES)
    w_check_host = wall_ms(lambda i: check(i, False), FRAMES)
    counts = np.mean([check(i, True).stats.as_tuple() for i in range(FRAMES)], axis=0)

    # the old route, once
    from tests import sample_reference as sr

    t0 = time.perf_counter()
    dump = vol.dump()
    dump_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = sr.sample_points(dump, bench.VOXEL, bench.SDF_TRUNC, points_host)
    numpy_s = time.perf_counter() - t0
    equal = all(np.array_equal(np.asarray(getattr(res, name)).view(np.uint8), ref[name].view(np.uint8))
                for name in ("sdf", "gradient", "color", "weight", "status"))
    print(json.dumps({
        "tool": "bench_sample", "voxel": bench.VOXEL, "units": units, "points": N_POINTS,
        "status_share": [round(float(x), 4) for x in share],
        "sample_kernel_ms": round(k_plain, 4), "sample_color_kernel_ms": round(k_color, 4),
        "sample_wall_ms_device": round(w_dev, 3), "sample_wall_ms_host": round(w_host, 3),
        "points_per_s": round(N_POINTS / (k_plain * 1e-3), 1),
        "width": s.width, "height": s.height, "check_kernel_ms": round(k_check, 4), "check_wall_ms_device": round(w_check_dev, 3),
        "check_wall_ms_host": round(w_check_host, 3), "check_counts": [round(float(x), 1) for x in counts],
        "dump_s": round(dump_s, 3), "numpy_s": round(numpy_s, 3), "dump_bytes": int(sum(a.nbytes for a in dump)),
        "equal_to_numpy": bool(equal),
    }))


if __name__ == "__main__":
    main()
