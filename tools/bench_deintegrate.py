"""TSDF de-integration on its own: device time of ScalableTSDFVolume.integrate_batch / deintegrate_batch / reintegrate_batch for
the same 64 frames of the synthetic 640x480 / 5 mm stream, on a map those frames and 448 more built, and the loop-closure
comparison: re-integrating 64 of the map's 512 frames against reset() + a replay of all 512.

Prints one JSON line:
  integrate_ms     median device time of integrate_batch(64 frames) (HIP events on the volume's stream around the call)
  deintegrate_ms   ... of deintegrate_batch(the same 64 frames) (the asynchronous C call: no stats read-back in the interval)
  reintegrate_ms   ... of reintegrate_batch(the same 64 frames, old = new poses)
  rebuild_ms       ... of reset() + integrate_batch of all 512 frames in 64-frame calls
  deint_over_int   deintegrate_ms / integrate_ms (target: <= 2)
  rebuild_over_re  rebuild_ms / reintegrate_ms
  wall_deintegrate_ms  mean wall time of the Python deintegrate_batch (waits once, reads the stats)
The map is restored after every timed call that changes it (integrate after deintegrate), so every repetition sees the same map."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pyslam_amd import _lib as L  # noqa: E402
from pyslam_amd.volumetric import PinholeCameraIntrinsic, ScalableTSDFVolume  # noqa: E402

N_MAP, BATCH, REPS = 512, 64, 5


def main():
    assert torch.cuda.is_available(), "bench_deintegrate needs a GPU"
    s, depth, rgb, T = bench.load_frames("synthetic_640x480_5mm", N_MAP)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    intr = K.as_array()
    dd, rr = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
    T = np.ascontiguousarray(T, dtype=np.float64)
    stream = torch.cuda.Stream()
    vol = ScalableTSDFVolume(bench.VOXEL, bench.SDF_TRUNC, max_blocks=1 << 17)
    vol.set_stream(stream.cuda_stream)
    H, W = s.height, s.width

    def replay():
        for k in range(N_MAP // BATCH):
            sl = slice(BATCH * k, BATCH * k + BATCH)
            vol.integrate_batch(dd[sl], rr[sl], K, T[sl], depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)

    replay()
    torch.cuda.synchronize()
    vol.synchronize()
    units = vol.num_blocks()
    # the 64 frames of the timed calls: every 8th frame of the map (a loop closure corrects keyframes spread over the map)
    sel = np.arange(0, N_MAP, N_MAP // BATCH)
    d64, c64 = dd[sel].contiguous(), rr[sel].contiguous()
    T64 = np.ascontiguousarray(T[sel].reshape(BATCH, 16))
    torch.cuda.synchronize()

    def timed(fn):
        vol.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def deint_async():
        L.check(vol._lib.hv_tsdf_deintegrate_batch(vol._h, L.ptr(d64), L.HV_DEPTH_F32, L.ptr(c64), BATCH, H, W, L.ptr(intr), L.ptr(T64),
                                                   1.0, bench.DEPTH_TRUNC, L.HV_DEVICE, None))

    def integ():
        vol.integrate_batch(d64, c64, K, T64, depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)

    def reint_async():
        L.check(vol._lib.hv_tsdf_reintegrate_batch(vol._h, L.ptr(d64), L.HV_DEPTH_F32, L.ptr(c64), BATCH, H, W, L.ptr(intr), L.ptr(T64),
                                                   L.ptr(T64), 1.0, bench.DEPTH_TRUNC, L.HV_DEVICE, None))

    de, it, re = [], [], []
    for rep in range(REPS + 1):  # the first repetition warms up
        x, y, z = timed(deint_async), timed(integ), timed(reint_async)
        if rep:
            de.append(x)
            it.append(y)
            re.append(z)
    t0 = time.perf_counter()
    for _ in range(REPS):
        st = vol.deintegrate_batch(d64, c64, K, T64, depth_trunc=bench.DEPTH_TRUNC)
        integ()
    vol.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / REPS  # (deintegrate + the restoring integrate's launch)
    rb = []
    for rep in range(3):
        rb.append(timed(lambda: (vol.reset(), replay())))
    out = {
        "tool": "bench_deintegrate", "width": W, "height": H, "voxel": bench.VOXEL, "map_frames": N_MAP, "frames": BATCH, "units": units,
        "integrate_ms": round(float(np.median(it)), 3), "deintegrate_ms": round(float(np.median(de)), 3),
        "reintegrate_ms": round(float(np.median(re)), 3), "rebuild_ms": round(float(np.median(rb)), 3),
        "wall_deintegrate_plus_integrate_launch_ms": round(wall, 3),
        "stats": {"units_listed": st.units_listed, "units_missing": st.units_missing, "voxels_removed": st.voxels_removed,
                  "voxels_underflow": st.voxels_underflow},
    }
    out["deint_over_int"] = round(out["deintegrate_ms"] / out["integrate_ms"], 3)
    out["rebuild_over_re"] = round(out["rebuild_ms"] / out["reintegrate_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
