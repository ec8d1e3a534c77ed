"""TSDF pruning on its own: ScalableTSDFVolume.prune() on the map 512 frames of the synthetic 640x480 / 5 mm stream build, after
the last 64 of them were de-integrated again, against what the library offered for the same end before: reset() + a replay of the
remaining 448 frames.  Both are timed in the same run, with HIP events on the volume's stream around the calls; prune() is timed on
a volume of its own after a warm-up call on a twin in the same state (the call is not repeatable: the first one releases).

Prints one JSON line:
  units_scanned / units_released / units_moved   units held at the call / released / survivors moved into holes
  prune_ms         device-event time of prune() (the whole call: it waits for the GPU)   wall_prune_ms   the same by the host clock
  noop_prune_ms    ... of a second prune() on the pruned map (nothing to release: the scan alone)
  algorithmic_mb   scanned x 16 KiB read + moved x 80 KiB read and written + released x 80 KiB zeroed
  prune_gb_s       that over prune_ms (the scan leaves a unit at its first weight, so fewer bytes than this are read)
  rebuild_ms       reset() + integrate_batch of the remaining 448 frames in 64-frame calls (median of 3)
  rebuild_over_prune   the condition: > 1
  extract_full_ms_before / _after   kernels of one full-pass mesh extraction (HV_EXTRACT_INCREMENTAL=0) before / after the prune
  raycast_ms_before / _after        kernel of one 640x480 ray cast at a fused pose (median of 9) before / after the prune"""
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

N_MAP, BATCH = 512, 64
KEPT = N_MAP - BATCH


def main():
    assert torch.cuda.is_available(), "bench_prune needs a GPU"
    os.environ["HV_EXTRACT_INCREMENTAL"] = "0"  # every extraction below is a full pass
    s, depth, rgb, T = bench.load_frames("synthetic_640x480_5mm", N_MAP)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    dd, rr = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
    T = np.ascontiguousarray(T, dtype=np.float64)
    stream = torch.cuda.Stream()

    def replay(vol, n):
        for k in range(n // BATCH):
            sl = slice(BATCH * k, BATCH * k + BATCH)
            vol.integrate_batch(dd[sl], rr[sl], K, T[sl], depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)

    def timed(vol, fn):
        vol.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out

    def kernels_ms(vol, fn, reps=1):
        ms = []
        for _ in range(reps):
            vol.profile_enable(True)
            fn()
            total, launches, _ = vol.profile_read()
            vol.profile_enable(False)
            ms.append(total)
        return float(np.median(ms))

    vols = []
    for _ in range(2):  # [0] the warm-up twin, [1] the measured volume
        vol = ScalableTSDFVolume(bench.VOXEL, bench.SDF_TRUNC, max_blocks=1 << 17)
        vol.set_stream(stream.cuda_stream)
        replay(vol, N_MAP)
        vol.deintegrate_batch(dd[KEPT:], rr[KEPT:], K, T[KEPT:], depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)
        vols.append(vol)
    twin, vol = vols
    pose = T[KEPT // 2]

    def cast(v):
        return lambda: v.ray_cast(K, pose, 0.1, bench.DEPTH_TRUNC, 3.0, device=True)

    def mesh(v):
        return lambda: v.extract_triangle_mesh(device=True)

    cast(vol)()
    # (the first extraction after a change of the map is the one that runs the kernels: a repeat is served from the result cache)
    extract_before, raycast_before = kernels_ms(vol, mesh(vol)), kernels_ms(vol, cast(vol), 9)
    tris_before = len(vol.extract_triangle_mesh(device=True).triangles)

    order_before = vol.unit_keys()
    twin.prune()  # warm-up: code objects loaded, allocator primed
    prune_ms, wall_ms, st = timed(vol, vol.prune)
    noop_ms, _, st2 = timed(vol, vol.prune)
    assert st2.as_tuple() == (st.units_after, 0, 0, st.units_after), st2
    kept = {tuple(k) for k in vol.unit_keys()}
    moved = sum(tuple(k) in kept for k in order_before[st.units_after:])
    released = st.units_before - st.units_after

    extract_after, raycast_after = kernels_ms(vol, mesh(vol)), kernels_ms(vol, cast(vol), 9)
    tris_after = len(vol.extract_triangle_mesh(device=True).triangles)
    assert tris_after == tris_before, (tris_before, tris_after)

    rb = [timed(twin, lambda: (twin.reset(), replay(twin, KEPT)))[0] for _ in range(3)]
    rebuild_ms = float(np.median(rb))

    mb = (st.units_before * 16 + moved * 160 + released * 80) * 1024 / 1e6
    out = {
        "tool": "bench_prune", "width": s.width, "height": s.height, "voxel": bench.VOXEL, "map_frames": N_MAP, "removed_frames": BATCH,
        "units_scanned": st.units_before, "units_released": released, "units_moved": int(moved), "units_after": st.units_after,
        "prune_ms": round(prune_ms, 3), "wall_prune_ms": round(wall_ms, 3), "noop_prune_ms": round(noop_ms, 3),
        "algorithmic_mb": round(mb, 1), "prune_gb_s": round(mb / 1e3 / (prune_ms * 1e-3), 1),
        "rebuild_ms": round(rebuild_ms, 3), "rebuild_over_prune": round(rebuild_ms / prune_ms, 2),
        "extract_full_ms_before": round(extract_before, 3), "extract_full_ms_after": round(extract_after, 3),
        "raycast_ms_before": round(raycast_before, 4), "raycast_ms_after": round(raycast_after, 4), "triangles": tris_after,
        "units_after_rebuild": twin.num_blocks(),
    }
    print(json.dumps(out))
    assert prune_ms < rebuild_ms, "prune() must be faster than reset() + replay"


if __name__ == "__main__":
    main()
