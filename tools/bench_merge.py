"""Volume-to-volume fusion on its own: ScalableTSDFVolume.integrate_volume() of the map 512 frames of the synthetic 640x480 / 5 mm
stream build, moved by a generic rigid transform (23 deg about (0.3, 1, 0.2), translation (0.31, -0.12, 0.23) m)
  (a) into an empty volume (the "move a map" recipe),
  (b) into a volume that holds the first 256 frames, fused in the moved frame (the "join submaps" recipe; the source then holds the
      other 256),
against what the library offered for the same end before: reset() + integrate_batch of all frames at the moved poses.  All are
timed in the same run with HIP events on the destination's stream around the calls (the merge waits for the GPU, so the host clock
is given too).  Each merge is timed on a destination of its own after a warm-up merge into a twin.  Reported, not asserted.

Prints one JSON line:
  source_units                          units of the whole map
  empty_*  / half_*                     per case: ms (device events), wall_ms, sweep_ms (the sweep kernel alone), units_source (source
                                        units holding a weight), units_claimed, units_written (= the kept units the sweep ran over), voxels_updated, voxels_trilinear
  *_algorithmic_mb                      units written x 80 KiB x 2 (read + write) + source units held x 80 KiB
  *_gb_s                                that over ms
  replay_ms                             reset() + integrate_batch of all 512 frames at the moved poses, 64-frame calls (median of 3)
  replay_over_empty                     replay_ms / empty_ms"""
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


def generic_transform():
    k = np.array([0.3, 1.0, 0.2])
    k /= np.linalg.norm(k)
    a = np.radians(23.0)
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * Kx + (1.0 - np.cos(a)) * (Kx @ Kx)
    T[:3, 3] = (0.31, -0.12, 0.23)
    return T


def main():
    assert torch.cuda.is_available(), "bench_merge needs a GPU"
    s, depth, rgb, T = bench.load_frames("synthetic_640x480_5mm", N_MAP)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    dd, rr = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
    T = np.ascontiguousarray(T, dtype=np.float64)
    X = generic_transform()
    X_inv = np.linalg.inv(X)
    T_moved = np.ascontiguousarray(T @ X_inv)  # the poses in the frame p' = X p
    stream = torch.cuda.Stream()

    def new_volume():
        vol = ScalableTSDFVolume(bench.VOXEL, bench.SDF_TRUNC, max_blocks=1 << 17)
        vol.set_stream(stream.cuda_stream)
        return vol

    def replay(vol, poses, lo, hi):
        for k in range(lo // BATCH, hi // BATCH):
            sl = slice(BATCH * k, BATCH * k + BATCH)
            vol.integrate_batch(dd[sl], rr[sl], K, poses[sl], depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)

    def timed(vol, fn):
        vol.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out

    def merge_case(src, prepare):
        twin, dst = prepare(), prepare()
        twin.integrate_volume(src, X)  # warm-up: code objects loaded, allocator primed
        dst.synchronize()
        before = dst.num_blocks()
        dst.profile_enable(True)
        ms, wall, st = timed(dst, lambda: dst.integrate_volume(src, X))
        sweep_ms, _, written = dst.profile_read()
        dst.profile_enable(False)
        assert dst.num_blocks() - before == st.units_claimed
        mb = (written * 160 + st.units_source * 80) * 1024 / 1e6
        return twin, dst, {"ms": round(ms, 3), "wall_ms": round(wall, 3), "sweep_ms": round(sweep_ms, 3), "units_source": st.units_source,
                           "units_claimed": st.units_claimed,
                           "units_written": int(written), "voxels_updated": st.voxels_updated, "voxels_trilinear": st.voxels_trilinear,
                           "algorithmic_mb": round(mb, 1), "gb_s": round(mb / 1e3 / (ms * 1e-3), 1)}

    whole = new_volume()
    replay(whole, T, 0, N_MAP)
    whole.synchronize()
    twin, moved, empty = merge_case(whole, new_volume)
    source_units = whole.num_blocks()
    del twin, moved

    second = new_volume()
    replay(second, T, N_MAP // 2, N_MAP)
    second.synchronize()

    def first_half():
        vol = new_volume()
        replay(vol, T_moved, 0, N_MAP // 2)
        return vol

    twin, joined, half = merge_case(second, first_half)
    rb = [timed(twin, lambda: (twin.reset(), replay(twin, T_moved, 0, N_MAP)))[0] for _ in range(3)]
    replay_ms = float(np.median(rb))

    out = {"tool": "bench_merge", "width": s.width, "height": s.height, "voxel": bench.VOXEL, "map_frames": N_MAP,
           "source_units": source_units}
    out.update({"empty_" + k: v for k, v in empty.items()})
    out.update({"half_" + k: v for k, v in half.items()})
    out.update({"replay_ms": round(replay_ms, 3), "replay_over_empty": round(replay_ms / empty["ms"], 2),
                "units_after_join": joined.num_blocks(), "units_after_replay": twin.num_blocks()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
