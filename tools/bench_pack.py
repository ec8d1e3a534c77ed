"""Packed maps on their own: ScalableTSDFVolume.pack / unpack / save / load of the map 512 frames of the synthetic 640x480 / 5 mm
stream build, against the only route the library had for the same job before: export_numerators(unit_keys()) followed by
import_numerators into an empty volume (80 KiB per unit whatever it holds, and a tsdf that is re-divided on import).  All are timed in
the same run with HIP events on the volume's stream around the calls; every one of them waits for the GPU, so the host clock is
given too.  Medians of REPS runs after a warm-up.  Reported, not asserted.

Prints one JSON line:
  units, stored_voxels                  of the map; stored_fraction = stored_voxels / (units x 4096)
  packed_bytes, raw_bytes               raw = units x 81 920; packed_over_raw = their ratio
  pack_device_* / pack_host_*           pack(device=True) / pack(): ms (device events), wall_ms
  unpack_device_* / unpack_host_*       unpack of a CUDA tensor / of the page-locked host array into a reset volume
  save_* / load_*                       save(path) / load(path) on the temporary directory's file system (wall only)
  numerators_device_* / numerators_host_*   export_numerators + import_numerators through a CUDA tensor / a host array
  roundtrip_exact                       the unpacked volume packs to the same bytes"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pyslam_amd.volumetric import PinholeCameraIntrinsic, ScalableTSDFVolume  # noqa: E402

N_MAP, BATCH, REPS = 512, 64, 5


def main():
    assert torch.cuda.is_available(), "bench_pack needs a GPU"
    s, depth, rgb, T = bench.load_frames("synthetic_640x480_5mm", N_MAP)
    K = PinholeCameraIntrinsic(s.width, s.height, *s.intrinsics)
    dd, rr = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
    T = np.ascontiguousarray(T, dtype=np.float64)
    stream = torch.cuda.Stream()

    def new_volume():
        vol = ScalableTSDFVolume(bench.VOXEL, bench.SDF_TRUNC, max_blocks=1 << 17)
        vol.set_stream(stream.cuda_stream)
        return vol

    def timed(vol, fn):
        vol.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out

    def median(vol, fn, prepare=None, reps=REPS):
        ms, wall = [], []
        for i in range(reps + 1):  # the first run warms up: code objects, allocator, page-locked blocks
            if prepare:
                prepare()
            m, w, _ = timed(vol, fn)
            if i:
                ms.append(m)
                wall.append(w)
        return {"ms": round(float(np.median(ms)), 3), "wall_ms": round(float(np.median(wall)), 3)}

    with torch.cuda.stream(stream):
        vol = new_volume()
        for k in range(N_MAP // BATCH):
            sl = slice(BATCH * k, BATCH * k + BATCH)
            vol.integrate_batch(dd[sl], rr[sl], K, T[sl], depth_scale=1.0, depth_trunc=bench.DEPTH_TRUNC)
        vol.synchronize()
        units = vol.num_blocks()
        host = vol.pack()
        dev = vol.pack(device=True)
        info = ScalableTSDFVolume.packed_info(host)
        out = {"tool": "bench_pack", "width": s.width, "height": s.height, "voxel": bench.VOXEL, "map_frames": N_MAP, "units": units,
               "stored_voxels": info["voxels"], "stored_fraction": round(info["voxels"] / max(1, units * 4096), 4),
               "packed_bytes": info["bytes"], "raw_bytes": units * 81920, "packed_over_raw": round(info["bytes"] / max(1, units * 81920), 4)}
        res = {"pack_device": median(vol, lambda: vol.pack(device=True)), "pack_host": median(vol, lambda: vol.pack())}
        dst = new_volume()
        res["unpack_device"] = median(dst, lambda: dst.unpack(dev), prepare=dst.reset)
        res["unpack_host"] = median(dst, lambda: dst.unpack(host), prepare=dst.reset)
        out["roundtrip_exact"] = bool(dst.pack().tobytes() == host.tobytes())
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "map.hvtsdf")
            res["save"] = median(vol, lambda: vol.save(path), reps=3)
            res["load"] = median(vol, lambda: ScalableTSDFVolume.load(path), reps=3)
        # the route of the parent commit: numerators out, numerators in
        keys = vol.unit_keys()
        payload_dev = torch.empty((units, 4096, 5), dtype=torch.float32, device="cuda")
        stream.synchronize()

        def numerators(payload):
            vol.export_numerators(keys, out=payload)
            dst.import_numerators(keys, payload)

        res["numerators_device"] = median(dst, lambda: numerators(payload_dev), prepare=dst.reset, reps=3)
        del payload_dev
        payload_host = np.zeros((units, 4096, 5), np.float32)
        res["numerators_host"] = median(dst, lambda: numerators(payload_host), prepare=dst.reset, reps=1)
        out["numerators_bytes"] = int(payload_host.nbytes)
    for name, r in res.items():
        if name not in ("save", "load"):  # (load runs on the new volume's own stream: the events here do not bracket it)
            out[name + "_ms"] = r["ms"]
        out[name + "_wall_ms"] = r["wall_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
