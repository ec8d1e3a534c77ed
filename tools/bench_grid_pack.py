"""Packed grids on their own: pack / unpack / save / load of the semantic map the bench's keyframe flow builds (synthetic 640x480
keyframes, 1 cm voxels, assign + remap + integrate per keyframe as tools/bench_semantic.py drives it from host images), against the
only route to the whole state that existed before: dump2(), which walks all bs^3 voxels of every block through the host and that
nothing reads back.  All are timed in the same run with HIP events on the grid's stream around the calls; every one of them waits
for the GPU, so the host clock is given too.  Medians of REPS runs after a warm-up.  Reported, not asserted.

Prints one JSON line per payload (voting, probabilistic):
  blocks, stored_voxels, extra_pairs    of the map; stored_fraction = stored_voxels / (blocks x 512)
  packed_bytes, pool_bytes              pool = blocks x bytes_per_block; packed_over_pool = their ratio
  pack_device_* / pack_host_*           pack(device=True) / pack(): ms (device events), wall_ms
  unpack_device_* / unpack_host_*       unpack of a CUDA tensor / of the host array into a cleared grid
  save_* / load_*                       save(path) / load(path) on the temporary directory's file system (wall only)
  dump2_wall_ms                         dump2(max_labels=7) of the same map
  roundtrip_exact                       the unpacked grid packs to the same bytes"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyslam_amd.synthetic import SyntheticRGBD  # noqa: E402
from pyslam_amd.volumetric import CameraFrustrum  # noqa: E402
from pyslam_amd.volumetric_semantic import (VoxelBlockSemanticGrid, VoxelBlockSemanticProbabilisticGrid, remap_instance_ids,  # noqa: E402
                                            set_next_object_id)
from tests.semantic_helpers import semantic_frame  # noqa: E402

FRAMES, STRIDE, VOXEL, REPS = 24, 3, 0.01, 5


def main():
    assert torch.cuda.is_available(), "bench_grid_pack needs a GPU"
    s = SyntheticRGBD("synthetic_640x480_5mm")
    intr = s.intrinsics
    frames = [semantic_frame(s, STRIDE * i, shuffle=i) for i in range(FRAMES)]
    for name, cls in (("voting", VoxelBlockSemanticGrid), ("probabilistic", VoxelBlockSemanticProbabilisticGrid)):
        stream = torch.cuda.Stream()

        def new_grid():
            g = cls(VOXEL, 8, max_blocks=1 << 17, max_points=max(1 << 20, s.width * s.height))
            g.set_stream(stream.cuda_stream)
            return g

        def timed(g, fn):
            g.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            t0 = time.perf_counter()
            out = fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out

        def median(g, fn, prepare=None, reps=REPS):
            ms, wall = [], []
            for i in range(reps + 1):  # the first run warms up: code objects, allocator, page-locked blocks
                if prepare:
                    prepare()
                m, w, _ = timed(g, fn)
                if i:
                    ms.append(m)
                    wall.append(w)
            return {"ms": round(float(np.median(ms)), 3), "wall_ms": round(float(np.median(wall)), 3)}

        with torch.cuda.stream(stream):
            g = new_grid()
            fr = CameraFrustrum(*intr, s.width, s.height, np.eye(4), depth_max=8.0, depth_min=0.01)
            set_next_object_id(1)
            for depth, rgb, T, cls_img, inst_img in frames:
                d = g.filter_shadow_points(depth)
                fr.set_T_cw(T)
                m = g.assign_object_ids_to_instance_ids(fr, cls_img, inst_img, d, depth_threshold=0.03, do_carving=False, min_vote_ratio=0.5, min_votes=3)
                obj = remap_instance_ids(inst_img, m, volume=g)
                g.integrate_rgbd(d, rgb, *intr, T, class_ids_image=cls_img, object_ids_image=obj, max_depth=4.0, use_depths=True)
            g.synchronize()
            host = g.pack()
            dev = g.pack(device=True)
            info = cls.packed_info(host)
            pool = info["blocks"] * g.bytes_per_block()
            out = {"tool": "bench_grid_pack", "payload": name, "width": s.width, "height": s.height, "voxel": VOXEL, "map_frames": FRAMES,
                   "blocks": info["blocks"], "stored_voxels": info["voxels"], "extra_pairs": info["extra_pairs"],
                   "stored_fraction": round(info["voxels"] / max(1, info["blocks"] * 512), 4), "packed_bytes": info["bytes"], "pool_bytes": pool,
                   "packed_over_pool": round(info["bytes"] / max(1, pool), 4)}
            res = {"pack_device": median(g, lambda: g.pack(device=True)), "pack_host": median(g, lambda: g.pack())}
            dst = new_grid()
            res["unpack_device"] = median(dst, lambda: dst.unpack(dev), prepare=dst.clear)
            res["unpack_host"] = median(dst, lambda: dst.unpack(host), prepare=dst.clear)
            out["roundtrip_exact"] = bool(dst.pack().tobytes() == host.tobytes())
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "map.hvgrid")
                res["save"] = median(g, lambda: g.save(path), reps=3)
                res["load"] = median(g, lambda: cls.load(path), reps=3)
            res["dump2"] = median(g, lambda: g.dump2(max_labels=7), reps=3)
        for key, r in res.items():
            if key not in ("save", "load", "dump2"):  # (load runs on the new grid's own stream; dump2 is host work between small copies)
                out[key + "_ms"] = r["ms"]
            out[key + "_wall_ms"] = r["wall_ms"]
        print(json.dumps(out), flush=True)
        del g, dst, host, dev


if __name__ == "__main__":
    main()
