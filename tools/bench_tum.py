#!/usr/bin/env python3
"""Secondary benchmark: BASELINE configs[0]'s shape - TUM fr1: 640x480, TUM1 intrinsics WITH their lens
distortion, uint16 depth / 5000 (settings/TUM1.yaml:27-39,54) - as one timed leg: pageable host keyframes -> H2D (pipelined
staging) -> undistort / rectify on the device (hv_tsdf_set_rectify_maps: colour bilinear, depth nearest,
volumetric_integrator_base.py:758-786,1017-1043) -> multi-frame TSDF sweep -> marching cubes every `mesh_every` frames, all
inside one clock; and the same stream written as a TUM folder (png + associations + groundtruth) through the drop-in for
main_map_dense_reconstruction.py (pyslam_amd/tools/dense_reconstruction.py).  No TUM data is in the image: the stream is the
synthetic scene rendered through TUM1's lens model.  Parity of exactly this call: tests/test_gpu_tum.py.  One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIG = "tum1_640x480_5mm"
DEPTH_FACTOR = 5000.0
D_TUM1 = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)  # Camera.k1 k2 p1 p2 k3, settings/TUM1.yaml:32-36


def tum_frames(n_frames, start=0):
    """(stream, depth u16 [n,H,W], rgb u8 [n,H,W,3], T_cw [n,4,4]) rendered through the lens model, cached under /tmp."""
    from pyslam_amd.synthetic import SyntheticRGBD

    from bench import frame_cache_path

    s = SyntheticRGBD(CONFIG, distorted=True, depth_dtype="uint16", depth_map_factor=DEPTH_FACTOR)
    cache = frame_cache_path(f"{CONFIG}_distorted_u16_{start}_{n_frames}")
    if not os.path.exists(cache):
        depth, rgb, T = s.batch(start, n_frames)
        try:
            tmp = f"{cache}.{os.getpid()}.tmp.npz"
            np.savez(tmp, depth=depth, rgb=rgb, T=T)
            os.replace(tmp, cache)
        except OSError:
            return s, depth, rgb, T
    try:
        z = np.load(cache)
        return s, z["depth"], z["rgb"], z["T"]
    except Exception:  # unreadable (another user's file) or damaged: render the same frames here
        return (s,) + tuple(s.batch(start, n_frames))


def rectification(s):
    from pyslam_amd import prep

    K = np.array([[s.fx, 0.0, s.cx], [0.0, s.fy, s.cy], [0.0, 0.0, 1.0]])
    new_K = prep.get_optimal_new_camera_matrix(K, s.dist, (s.width, s.height), 0.7, (s.width, s.height))[0]
    mx, my = prep.init_undistort_rectify_map(K, s.dist, new_K, (s.width, s.height))
    return mx, my, (float(new_K[0, 0]), float(new_K[1, 1]), float(new_K[0, 2]), float(new_K[1, 2]))


def write_tum_folder(root, name, s, depth, rgb, T):
    """<root>/<name>/{rgb/*.png, depth/*.png uint16, associations.txt, groundtruth.txt} (pyslam/io/dataset.py:576-643)."""
    from scipy.spatial.transform import Rotation

    from pyslam_amd.io.images import imwrite

    base = os.path.join(root, name)
    os.makedirs(os.path.join(base, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(base, "depth"), exist_ok=True)
    assoc, gt = [], ["# ground truth trajectory", "# file: synthetic", "# timestamp tx ty tz qx qy qz qw"]
    for i in range(len(T)):
        t = 1000.0 + i / 30.0
        imwrite(os.path.join(base, "rgb", f"{t:.6f}.png"), np.ascontiguousarray(rgb[i][..., ::-1]))
        imwrite(os.path.join(base, "depth", f"{t:.6f}.png"), depth[i])
        assoc.append(f"{t:.6f} rgb/{t:.6f}.png {t:.6f} depth/{t:.6f}.png")
        Twc = np.linalg.inv(T[i])
        q = Rotation.from_matrix(Twc[:3, :3]).as_quat()
        gt.append(f"{t + 0.001:.6f} {Twc[0, 3]:.9f} {Twc[1, 3]:.9f} {Twc[2, 3]:.9f} {q[0]:.9f} {q[1]:.9f} {q[2]:.9f} {q[3]:.9f}")
    open(os.path.join(base, "associations.txt"), "w").write("\n".join(assoc) + "\n")
    open(os.path.join(base, "groundtruth.txt"), "w").write("\n".join(gt) + "\n")
    return base


def tum_leg(n_frames=192, B=32, mesh_every=64, cli_frames=48, cli=True, h2d_gbs=None):
    import torch

    from pyslam_amd.volumetric import PinholeCameraIntrinsic, ScalableTSDFVolume
    from tools.bench_host import h2d_rate_gbs

    s, depth_h, rgb_h, T_h = tum_frames(n_frames)
    mx, my, intr = rectification(s)
    K = PinholeCameraIntrinsic(s.width, s.height, *intr)
    steps = n_frames // B
    # one allocation per keyframe, pageable: what arrives through pySLAM's queue (uint16 depth: the sensor's own format)
    depths = [np.array(depth_h[i]) for i in range(n_frames)]
    colors = [np.array(rgb_h[i]) for i in range(n_frames)]
    frame_bytes = depths[0].nbytes + colors[0].nbytes
    rate = h2d_gbs or h2d_rate_gbs()
    vol = ScalableTSDFVolume(0.005, 0.04, max_blocks=1 << 17, max_points=s.width * s.height)
    vol.set_rectify_maps(mx, my)

    def run(mesh, dtype=None):
        vol.reset()
        vol.synchronize()
        tri = 0
        t0 = time.perf_counter()
        for k in range(steps):
            lo = k * B
            vol.integrate_frames(depths[lo:lo + B], colors[lo:lo + B], K, T_h[lo:lo + B], depth_scale=DEPTH_FACTOR, depth_trunc=4.0)
            if mesh and mesh_every and (lo + B) % mesh_every == 0:
                tri = len(vol.extract_triangle_mesh(dtype=dtype).triangles)
        vol.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, tri

    run(True)  # warm-up: units allocated, staging slots page-locked, copy threads started, result arrays page-locked
    t_fuse = min(run(False)[0] for _ in range(3))
    t_all, tri = min(run(True) for _ in range(2))
    run(True, np.float32)  # (page-locks the float32 result arrays)
    t_all_f32 = min(run(True, np.float32)[0] for _ in range(2))
    fps, fps_mesh = steps * B / t_fuse, steps * B / t_all
    out = {"metric": "RGB-D frames/sec fused (TUM-fr1 shape: 640x480, TUM1 intrinsics + distortion, uint16 depth / 5000, 5 mm TSDF)",
           "config": "BASELINE.json configs[0] shape on synthetic frames rendered through TUM1's lens model (no TUM data in the image)",
           "value": round(fps_mesh, 1), "unit": "frames/s", "frames": steps * B, "frames_per_call": B,
           "what": f"pageable uint16 depth + uint8 colour keyframes -> integrate_frames (pipelined H2D staging) -> rectify on the device "
                   f"(one launch per batch) -> multi-frame sweep -> extract_triangle_mesh every {mesh_every} frames (host-visible result), "
                   f"volume empty when the clock starts",
           "fuse_only": {"value": round(fps, 1), "unit": "frames/s"},
           "with_float32_mesh": {"value": round(steps * B / t_all_f32, 1), "unit": "frames/s",
                                 "what": "the same clock with extract_triangle_mesh(dtype=np.float32): vertices / colours rounded to float32 on the "
                                         "device (opt-in; the value above hands over Open3D's float64 arrays)"},
           "triangles_last": int(tri), "units": int(vol.num_blocks()),
           "bytes_per_frame": int(frame_bytes), "h2d_pinned_GBs": round(rate, 1),
           "roofline": {"bound": "pcie", "algorithmic_bytes_per_frame": int(frame_bytes),
                        "what": "5 B / pixel cross PCIe once (uint16 depth + uint8 x 3 colour); everything behind it runs beside the copy",
                        "achieved": round(frame_bytes * fps / 1e9, 2), "peak": round(rate, 1), "unit": "GB/s",
                        "frac": round(frame_bytes * fps / 1e9 / rate, 3), "peak_what": "pinned-memory H2D rate measured in this process",
                        "h2d_bound_frames_per_s": round(rate * 1e9 / frame_bytes, 1), "traffic": None},
           "parity": "tests/test_gpu_tum.py (this call against oracle.PortTsdf on frames rectified by oracle/host_prep.py); TSDF and remap "
                     "semantics are restatements of Open3D / OpenCV: parity unpinned"}
    del vol
    if not cli:
        return out
    try:
        out["dense_reconstruction_cli"] = cli_leg(s, depth_h[:cli_frames], rgb_h[:cli_frames], T_h[:cli_frames])
    except Exception as e:  # the worker process is the fragile part of a benchmark box: never lose the line for it
        out["dense_reconstruction_cli"] = {"error": f"{type(e).__name__}: {e}"}
    return out


def cli_leg(s, depth, rgb, T):
    """The same stream as a TUM folder through pyslam_amd/tools/dense_reconstruction.py (the drop-in for
    main_map_dense_reconstruction.py:73-222): TumDataset reads the pngs, Frame's depth conversion (uint16 * 1/5000 -> float32),
    the integrator front with a distorted camera (maps handed to the volume), mesh, dense_map.ply."""
    import tempfile
    import types

    from pyslam_amd.dense.parameters import get_parameters
    from pyslam_amd.io.datasets import dataset_factory
    from pyslam_amd.tools import dense_reconstruction

    P = get_parameters()
    P.kVolumetricIntegrationTSdfTrunc = 0.04
    P.kVolumetricIntegrationHipMaxBlocks = 1 << 16
    P.kVolumetricIntegrationFpsThrottleEnabled = False
    cam = types.SimpleNamespace(fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, width=s.width, height=s.height, D=np.array(D_TUM1),
                                depth_factor=1.0 / DEPTH_FACTOR, bf=40.0, fps=30)
    with tempfile.TemporaryDirectory(prefix="pyslam_amd_tum_") as root:
        t0 = time.perf_counter()
        write_tum_folder(root, "rgbd_dataset_synthetic_fr1", s, depth, rgb, T)
        t_write = time.perf_counter() - t0
        ds = dataset_factory("tum", root, "rgbd_dataset_synthetic_fr1", cam)
        t0 = time.perf_counter()
        kfs = list(ds.keyframes())
        t_read = time.perf_counter() - t0
        out_dir = os.path.join(root, "out")
        log = []
        t0 = time.perf_counter()
        n = dense_reconstruction.run(iter(kfs), cam, ds.environment_type, ds.sensor_type, "TSDF", out_dir, voxel_length=0.005, log=log.append)
        dt = time.perf_counter() - t0
        ply = os.path.join(out_dir, "dense_map.ply")
        size = os.path.getsize(ply) if os.path.exists(ply) else 0
    return {"value": round(n / dt, 1), "unit": "frames/s", "frames": int(n), "total_s": round(dt, 3),
            "png_decode_s": round(t_read, 3), "png_encode_s": round(t_write, 3), "dense_map_ply_bytes": int(size),
            "what": "dense_reconstruction.run(): worker start-up, add_keyframe x N (float32 metric depth as pySLAM's Frame makes it), "
                    "rectify on the device, fuse, final mesh, save dense_map.ply - all inside the clock (png decode outside: png_decode_s)"}


if __name__ == "__main__":
    print(json.dumps(tum_leg(cli="--no-cli" not in sys.argv)))
