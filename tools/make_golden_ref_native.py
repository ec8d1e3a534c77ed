#!/usr/bin/env python3
"""Generate tests/golden/ref_native_tiny.npz: the outputs of the reference compiled with its OWN optimisation flags
(oracle/Makefile ref_native: -O3 -march=native, GCC's default -ffp-contract=fast) on six frames of tiny_160x120_2cm, for
tests/test_oracle_vs_reference.py::test_optimised_reference_build_against_the_portable_oracle_build, which measures them against
the portable build the oracle is.  Needs the reference sources (dev container only); the recording host's AVX2 flag is stored
with the outputs, since with AVX2 the reference's direct voxel hash takes its SIMD branch.

The two builds differ in a few hundred values out of a few million, so the native outputs are stored exactly but compactly, as a
patch on the portable build's outputs: per array the SHA-256 of the portable bits it was recorded against, and the flat indices
and native values where the bits differ (encode / decode)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_native_tiny.npz")


def cpu_has_avx2():
    try:
        return "avx2" in open("/proc/cpuinfo").read()
    except OSError:
        return False


def clouds():
    """Six frames of tiny_160x120_2cm as float32 world points with float32 and uint8 colours."""
    sys.path.insert(0, ROOT)
    from oracle import host_prep as hp
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD("tiny_160x120_2cm")
    out = []
    for i in range(6):
        d, c, T = s[i]
        pts, cols, _ = hp.frame_to_world_f32(d, c, *s.intrinsics, T, 4.0)
        pts, cols = np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(cols, np.float32)
        out.append((pts, cols, np.ascontiguousarray(np.clip(np.rint(cols * (255.0 if cols.max() <= 1.0 else 1.0)), 0, 255).astype(np.uint8))))
    return out


def reference_outputs(lib_path, frames):
    """-> {"block<kind>_keys" / "_counts" / "_sums": the default VoxelBlockGrid (0.02 m, 8^3 blocks) fed float32 (kind 2) and
    uint8 (kind 1) colours, "direct_points" / "direct_colors": volumetric::VoxelGrid (direct hash) voxels sorted by voxel key}."""
    vp, i64, i32, f32, f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_double
    L = C.CDLL(lib_path)
    L.ref_grid_create.restype = vp
    L.ref_grid_create.argtypes = [f32, i32]
    L.ref_grid_destroy.argtypes = [vp]
    L.ref_grid_integrate.argtypes = [vp, vp, i64, vp, i32]
    L.ref_grid_num_blocks.restype = i64
    L.ref_grid_num_blocks.argtypes = [vp]
    L.ref_grid_dump.restype = i64
    L.ref_grid_dump.argtypes = [vp, vp, vp, vp, vp]
    out = {}
    for kind in (2, 1):
        h = L.ref_grid_create(0.02, 8)
        for pts, cols, cols8 in frames:
            cc = cols if kind == 2 else cols8
            L.ref_grid_integrate(h, pts.ctypes.data_as(vp), len(pts), cc.ctypes.data_as(vp), kind)
        nb = L.ref_grid_num_blocks(h)
        keys, hs = np.zeros((nb, 3), np.int32), np.zeros(nb, np.uint64)
        cnt, sums = np.zeros((nb, 512), np.int32), np.zeros((nb, 512, 6), np.float32)
        L.ref_grid_dump(h, keys.ctypes.data_as(vp), hs.ctypes.data_as(vp), cnt.ctypes.data_as(vp), sums.ctypes.data_as(vp))
        L.ref_grid_destroy(h)
        out[f"block{kind}_keys"], out[f"block{kind}_counts"], out[f"block{kind}_sums"] = keys, cnt, sums
    L.ref_vgrid_create.restype = vp
    L.ref_vgrid_create.argtypes = [f64]
    L.ref_vgrid_destroy.argtypes = [vp]
    L.ref_vgrid_integrate.argtypes = [vp, vp, i64, vp, i32]
    L.ref_vgrid_get_voxels.restype = i64
    L.ref_vgrid_get_voxels.argtypes = [vp, i32, f32, vp, vp, i64]
    h = L.ref_vgrid_create(0.02)
    for pts, cols, _ in frames:
        L.ref_vgrid_integrate(h, pts.ctypes.data_as(vp), len(pts), cols.ctypes.data_as(vp), 2)
    n = L.ref_vgrid_get_voxels(h, 1, 0.0, None, None, 0)
    P, Cc = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    L.ref_vgrid_get_voxels(h, 1, 0.0, P.ctypes.data_as(vp), Cc.ctypes.data_as(vp), n)
    L.ref_vgrid_destroy(h)
    order = np.lexsort(np.floor(P / 0.02).astype(np.int64).T[::-1])
    out["direct_points"], out["direct_colors"] = P[order], Cc[order]
    return out


def _digest(a):
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + np.ascontiguousarray(a).tobytes()).hexdigest()


def encode(native, portable):
    """-> per array <name>_base_sha256, <name>_diff_index, <name>_diff_value: native = portable with the values at the indices replaced."""
    out = {}
    for k, b in native.items():
        a = portable[k]
        if a.shape != b.shape or a.dtype != b.dtype:
            raise SystemExit(f"{k}: native {b.dtype}{b.shape} vs portable {a.dtype}{a.shape} - not expressible as a patch")
        bits = np.dtype(f"u{a.dtype.itemsize}")
        idx = np.flatnonzero(a.ravel().view(bits) != b.ravel().view(bits))
        out[k + "_base_sha256"] = np.array(_digest(a))
        out[k + "_diff_index"] = idx.astype(np.int64)
        out[k + "_diff_value"] = b.ravel()[idx]
    return out


def decode(z, portable):
    """The native outputs from the stored patch and the live portable build's outputs, which must be the bits it was recorded against."""
    native = {}
    for k, a in portable.items():
        if _digest(a) != str(z[k + "_base_sha256"]):
            raise AssertionError(f"{k}: the portable build no longer gives the outputs the native ones were recorded against")
        b = a.copy().ravel()
        b[z[k + "_diff_index"]] = z[k + "_diff_value"]
        native[k] = b.reshape(a.shape)
    return native


def main():
    subprocess.check_call(["make", "-s", "-C", ORACLE, "-f", os.path.join(ORACLE, "Makefile"), "ref", "ref_native"])
    frames = clouds()
    native = reference_outputs(os.path.join(ORACLE, "_ref", "libref_volumetric_native.so"), frames)
    portable = reference_outputs(os.path.join(ORACLE, "_ref", "libref_volumetric.so"), frames)
    np.savez_compressed(GOLDEN, avx2=cpu_has_avx2(), **encode(native, portable))
    print("wrote", GOLDEN, {k: int((native[k] != portable[k]).sum()) for k in native}, "values differ")


if __name__ == "__main__":
    main()
