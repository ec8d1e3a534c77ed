"""CPU: the C restatement against the live compiled reference (oracle/_ref, built from the reference
sources by oracle/Makefile) on larger seeded inputs than the golden fixtures."""
import os

import numpy as np
import pytest

import oracle
from oracle import host_prep as hp

pytestmark = pytest.mark.skipif(not oracle.ref_available(), reason="compiled reference not available")


def test_keys_random_and_adversarial():
    from tools.make_golden import golden_points

    for voxel in (0.005, 0.004, 0.002, 0.015, 0.05):
        pts, _ = golden_points(3, 100_000, voxel)
        for a, b in zip(oracle.keys(pts, voxel, 8, "port"), oracle.keys(pts, voxel, 8, "ref")):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("bs", [4, 8, 16])
def test_integrate_stream_bit_exact(bs):
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD("tiny_160x120_2cm")
    port, ref = oracle.PortGrid(0.02, bs), oracle.RefGrid(0.02, bs)
    for i in range(3):
        depth, rgb, T = s[i]
        p, c, _ = hp.frame_to_world_f32(depth, rgb, *s.intrinsics, T, 4.0)
        for g in (port, ref):
            g.integrate(p, c if i != 1 else (c * 255).astype(np.uint8))
    for a, b in zip(port.dump(), ref.dump()):
        np.testing.assert_array_equal(a, b)
    assert port.size() == ref.size() and port.num_blocks() == ref.num_blocks()
    port.remove_low_count_voxels(2)
    ref.remove_low_count_voxels(2)
    for a, b in zip(port.dump(), ref.dump()):
        np.testing.assert_array_equal(a, b)
    port.clear()
    ref.clear()
    assert port.empty() and ref.empty()


def test_frustum_contains():
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD("tiny_160x120_2cm")
    intr = np.array(s.intrinsics, np.float32)
    rng = np.random.default_rng(0)
    for f in range(3):
        T = s.pose(f * 17)
        for p in (rng.random((300, 3)) * np.array([6, 4, 3])).astype(np.float32):
            a = oracle.frustum_contains(intr, s.width, s.height, T, 8.0, 0.01, p, "port")
            b = oracle.frustum_contains(intr, s.width, s.height, T, 8.0, 0.01, p, "ref")
            assert a[0] == b[0]
            np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(oracle.frustum_bbox(intr, s.width, s.height, T, 8.0, 0.01, "port"),
                                      oracle.frustum_bbox(intr, s.width, s.height, T, 8.0, 0.01, "ref"))


@pytest.mark.skipif(not oracle.ref_available(), reason="compiled reference not available")
def test_reference_double_overload_keys_in_double():
    """Pins what `integrate(points float64)` means in the reference (volumetric_grid_module.h:738-741 ->
    integrate_raw<double, ...>): the voxel index is floor(x * (double)inv_voxel_size_f32) in DOUBLE, the voxel sums take
    static_cast<float>(x).  Checked on points whose float32 narrowing lands in the neighbouring cell; the GPU path is held to
    the same compiled reference in tests/test_gpu_voxel_grid.py::test_float64_points_take_the_double_overload."""
    rng = np.random.default_rng(5)
    vs = float(np.float32(0.005))
    inv = float(np.float32(1.0) / np.float32(0.005))
    k = rng.integers(-4000, 4000, size=(20000, 3)).astype(np.float64)
    pts = np.concatenate([k * vs * (1.0 - 1e-12), k * vs * (1.0 + 1e-12), (rng.random((20000, 3)) - 0.5) * 40.0])
    g = oracle.RefGrid(0.005, 8)
    g.integrate(pts)
    keys, _, counts, sums = g.dump()
    # restatement: voxel index in double, block = floor_div(v, 8), local = v - 8 block, linear x + 8 y + 64 z
    v = np.floor(pts * inv).astype(np.int64)
    b = v >> 3
    lin = (v - 8 * b) @ np.array([1, 8, 64])
    order = {tuple(key): i for i, key in enumerate(keys)}
    want = np.zeros_like(counts)
    pos = np.zeros(counts.shape + (3,), np.float32)
    for row, (bk, l) in enumerate(zip(map(tuple, b), lin)):  # sequential float32 accumulation, point order
        i = order[bk]
        want[i, l] += 1
        pos[i, l] += pts[row].astype(np.float32)
    np.testing.assert_array_equal(counts, want)
    np.testing.assert_array_equal(sums[..., :3].view(np.uint32), pos.view(np.uint32))
    g32 = oracle.RefGrid(0.005, 8)
    g32.integrate(pts.astype(np.float32))
    assert g32.dump()[0].shape != keys.shape or not np.array_equal(g32.dump()[2], counts)  # and NOT the float overload's result


def test_optimised_reference_build_against_the_portable_oracle_build():
    """The oracle is the reference compiled WITHOUT -march=native and with -ffp-contract=off (it has to give the same bits
    on any host).  The reference's own CMake flags are -O3 -march=native with GCC's default contraction.  That variant's outputs
    (oracle/Makefile ref_native, built and recorded on the dev host by tools/make_golden_ref_native.py; never shipped, never the
    oracle) are in tests/golden/ref_native_tiny.npz, stored as a patch on the portable build's outputs (decode() first checks that the
    live portable build still gives exactly the bits they were recorded against); this test measures the gap to the portable build:
      * VoxelBlockGrid (pySLAM's default grid): keys and counts identical, position / colour sums within 1e-5 relative
        (bit-identical on the AVX2 + FMA host this was written on);
      * volumetric::VoxelGrid (direct hash, V16): with AVX2 the reference switches to a SIMD branch that sums four points per
        step (voxel_grid.h:42-46, voxel_grid_simd.hpp) - same voxels, positions within 2e-6 m, colours within 1e-6, under
        2 % of the values differ at all: two orders of magnitude inside the north star's 1e-4.
    The GPU path is bit-identical to the portable build (tests/test_gpu_voxel_grid.py)."""
    from tools.make_golden_ref_native import clouds, decode, reference_outputs

    oracle.ref_lib()  # builds the portable variant if needed
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    port = reference_outputs(os.path.join(here, "_ref", "libref_volumetric.so"), clouds())
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_native_tiny.npz"))
    native = decode(z, port)
    for kind in (2, 1):
        ka, ca, sa = (port[f"block{kind}_{x}"] for x in ("keys", "counts", "sums"))
        kb, cb, sb = (native[f"block{kind}_{x}"] for x in ("keys", "counts", "sums"))
        np.testing.assert_array_equal(ka, kb)
        np.testing.assert_array_equal(ca, cb)
        np.testing.assert_allclose(sa, sb, rtol=1e-5, atol=1e-6)
    (pa, ca), (pb, cb) = (port["direct_points"], port["direct_colors"]), (native["direct_points"], native["direct_colors"])
    assert pa.shape == pb.shape and len(pa) > 10_000
    assert float(np.abs(pa - pb).max()) <= 2e-6 and float(np.abs(ca - cb).max()) <= 1e-6
    if bool(z["avx2"]):
        assert float((pa.view(np.uint32) != pb.view(np.uint32)).mean()) < 0.02


def test_openmp_two_phase_restatement_is_bit_identical_to_the_sequential_branch():
    """oracle.PortGrid.integrate_parallel (the reference's TBB branch, voxel_block_grid.hpp:292-456, restated with OpenMP for the
    all-cores CPU baseline) against the sequential restatement - which the tests above pin to the compiled reference."""
    import oracle
    from oracle import host_prep as hp
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD("tiny_160x120_2cm")
    a, b = oracle.PortGrid(0.02, 8), oracle.PortGrid(0.02, 8)
    for i, th in ((0, 1), (5, 3), (9, 8), (5, 16)):
        d, c, T = s[i]
        p, col, _ = hp.frame_to_world_f32(d, c, *s.intrinsics, T, 4.0)
        cols = (col * 255).astype(np.uint8) if i == 9 else col
        a.integrate(p, cols)
        b.integrate_parallel(p, cols, threads=th)
    assert a.num_blocks() == b.num_blocks() > 100
    for x, y in zip(a.dump(), b.dump()):
        np.testing.assert_array_equal(x, y)
