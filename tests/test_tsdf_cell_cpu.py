"""pyslam_amd/csrc/hv_tsdf_cell.h on the host, bit for bit against the numpy restatements - no GPU, no library.

The header's arithmetic part (cell rule, corner order, trilinear value and gradient) is what every map query of the library compiles;
tests/tsdf_cell_host.cpp includes it without HIP.  The driver is built with the oracle build's compiler and -ffp-contract=off, fed
seeded points and eight-value sets plus the edge cases of the cell rule, and its output is compared for equality of bit patterns with
tests/sample_reference.py (locate, _tri) and with the float formula of tests/raycast_reference.py.  A second build of the same driver
runs once as a plain executable under the address and undefined-behaviour sanitizers.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import raycast_reference as rr
from tests import sample_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyslam_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "tsdf_cell_host.cpp")
N_SEEDED = 4096
VL_EXACT = 2.0 ** -7  # p / VL_EXACT is exact: the edge cases below land on the lattice values they name

IN = np.dtype([("p", "<f8", 3), ("vl", "<f8"), ("f", "<f8", 8), ("rf", "<f4", 3), ("ff", "<f4", 8), ("pad", "<f4")])
OUT = np.dtype([("g0", "<i4", 3), ("ok", "<i4"), ("r", "<f8", 3), ("phi", "<f8"), ("phi_grad", "<f8"), ("e", "<f8", 3), ("lerp_f", "<f4"),
                ("pad", "<f4")])


def _edge_points():
    """Points of the cell rule's edges at VL_EXACT, as lattice coordinates g = p / vl - 0.5 per axis."""
    below = np.nextafter(1.0e9, 0.0)
    g = []
    for k in (-3.0, -1.0, 0.0, 1.0, 16.0, 2.0 ** 30 / 2):  # exact integers: r = 0
        g.append((k, k + 1.0, -k))
    for k in (-2.0, 0.0, 7.0):  # exact halves: r = 0.5, the nearest voxel flips
        g.append((k + 0.5, k - 0.5, k + 0.5))
    g.append((below, 0.25, -below))  # the last representable cells
    g.append((-below, below, 0.75))
    for a in range(3):  # |g| = 1e9, infinity and NaN in one axis: the axes after it take g0 = 0 as well
        for bad in (1.0e9, -1.0e9, np.inf, -np.inf, np.nan):
            row = [3.25, -4.5, 5.75]
            row[a] = bad
            g.append(tuple(row))
    p = (np.asarray(g, np.float64) + 0.5) * VL_EXACT
    zeros = np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0]])  # negative zero as a coordinate
    return np.concatenate([p, zeros])


def _inputs():
    rng = np.random.default_rng(20240607)
    edge = _edge_points()
    n = N_SEEDED + len(edge)
    rec = np.zeros(n, IN)
    rec["p"][:N_SEEDED] = rng.uniform(-3.0, 3.0, (N_SEEDED, 3))
    rec["vl"][:N_SEEDED] = rng.choice([0.004, 0.01, 0.0123, VL_EXACT], N_SEEDED)
    rec["p"][N_SEEDED:] = edge
    rec["vl"][N_SEEDED:] = VL_EXACT
    rec["f"] = rng.uniform(-1.0, 1.0, (n, 8))
    rec["f"][::7] = rng.integers(0, 256, (len(rec[::7]), 8))  # colour means too
    rec["f"][::11] = np.round(rec["f"][::11])  # and the band's ends -1, 0, 1
    rec["rf"] = rng.random((n, 3), np.float32)
    rec["ff"] = rng.uniform(-1.0, 1.0, (n, 8)).astype(np.float32)
    rec["rf"][:4] = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0, 1], [0, 1, 0.5]], np.float32)
    return rec


SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _cxx():
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ not found: the oracle build (oracle/Makefile) needs it as well"
    return cxx


def _build(tmp, name, extra):
    exe = os.path.join(tmp, name)
    cmd = [_cxx(), "-std=c++17", "-O3", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, DRIVER, "-o", exe] + extra
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    return exe


def _has_sanitizer_runtimes(tmp):
    """Does this compiler link and run a trivial program under the sanitizers at all?  (Decided on that program, never on the driver.)"""
    src, exe = os.path.join(tmp, "probe.cpp"), os.path.join(tmp, "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    if subprocess.run([_cxx(), src, "-o", exe] + SANITIZE, capture_output=True).returncode != 0:
        return False
    return subprocess.run([exe], capture_output=True).returncode == 0


def _run(exe, tmp, rec):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, os.path.basename(exe) + ".out")
    with open(src, "wb") as f:
        f.write(np.int64(len(rec)).tobytes())
        f.write(rec.tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    raw = open(dst, "rb").read()
    assert len(raw) == len(rec) * OUT.itemsize + 8 * 3 * 4
    return np.frombuffer(raw[:len(rec) * OUT.itemsize], OUT), np.frombuffer(raw[len(rec) * OUT.itemsize:], "<i4").reshape(8, 3)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("tsdf_cell"))
    rec = _inputs()
    out, corners = _run(_build(tmp, "cell_host", []), tmp, rec)
    return tmp, rec, out, corners


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)


def test_the_header_compiles_without_hip_and_names_the_corner_order(case):
    _, _, _, corners = case
    assert [tuple(c) for c in corners] == [(sx, sy, sz) for _i, sx, sy, sz in rr._corners()]


def test_locate_matches_the_restatement_bit_for_bit(case):
    _, rec, out, _ = case
    with np.errstate(invalid="ignore", over="ignore"):
        ok_ref = np.zeros(len(rec), bool)
        g0_ref = np.zeros((len(rec), 3), np.int64)
        r_ref = np.zeros((len(rec), 3), np.float64)
        for vl in np.unique(rec["vl"]):  # (the restatement takes one voxel length per call)
            m = rec["vl"] == vl
            ok, g0, r = sr.locate(rec["p"][m], vl)
            ok_ref[m] = ok
            g0_ref[m] = np.stack(g0, axis=-1)
            r_ref[m] = np.stack(r, axis=-1)
    assert np.array_equal(out["ok"] != 0, ok_ref)
    assert np.array_equal(out["g0"].astype(np.int64), g0_ref)  # refused points included: 0 from the first refused axis on
    assert np.array_equal(_bits(out["r"][ok_ref]), _bits(r_ref[ok_ref]))
    # the edge cases did what they are there for
    edge = slice(N_SEEDED, None)
    assert (~ok_ref[edge]).sum() == 15 and ok_ref[:N_SEEDED].all()
    assert (out["r"][edge][ok_ref[edge]] == 0.0).any() and (out["r"][edge][ok_ref[edge]] == 0.5).any()
    assert out["g0"][edge].max() == 999999999 and out["g0"][edge].min() == -1000000000
    refused = out["g0"][edge][~ok_ref[edge]]
    assert (refused[:, 0] != 0).any() and (refused[:, 2] == 0).all()  # an axis before the bad one keeps its g0, none after it


def test_trilinear_value_and_gradient_match_the_restatement_bit_for_bit(case):
    _, rec, out, _ = case
    r = np.where((out["ok"] != 0)[:, None], out["r"], 0.0)
    phi, e = sr._tri([r[:, a] for a in range(3)], [rec["f"][:, c] for c in range(8)])
    assert np.array_equal(_bits(out["phi"]), _bits(phi))
    assert np.array_equal(_bits(out["phi_grad"]), _bits(phi))
    assert np.array_equal(_bits(out["e"]), _bits(np.stack(e, axis=-1)))
    assert np.abs(out["e"]).max() > 1.0  # (not a comparison of zeros)


def test_float_lerp_matches_the_ray_cast_restatement_bit_for_bit(case):
    _, rec, out, _ = case
    ref = rr._lerp([rec["rf"][:, a] for a in range(3)], [rec["ff"][:, c] for c in range(8)])
    assert ref.dtype == np.float32
    assert np.array_equal(_bits(out["lerp_f"]), _bits(ref))


def test_the_driver_is_clean_under_address_and_undefined_behaviour_sanitizers(case):
    """The same driver as a plain executable built with the sanitizers (never loaded into Python): it ends clean on the same input,
    NaN, infinity and the refused cells included, and writes the same bytes."""
    tmp, rec, out, _ = case
    if not _has_sanitizer_runtimes(tmp):
        pytest.skip("this machine's g++ cannot link an empty program with -fsanitize=address,undefined (no sanitizer runtimes)")
    again, _ = _run(_build(tmp, "cell_host_san", SANITIZE), tmp, rec)
    assert again.tobytes() == out.tobytes()
