"""CPU: the map-to-map registration contract (include/hipvol.h, hv_tsdf_register_volume) as tests/register_reference.py restates
it, on the planted scenes of tests/register_scenes.py (a 3 x 3 x 3 unit cluster, voxel 0.02, sdf_trunc 0.08), and the entry point's
presence in the library and the binding.  No GPU.

What the restatement reaches is RECORDED here, because it is the bar of the GPU tests (tests/test_gpu_tsdf_register.py holds the
library to twice these figures): they are the discretisation error of two samplings of one analytic field on lattices that do not
coincide, not a property of any kernel.
"""
import ctypes

import numpy as np
import pytest

from tests import merge_reference as mr
from tests import planted_states as ps
from tests import raycast_reference as rr
from tests import register_reference as rg
from tests import register_scenes as sc
from tests.test_merge_reference_cpu import CAST_POSES, rigid, rigid_inverse

# Recorded from test_restatement_recovers_the_ground_truth and test_merge_after_registration_against_the_ground_truth when they
# were written: the pose error the restatement ends at from INIT (1 voxel, 1 degree off), and the mean |dz| between casts of the
# destination merged with the registered and with the true transform.
RECORDED_TRANSLATION_ERROR = 1.110e-4  # metres, at the cluster's centre (0.0055 voxel)
RECORDED_ROTATION_ERROR = 3.185e-3     # degrees
RECORDED_MERGE_DZ = 0.01006            # voxels, mean over the commonly hit pixels of the four casts
PRM = rg.params(sc.VOX, sc.TRUNC)


@pytest.fixture(scope="module")
def pair():
    """(dst dump, src dump) of the corner-and-sphere pair; shared, nothing of it may be written to."""
    return ps.as_dump(sc.corner_and_sphere(frame=sc.T_TRUE)), ps.as_dump(sc.corner_and_sphere())


@pytest.fixture(scope="module")
def registered(pair):
    return rg.register_reference(pair[0], pair[1], sc.INIT, PRM, 30)


def cast_poses():
    """CAST_POSES carried into the destination's frame."""
    return [P @ rigid_inverse(sc.T_TRUE) for P in CAST_POSES]


def casts_of(dump):
    return [rr.ray_cast(dump, sc.VOX, sc.TRUNC, sc.cast_intrinsics(), P, sc.CAST_H, sc.CAST_W, 0.1, 3.0, 3.0, render_attributes=("depth", "mask"))
            for P in cast_poses()]


def test_register_volume_is_bound_and_exported():
    from pyslam_amd import _lib, build
    from pyslam_amd.volumetric import RegistrationResult, ScalableTSDFVolume

    assert "hv_tsdf_register_volume" in _lib.SIGNATURES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "hv_tsdf_register_volume")
    assert callable(ScalableTSDFVolume.register_volume)
    assert ctypes.sizeof(_lib.HvRegisterParams) == 4 * 8 + 2 * 4 and ctypes.sizeof(_lib.HvRegisterResult) == (16 + 36 + 3 + 2) * 8 + 2 * 8 + 2 * 4
    r = RegistrationResult(np.eye(4), 0.5, 0.001, np.eye(6), True, 3, 10, 20, np.zeros(3))
    assert r.success and r.iterations == 3 and r.trace is None and "fitness=0.5000" in repr(r)
    text = open(build.INCLUDE + "/hipvol.h").read()
    for name, value in (("MIN_INLIERS", rg.MIN_INLIERS), ("PIVOT_REL", rg.PIVOT_REL), ("CONVERGED", rg.CONVERGED), ("TRACE_STRIDE", rg.TRACE_STRIDE)):
        line = [l for l in text.splitlines() if l.startswith(f"#define HV_REGISTER_{name} ")]
        assert len(line) == 1 and float(line[0].split()[2]) == value, name
    assert _lib.HV_REGISTER_TRACE_STRIDE == rg.TRACE_STRIDE == 5 + 16 + 21 + 6 + 6


def test_restatement_recovers_the_ground_truth(registered):
    """From INIT = T_TRUE perturbed by (1 voxel, 1 degree about the cluster's centre) the restatement converges (status 1) in 4
    linearisations over 22 085 candidates (19 023 inliers at the end, fitness 0.861, inlier rmse 0.43 mm) and ends 1.110e-4 m
    (0.0055 voxel) and 3.185e-3 degrees from T_TRUE; the first step alone takes the error from (20 mm, 1 deg) to (0.09 mm,
    0.018 deg).  These figures, times 2, are the bars of tests/test_gpu_tsdf_register.py::test_ground_truth."""
    out = registered
    t_err, r_err = sc.pose_error(out["transformation"], sc.T_TRUE)
    t0, r0 = sc.pose_error(sc.INIT, sc.T_TRUE)
    print(f"init {t0:.6g} m {r0:.6g} deg -> {t_err:.6g} m {r_err:.6g} deg in {out['iterations']} linearisations; candidates {out['candidates']}, "
          f"inliers {out['inliers']}, fitness {out['fitness']:.4f}, rmse {out['inlier_rmse']:.3g}")
    assert abs(t0 - sc.VOX) < 1e-12 and abs(r0 - 1.0) < 1e-9
    assert out["success"] and out["trace"][-1]["status"] == 1 and 2 <= out["iterations"] <= 8
    # the record is what the restatement gives (1 % for a numpy whose sums associate otherwise)
    assert abs(t_err - RECORDED_TRANSLATION_ERROR) <= 0.01 * RECORDED_TRANSLATION_ERROR
    assert abs(r_err - RECORDED_ROTATION_ERROR) <= 0.01 * RECORDED_ROTATION_ERROR
    assert out["candidates"] > 20000 and out["fitness"] > 0.8 and out["inlier_rmse"] < 1e-3
    # every row: H xi = -g, and the next row starts from exp(xi) A
    rows = out["trace"]
    for a, b in zip(rows, rows[1:]):
        assert np.linalg.norm(a["H"] @ a["xi"] + a["g"]) <= 1e-12 * (np.linalg.norm(a["H"]) * np.linalg.norm(a["xi"]) + np.linalg.norm(a["g"]))
        assert np.abs(b["A"] - rg.exp_se3(a["xi"]) @ a["A"]).max() <= 1e-14
    # H is well conditioned about the anchor: all six motions are fixed
    ev = np.linalg.eigvalsh(out["information"])
    assert ev[0] > 1e-3 * ev[-1], ev


def test_no_fragile_voxels_at_the_first_linearisation(pair):
    """The transforms the GPU tests compare counts at put no candidate within 1e-9 of a boundary of the rules."""
    dst, src = pair
    assert rg.linearise(dst, src, sc.INIT, np.eye(4), PRM).fragile == 0
    assert rg.linearise(dst, src, sc.T_TRUE, np.eye(4), PRM).fragile == 0
    for wt in (0.0, 3.0):
        prm = rg.params(sc.VOX, sc.TRUNC, weight_threshold=wt)
        lin = rg.linearise(ps.as_dump(ps.sphere_and_plane(sc.CLUSTER, special=False)), ps.as_dump(sc.corner_and_sphere()), sc.INIT, np.eye(4), prm)
        assert lin.fragile == 0 and lin.candidates > 0


def test_merge_after_registration_against_the_ground_truth(pair, registered):
    """What the call is for: the destination merged with the registered transform, cast from CAST_POSES (80 x 60), is 0.01006 voxel
    (mean |dz| over the commonly hit pixels) from the destination merged with T_TRUE; merged with INIT it is 1.04 voxel away."""
    dst, src = pair
    cast = {name: casts_of(mr.merge_reference(dst, src, T, sc.VOX)[0]) for name, T in
            (("registered", registered["transformation"]), ("true", sc.T_TRUE), ("init", sc.INIT))}
    dz_reg, n_reg = sc.depth_difference(cast["registered"], cast["true"])
    dz_init, n_init = sc.depth_difference(cast["init"], cast["true"])
    print(f"|dz| registered {dz_reg:.4f} voxel over {n_reg} pixels; init {dz_init:.4f} voxel over {n_init}")
    assert n_reg > 5000 and n_init > 5000
    assert abs(dz_reg - RECORDED_MERGE_DZ) <= 0.05 * RECORDED_MERGE_DZ
    assert dz_init > 10 * dz_reg


def test_dyadic_plane_is_degenerate():
    """One plane fixes three of six motions: the x / y gradients of every sample are exactly 0, the Cholesky meets a zero pivot at
    omega_z, the step is refused and the transformation is the initial one bit for bit."""
    dump = ps.as_dump(sc.dyadic_plane())
    assert np.array_equal(dump[1], sc.dyadic_plane()[1])  # multiples of 1/8 survive the import's product and quotient
    out = rg.register_reference(dump, dump, sc.DYADIC_INIT, PRM, 5)
    assert not out["success"] and out["iterations"] == 1 and out["trace"][0]["status"] == 2 and out["inliers"] > 1000
    assert np.array_equal(out["transformation"], sc.DYADIC_INIT)
    H = out["information"]
    assert np.array_equal(H[2], np.zeros(6)) and np.array_equal(H[3], np.zeros(6)) and np.array_equal(H[4], np.zeros(6))
    assert H[0, 0] > 0 and H[1, 1] > 0 and H[5, 5] > 0 and np.linalg.matrix_rank(H) == 3
    # the residual is the plane's offset: a quarter of a voxel at every inlier
    assert abs(out["inlier_rmse"] - 0.25 * sc.VOX) < 1e-12


def test_disjoint_and_empty_maps(pair):
    dst, src = pair
    far = ps.as_dump(sc.shifted(sc.corner_and_sphere(frame=sc.T_TRUE), (100, 0, 0)))
    out = rg.register_reference(far, src, sc.INIT, PRM, 5)
    assert out["inliers"] == 0 and out["candidates"] > 20000 and not out["success"] and out["iterations"] == 1
    assert np.array_equal(out["transformation"], sc.INIT) and out["fitness"] == 0.0 and out["inlier_rmse"] == 0.0
    for d, s in ((mr.empty_dump(), src), (dst, mr.empty_dump())):
        out = rg.register_reference(d, s, sc.INIT, PRM, 5)
        assert not out["success"] and np.array_equal(out["transformation"], sc.INIT) and out["inliers"] == 0


def test_argument_rules():
    ok = rg.check_arguments(sc.INIT, PRM, 30)
    assert ok is None
    scaled, mirrored, bottom, nan = sc.INIT.copy(), sc.INIT.copy(), sc.INIT.copy(), sc.INIT.copy()
    scaled[:3, :3] *= 1.001
    mirrored[:3, 0] *= -1.0
    bottom[3, 0] = 1e-3
    nan[1, 3] = np.nan
    assert [rg.check_arguments(T, PRM, 30) for T in (scaled, mirrored, bottom, nan)] == ["not rigid", "not rigid", "bottom row", "not finite"]
    assert rg.check_arguments(rigid((1, 2, 3), 179.0, (1e5, 0, 0)), PRM, 1) is None
    assert rg.check_arguments(sc.INIT, PRM, 0) == "max_iterations" and rg.check_arguments(sc.INIT, PRM, 10001) == "max_iterations"
    for bad in (dict(weight_threshold=-1.0), dict(weight_threshold=np.inf), dict(tsdf_band=0.0), dict(tsdf_band=1.5), dict(tsdf_band=np.nan),
                dict(residual_trunc=0.0), dict(residual_trunc=-0.01), dict(huber_delta=0.0), dict(huber_delta=np.nan)):
        assert rg.check_arguments(sc.INIT, rg.params(sc.VOX, sc.TRUNC, **bad), 30) is not None, bad
    assert rg.check_arguments(sc.INIT, rg.params(sc.VOX, sc.TRUNC, tsdf_band=1.0, weight_threshold=0.0), 30) is None
    with pytest.raises(ValueError):
        rg.register_reference(mr.empty_dump(), mr.empty_dump(), scaled, PRM)
    # the defaults of the binding
    assert PRM.residual_trunc == 0.5 * sc.TRUNC and PRM.huber_delta == 0.25 * sc.TRUNC and PRM.tsdf_band == 0.5 and PRM.weight_threshold == 3.0
