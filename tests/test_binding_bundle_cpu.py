"""What bundle_adjust and bundle_linearise send over the C ABI, pinned against the recording stand-in for the library
(tests/recording_lib.py; no GPU), in the manner of tests/test_binding_pose_graph_cpu.py; and the two-phase schedule of
pyslam_amd/bundle.py on a stub volume."""
import types

import numpy as np
import pytest

from pyslam_amd import _lib as L
from pyslam_amd import bundle as B
from pyslam_amd import volumetric as V
from pyslam_amd import volumetric_semantic as S
from tests.recording_lib import ref, volume
from tests.test_binding_calls_cpu import ANY, SKIP, P, REF, covers, expect, host, refused, shaped, tsdf  # noqa: F401 (host: a fixture)

I64 = L.ctypes.c_int64
FIELDS = ("fx", "fy", "cx", "cy", "bf", "huber_delta2_mono", "huber_delta2_stereo", "min_depth", "lambda_scale", "gradient_tolerance",
          "step_tolerance", "decrease_tolerance", "residual_tolerance", "cg_tolerance", "max_iterations", "cg_max_iterations", "huber",
          "fixed_points", "trace_state", "reserved")
CAM = types.SimpleNamespace(fx=30.0, fy=31.0, cx=9.5, cy=2.5)


def problem(n=3, m=5, seed=0):
    rng = np.random.default_rng(seed)
    cams = np.tile(np.eye(4), (n, 1, 1))
    cams[:, :3, 3] = rng.random((n, 3))
    pts = rng.random((m, 3)) + (0, 0, 3)
    idx = np.stack(np.meshgrid(np.arange(n), np.arange(m), indexing="ij"), -1).reshape(-1, 2).astype(np.int32)
    uv = rng.random((n * m, 2)) * 20
    return cams, pts, idx, uv


def params(call, index):
    p = ref(call[1][index])
    return {f: getattr(p, f) for f in FIELDS}


def test_structs_mirror_the_header():
    assert [n for n, _ in L.HvBundleParams._fields_] == list(FIELDS)
    assert L.ctypes.sizeof(L.HvBundleParams) == 14 * 8 + 6 * 4
    assert [n for n, _ in L.HvBundleResult._fields_] == ["chi2_initial", "chi2_final", "lambda_", "iterations", "cg_iterations_total", "converged",
                                                       "success"]
    assert L.ctypes.sizeof(L.HvBundleResult) == 3 * 8 + 4 * 4
    text = open(L.os.path.join(L.os.path.dirname(L.os.path.dirname(L.__file__)), "include", "hipvol.h")).read()
    header = text[text.index("typedef struct hv_bundle_params"):text.index("} hv_bundle_params;")]
    assert [f for f in FIELDS if f not in header] == []


@covers("bundle_adjust")
def test_defaults_on_every_kind_of_volume(host):
    cams, pts, idx, uv = problem()
    before = cams.copy(), pts.copy()
    for vol in (tsdf(), volume(V.VoxelBlockGrid, voxel_size=0.05, block_size=8), volume(S.VoxelBlockSemanticGrid, voxel_size=0.05, block_size=8)):
        vol._lib.script("hv_bundle_adjust", peek={1: (np.float64, 48), 3: (np.float64, 15), 7: (np.float64, 60)})
        out = vol.bundle_adjust(host(cams), host(pts), host(idx), host(uv), CAM)
        call, = expect(vol, ("hv_bundle_adjust", P(out.cameras), 3, P(out.points), 5, None, P(idx), ANY, None, 15, REF(L.HvBundleParams), P(out.chi2),
                             ANY, REF(L.HvBundleResult), None, None, None, 0, REF(I64), L.HV_HOST))
        assert params(call, 10) == dict(fx=30.0, fy=31.0, cx=9.5, cy=2.5, bf=1.0, huber_delta2_mono=5.991, huber_delta2_stereo=7.815, min_depth=1e-6,
                                        lambda_scale=1e-5, gradient_tolerance=1e-6, step_tolerance=1e-6, decrease_tolerance=1e-6,
                                        residual_tolerance=1e-6, cg_tolerance=1e-8, max_iterations=100, cg_max_iterations=100, huber=1,
                                        fixed_points=0, trace_state=0, reserved=0)
        # the in / out buffers are the result's own arrays, filled with the caller's state; the caller's arrays are not written
        got = vol._lib.peeked[-1]
        np.testing.assert_array_equal(got[1], before[0].ravel())
        np.testing.assert_array_equal(got[3], before[1].ravel())
        # (u, v) measurements become (u, v, nan, inv_sigma2) records: monocular, weight 1
        rec = got[7].reshape(15, 4)
        np.testing.assert_array_equal(rec[:, :2], uv)
        assert np.isnan(rec[:, 2]).all() and (rec[:, 3] == 1.0).all()
        assert np.array_equal(cams, before[0]) and np.array_equal(pts, before[1]) and out.cameras is not cams and out.points is not pts
        shaped(out.cameras, (3, 4, 4), np.float64), shaped(out.points, (5, 3), np.float64), shaped(out.chi2, (15,), np.float64)
        shaped(out.behind, (15,), np.bool_), shaped(out.inlier, (15,), np.bool_)
        assert isinstance(out, V.BundleResult) and out.trace is None and out.success is False and out.converged == "max_iterations"
        assert out.iterations == 0 and out.chi2_final == 0.0 and out.inlier.all() and not out.behind.any()


@covers("bundle_adjust")
def test_marshals_every_argument_dtype_and_layout(host):
    cams, pts, idx, uv = problem(4, 6)
    vol = tsdf()
    vol._lib.script("hv_bundle_adjust", 2, peek={5: (np.uint8, 4), 6: (np.int32, 48), 7: (np.float64, 96), 8: (np.uint8, 24)})
    z = np.c_[uv, np.where(np.arange(24) % 2 == 0, uv[:, 0] - 2.0, np.inf)]
    s2 = 4.0 ** -(np.arange(24) % 3)
    active = np.arange(24) % 5 != 0
    wide = np.zeros((6, 6))
    wide[:, ::2] = pts  # a strided operand is sent contiguous
    out = vol.bundle_adjust(host(cams.astype(np.float32)), wide[:, ::2], idx.astype(np.int64).tolist(), host(np.asfortranarray(z)), CAM, bf=7.5,
                            inv_sigma2=host(s2.astype(np.float32)), active=active.tolist(), camera_fixed=[1, 0, 0, 1], fixed_points=True,
                            huber=False, trace=True, max_iterations=7, cg_max_iterations=9, lambda_scale=1e-3, gradient_tolerance=1e-7,
                            step_tolerance=1e-8, decrease_tolerance=1e-9, residual_tolerance=1e-10, cg_tolerance=1e-4, min_depth=0.5,
                            huber_delta2_mono=2.0, huber_delta2_stereo=3.0)
    call, = expect(vol, ("hv_bundle_adjust", P(out.cameras), 4, P(out.points), 6, ANY, ANY, ANY, ANY, 24, REF(L.HvBundleParams), P(out.chi2), ANY,
                         REF(L.HvBundleResult), ANY, ANY, ANY, 7, REF(I64), L.HV_HOST))
    assert params(call, 10) == dict(fx=30.0, fy=31.0, cx=9.5, cy=2.5, bf=7.5, huber_delta2_mono=2.0, huber_delta2_stereo=3.0, min_depth=0.5,
                                    lambda_scale=1e-3, gradient_tolerance=1e-7, step_tolerance=1e-8, decrease_tolerance=1e-9,
                                    residual_tolerance=1e-10, cg_tolerance=1e-4, max_iterations=7, cg_max_iterations=9, huber=0, fixed_points=1,
                                    trace_state=1, reserved=0)
    got = vol._lib.peeked[-1]
    np.testing.assert_array_equal(got[5], [1, 0, 0, 1])
    np.testing.assert_array_equal(got[6], idx.ravel())
    np.testing.assert_array_equal(got[7].reshape(24, 4), np.c_[z, s2])
    np.testing.assert_array_equal(got[8], active.astype(np.uint8))
    # inlier: active, not behind, chi2 (0 from the stand-in) within the gate of its kind
    assert np.array_equal(out.inlier, active)
    # two rows came back (scripted), each with the state its iteration started from
    assert len(out.trace) == 2 and set(out.trace[0]) == {n for n, _ in V._POSE_GRAPH_TRACE} | {"cameras", "points"}
    assert out.trace[1]["cameras"].shape == (4, 4, 4) and out.trace[1]["points"].shape == (6, 3)
    # no observation at all is a legal problem
    vol = tsdf()
    out = vol.bundle_adjust(cams, pts, np.zeros((0, 2), np.int32), np.zeros((0, 3)), CAM)
    expect(vol, ("hv_bundle_adjust", P(out.cameras), 4, P(out.points), 6, None, SKIP, SKIP, None, 0, REF(L.HvBundleParams), SKIP, SKIP,
                 REF(L.HvBundleResult), None, None, None, 0, REF(I64), L.HV_HOST))
    assert out.chi2.shape == (0,) and out.inlier.shape == (0,)


@covers("bundle_adjust")
def test_refusals_come_before_any_call():
    cams, pts, idx, uv = problem()
    vol = tsdf()
    call = vol.bundle_adjust
    refused(vol, ValueError, "cameras must be [N,4,4], got (3, 16)", call, cams.reshape(3, 16), pts, idx, uv, CAM)
    refused(vol, ValueError, "points must be [M,3], got (3, 5)", call, cams, pts.T, idx, uv, CAM)
    refused(vol, ValueError, "measurements must be [15,2] (u, v) or [15,3] (u, v, u_r) for 15 observations, got (14, 2)", call, cams, pts, idx, uv[:14], CAM)
    refused(vol, ValueError, "measurements must be [15,2] (u, v) or [15,3] (u, v, u_r) for 15 observations, got (15, 4)", call, cams, pts, idx,
            np.zeros((15, 4)), CAM)
    refused(vol, ValueError, "inv_sigma2 must be a number or [15], got (14,)", call, cams, pts, idx, uv, CAM, inv_sigma2=np.ones(14))
    refused(vol, ValueError, "active must be [15], got (3,)", call, cams, pts, idx, uv, CAM, active=[1, 1, 1])
    refused(vol, ValueError, "camera_fixed must be [3], got (4,)", call, cams, pts, idx, uv, CAM, camera_fixed=[1, 0, 0, 0])
    refused(vol, ValueError, "bf must be positive and finite, got 0.0", call, cams, pts, idx, uv, CAM, bf=0.0)
    refused(vol, ValueError, "max_iterations and cg_max_iterations must be in 1..10000", call, cams, pts, idx, uv, CAM, max_iterations=0)
    refused(vol, ValueError, "max_iterations and cg_max_iterations must be in 1..10000", call, cams, pts, idx, uv, CAM, cg_max_iterations=10001)
    refused(vol, TypeError, "unknown parameter fixed (known: huber_delta2_mono", call, cams, pts, idx, uv, CAM, fixed=0)


@covers("bundle_linearise")
def test_linearise_call(host):
    cams, pts, idx, uv = problem()
    vol = tsdf()
    out = vol.bundle_linearise(host(cams), host(pts), host(idx), host(uv), CAM, bf=2.0, huber=False, min_depth=0.25)
    call, = expect(vol, ("hv_bundle_linearise", P(cams), 3, P(pts), 5, P(idx), ANY, None, 15, REF(L.HvBundleParams), P(out["r"]), P(out["chi2"]),
                         P(out["w"]), ANY, P(out["B"]), P(out["bc"]), P(out["C"]), P(out["bp"]), ANY, L.HV_HOST))
    p = params(call, 9)
    assert (p["bf"], p["huber"], p["min_depth"], p["fixed_points"], p["trace_state"]) == (2.0, 0, 0.25, 0, 0)
    shaped(out["r"], (15, 3), np.float64), shaped(out["B"], (3, 6, 6), np.float64), shaped(out["C"], (5, 3, 3), np.float64)
    shaped(out["bc"], (3, 6), np.float64), shaped(out["bp"], (5, 3), np.float64), shaped(out["behind"], (15,), np.bool_)
    assert out["F"] == 0.0
    refused(vol, ValueError, "needs a camera, a point and an observation, got 3, 5, 0", vol.bundle_linearise, cams, pts, idx[:0], uv[:0], CAM)


# -- the two-phase schedule on a stub ------------------------------------------------------------------------------------------

class StubVolume:
    def __init__(self, inlier):
        self.calls, self.inlier = [], np.asarray(inlier, bool)

    def bundle_adjust(self, cameras, points, observations, measurements, intrinsic, **kw):
        self.calls.append(dict(kw, cameras=cameras, points=points))
        O = len(observations)
        moved = cameras + 1.0
        return V.BundleResult(moved, points + 1.0, np.arange(O, dtype=np.float64), np.zeros(O, bool), self.inlier.copy(), 9.0, 3.0, 0.1,
                              kw["max_iterations"], 5, "max_iterations", False, None)


def test_two_phase_schedule():
    cams, pts, idx, uv = problem()
    inlier = np.arange(15) % 4 != 0
    stub = StubVolume(inlier)
    result, active, mean = B.bundle_adjust_two_phase(stub, cams, pts, idx, uv, CAM, bf=3.0, camera_fixed=[1, 0, 0], rounds=7, cg_tolerance=1e-6)
    first, second = stub.calls
    assert (first["huber"], first["max_iterations"], first.get("active")) == (True, 3, None)
    assert (second["huber"], second["max_iterations"]) == (False, 4) and np.array_equal(second["active"], inlier)
    assert first["cg_tolerance"] == second["cg_tolerance"] == 1e-6 and first["bf"] == second["bf"] == 3.0
    assert np.array_equal(second["cameras"], cams + 1.0) and np.array_equal(result.cameras, cams + 2.0)
    assert np.array_equal(active, inlier) and mean == np.arange(15.0)[inlier].mean()
    # one round: the first phase alone
    stub = StubVolume(inlier)
    result, _, _ = B.bundle_adjust_two_phase(stub, cams, pts, idx, uv, CAM, bf=3.0, rounds=1)
    assert len(stub.calls) == 1 and stub.calls[0]["max_iterations"] == 1 and np.array_equal(result.cameras, cams + 1.0)
