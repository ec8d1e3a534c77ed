"""CPU: the ray-cast contract (include/hipvol.h, hv_tsdf_ray_cast) as tests/raycast_reference.py restates it, held to closed-form
geometry, and the new entry point's presence in the library and the binding.  No GPU.

Measured when the thresholds were set (C restatement oracle.PortTsdf fed tests/tsdf_closed_form.frames(), weight_threshold 0.5,
640 x 480, 5 mm voxels):
    input pose  hits 99.92 % of the observed ground-truth pixels; |dz| median 0.020 voxel, p99 0.49 voxel; normal error median 1.11 deg
    novel pose  hits 99.99 %;                                       |dz| median 0.016 voxel, p99 0.53 voxel; normal error median 0.95 deg
The bars below (>= 97 %, median <= 0.2 voxel, p99 <= 1 voxel, median <= 3 deg) leave room for a field fused another way.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import raycast_reference as rr
from tests import tsdf_closed_form as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOVEL = cf.pose((-0.05, 0.025, -0.275), (0.075, -0.025, 1.25))  # between the first two input poses


def test_header_constants_match_the_reference():
    text = open(os.path.join(ROOT, "include", "hipvol.h")).read()
    consts = dict(re.findall(r"#define\s+HV_RAYCAST_(\w+)\s+([0-9.]+)f?", text))
    assert float(consts["STEP_FRAC"]) == rr.STEP_FRAC
    assert int(consts["REFINE_ITERS"]) == rr.REFINE_ITERS
    assert float(consts["UNIT_EPS"]) == rr.UNIT_EPS


def test_ray_cast_is_bound_and_exported():
    from pyslam_amd import _lib, build

    assert "hv_tsdf_ray_cast" in _lib.SIGNATURES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "hv_tsdf_ray_cast")


def _linear_volume(z0, voxel=0.005, trunc=0.04):
    """Units (0, 0, 0..4) holding tsdf = clip((z0 - z) / trunc, -1, 1) at every voxel centre, weight 10, one colour."""
    import oracle

    vol = oracle.PortTsdf(voxel, trunc)
    keys = np.array([[0, 0, k] for k in range(5)], np.int32)
    zc = (np.arange(16) + 0.5) * voxel
    tsdf = np.zeros((5, 16, 16, 16), np.float32)
    for k in range(5):
        tsdf[k] = np.clip((z0 - (k * 16 * voxel + zc)) / trunc, -1.0, 1.0)[None, None, :]
    weight = np.full((5, 16, 16, 16), 10.0, np.float32)
    color = np.broadcast_to(np.array([100.0, 150.0, 200.0]), (5, 16, 16, 16, 3)).copy()
    vol.load_units(keys, tsdf, weight, color)
    return vol


def test_linear_field_root_is_exact():
    z0 = 0.2137
    dump = _linear_volume(z0).dump()
    T_cw = np.eye(4)
    T_cw[:3, 3] = [-0.04, -0.04, 0.0]  # camera centre (0.04, 0.04, 0): the rays stay inside the units' x / y extent
    intr = (500.0, 500.0, 3.5, 3.5)
    out = rr.ray_cast(dump, 0.005, 0.04, intr, T_cw, 8, 8, depth_min=0.1, depth_max=0.39)
    assert out["mask"].all()
    np.testing.assert_allclose(out["depth"], z0, atol=1e-6)
    np.testing.assert_allclose(out["vertex"][..., 2], z0, atol=1e-6)
    np.testing.assert_allclose(out["normal"], np.broadcast_to([0.0, 0.0, -1.0], (8, 8, 3)), atol=1e-6)
    np.testing.assert_allclose(out["color"], np.broadcast_to(np.array([100, 150, 200]) / 255.0, (8, 8, 3)), atol=1e-6)
    # unobserved (weight not above the threshold): no hit; a subset of attributes gives the same depth
    assert not rr.ray_cast(dump, 0.005, 0.04, intr, T_cw, 8, 8, 0.1, 0.39, weight_threshold=10.0)["mask"].any()
    sub = rr.ray_cast(dump, 0.005, 0.04, intr, T_cw, 8, 8, 0.1, 0.39, render_attributes=("depth",))
    assert set(sub) == {"depth"} and np.array_equal(sub["depth"], out["depth"])


def closed_form_scores(out, T_cw, dump, weight_threshold):
    """-> dict: hit fraction on the ground-truth pixels whose surface voxel is observed, |dz| in voxels, normal error in degrees."""
    gt, _ = cf.render(T_cw)
    fx, fy, cx, cy = cf.K
    T_wc = np.linalg.inv(T_cw)
    v, u = np.mgrid[0:cf.H, 0:cf.W].astype(np.float64)
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ T_wc[:3, :3].T
    o = T_wc[:3, 3]
    p = o + gt[..., None].astype(np.float64) * d
    grid = rr._Grid(dump)
    gv = np.floor(p / cf.VOXEL).astype(np.int64)
    row, word = grid.locate(gv[..., 0], gv[..., 1], gv[..., 2])
    observed = (gt > 0) & (row >= 0) & (grid.weight[np.maximum(row, 0), word] > weight_threshold)
    mask = np.asarray(out["mask"], bool)
    both = mask & (gt > 0)
    dz = np.abs(np.asarray(out["depth"], np.float64) - gt)[both] / cf.VOXEL
    on_sphere = np.abs(np.linalg.norm(p - cf.SPHERE_C, axis=-1) - cf.SPHERE_R) < np.abs(p @ cf.PLANE_N - cf.PLANE_D)
    n_gt = np.where(on_sphere[..., None], (p - cf.SPHERE_C) / cf.SPHERE_R, cf.PLANE_N)
    n_gt = n_gt * np.sign(((o - p) * n_gt).sum(-1))[..., None]  # facing the camera: the tsdf grows towards free space
    ang = np.degrees(np.arccos(np.clip((np.asarray(out["normal"], np.float64) * n_gt).sum(-1), -1.0, 1.0)))[both]
    return {"hit_frac": float((mask & observed).sum() / observed.sum()), "dz_median": float(np.median(dz)),
            "dz_p99": float(np.percentile(dz, 99)), "normal_median_deg": float(np.median(ang))}


def check_closed_form_scores(s):
    assert s["hit_frac"] >= 0.97, s
    assert s["dz_median"] <= 0.2 and s["dz_p99"] <= 1.0, s
    assert s["normal_median_deg"] <= 3.0, s


@pytest.fixture(scope="module")
def closed_form_dump():
    import oracle

    vol = oracle.PortTsdf(cf.VOXEL, cf.TRUNC)
    for depth, rgb, T in cf.frames():
        vol.integrate(depth, rgb, cf.K, T, 1.0, cf.DEPTH_TRUNC)
    return vol.dump()


@pytest.mark.parametrize("which", ["input", "novel"])
def test_closed_form_scene(closed_form_dump, which):
    T = cf.POSES[0] if which == "input" else NOVEL
    out = rr.ray_cast(closed_form_dump, cf.VOXEL, cf.TRUNC, cf.K, T, cf.H, cf.W, 0.1, 3.0, 0.5)
    check_closed_form_scores(closed_form_scores(out, T, closed_form_dump, 0.5))
    hit = out["mask"]
    assert not out["depth"][~hit].any() and not out["normal"][~hit].any() and not out["color"][~hit].any()
    assert (out["color"][hit] >= 0).all() and (out["color"][hit] <= 1).all()
