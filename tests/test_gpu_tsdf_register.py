"""GPU: ScalableTSDFVolume.register_volume (hv_register.hip) on planted voxel states (tests/register_scenes.py,
tests/planted_states.py), held to the numpy restatement (tests/register_reference.py) run on the planted volumes' OWN dumps.

Every traced linearisation is re-done by the restatement at the row's state A: counts equal (the transforms used put no candidate
within 1e-9 of a boundary of the rules - asserted per row), every entry of H, g and e within 1e-10 x the sum of the absolute terms
(2 x 10^5 double additions at 1.1e-16 each, plus the per-term rounding), the solve and the state update to 1e-12 / 1e-14.  The
ground-truth bars are twice what tests/test_register_reference_cpu.py records for the restatement itself: the discretisation error
of the two lattices, with room for the library ending one iteration apart.

Voxel 0.02, sdf_trunc 0.08; at most 27 units per map.

Measured on the MI355X when the file was written: every traced sum of every case is within 8.1e-16 of the restatement's relative to
its sum |terms| (counts equal, no fragile voxel); the corner-and-sphere pair converges in 4 linearisations to 1.10971e-4 m and
3.18458e-3 deg of the ground truth - the restatement's own figures to six digits; the merge with the registered transform casts
0.0101 voxel from the merge with the true one, the merge with the guess 1.04 voxel; the pair carried 200 km away differs from the
same problem at the origin by 1.32e-11 of sum |terms| in its first row.  The file runs in 4 s.
"""
import numpy as np
import pytest

from tests import planted_states as ps
from tests import register_reference as rg
from tests import register_scenes as sc
from tests.test_gpu_tsdf_deintegrate import assert_bitwise
from tests.test_gpu_tsdf_edges import volume
from tests.test_gpu_tsdf_merge import merges_that_leave_untouched
from tests.test_gpu_tsdf_merge_edges import planted
from tests.test_merge_reference_cpu import rigid
from tests.test_register_reference_cpu import (RECORDED_MERGE_DZ, RECORDED_ROTATION_ERROR, RECORDED_TRANSLATION_ERROR, cast_poses)

pytestmark = pytest.mark.gpu

VOX, TRUNC = sc.VOX, sc.TRUNC
SUM_TOL = 1e-10
SMALL = rigid((0.3, 1.0, 0.2), 2.0, (0.013, -0.007, 0.011))  # a generic guess between two maps in nearly the same frame


def check_call(dst, src, T_init, name, near_origin=True, **kw):
    """One traced call held to the restatement row by row.  -> (result, [Lin of every row])"""
    dst_dump, src_dump = dst.dump(), src.dump()
    res = dst.register_volume(src, T_init, trace=True, **kw)
    prm = rg.params(VOX, TRUNC, **{k: v for k, v in kw.items() if k != "max_iterations"})
    P = rg.Problem(dst_dump, src_dump, T_init, prm)
    assert res.iterations == len(res.trace) >= 1, name
    lins = []
    for i, row in enumerate(res.trace):
        lin = rg.linearise(dst_dump, src_dump, T_init, row["A"], prm, P)
        lins.append(lin)
        assert lin.fragile == 0, (name, i, lin.fragile)
        assert (row["inliers"], row["candidates"]) == (lin.inliers, lin.candidates), (name, i, row["inliers"], row["candidates"], lin.inliers, lin.candidates)
        dH, dg, de = np.abs(row["H"] - lin.H), np.abs(row["g"] - lin.g), abs(row["sq_error"] - lin.e)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(np.nanmax(np.where(lin.H_abs > 0, dH / lin.H_abs, 0.0)), np.nanmax(np.where(lin.g_abs > 0, dg / lin.g_abs, 0.0)), de / lin.e if lin.e else 0.0)
        print(f"{name} row {i}: status {row['status']} inliers {row['inliers']} / {row['candidates']}, worst sum error {worst:.3g} of sum |terms|")
        assert (dH <= SUM_TOL * lin.H_abs).all() and (dg <= SUM_TOL * lin.g_abs).all() and de <= SUM_TOL * lin.e, (name, i, worst)
        assert row["iteration"] == i and row["status"] in (0, 1, 2)
        if row["status"] == 2:
            assert i == len(res.trace) - 1 and not row["xi"].any(), name
            continue
        H, g, xi = row["H"], row["g"], row["xi"]
        assert np.linalg.norm(H @ xi + g) <= 1e-12 * (np.linalg.norm(H) * np.linalg.norm(xi) + np.linalg.norm(g)), (name, i)
        if i + 1 < len(res.trace):
            assert row["status"] == 0 and np.abs(res.trace[i + 1]["A"] - rg.exp_se3(xi) @ row["A"]).max() <= 1e-14, (name, i)
    last = res.trace[-1]
    A_last = last["A"] if last["status"] == 2 else rg.exp_se3(last["xi"]) @ last["A"]
    np.testing.assert_array_equal(res.anchor, P.c)
    expect = rg.compose(P.c, A_last, T_init) if not np.array_equal(A_last, np.eye(4)) else np.asarray(T_init, np.float64)
    scale = 1.0 if near_origin else max(1.0, np.abs(P.c).max())  # (far from the origin one ulp of c is 3e-11)
    assert np.abs(res.transformation - expect).max() <= 1e-14 * scale, (name, np.abs(res.transformation - expect).max())
    np.testing.assert_array_equal(res.information, last["H"])
    assert (res.inliers, res.candidates) == (last["inliers"], last["candidates"])
    assert res.success == (last["status"] != 2 and last["inliers"] >= rg.MIN_INLIERS)
    return res, lins


@pytest.fixture(scope="module")
def states():
    """(destination, source) states of the corner-and-sphere pair; shared, nothing of it may be written to."""
    return sc.corner_and_sphere(frame=sc.T_TRUE), sc.corner_and_sphere()


@pytest.fixture(scope="module")
def traced(states):
    dst, src = planted(states[0]), planted(states[1])
    res, lins = check_call(dst, src, sc.INIT, "corner and sphere")
    return res, lins, dst.dump(), src.dump()


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_row_by_row_against_the_restatement(traced):
    res, lins, _, _ = traced
    assert res.success and res.trace[-1]["status"] == 1 and 2 <= res.iterations <= 8
    assert lins[0].candidates > 20000 and lins[0].inliers > 15000


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_ground_truth(traced):
    res, lins, _, _ = traced
    t_err, r_err = sc.pose_error(res.transformation, sc.T_TRUE)
    print(f"pose error {t_err:.6g} m, {r_err:.6g} deg after {res.iterations} linearisations (restatement: {RECORDED_TRANSLATION_ERROR:.6g} m, "
          f"{RECORDED_ROTATION_ERROR:.6g} deg); fitness {res.fitness:.6f}, rmse {res.inlier_rmse:.6g}")
    assert res.success
    assert t_err <= 2 * RECORDED_TRANSLATION_ERROR and r_err <= 2 * RECORDED_ROTATION_ERROR
    last = lins[-1]
    assert abs(res.fitness - last.inliers / last.candidates) <= 1e-9
    assert abs(res.inlier_rmse - np.sqrt(last.e / last.inliers)) <= 1e-9


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_the_point_of_it(states, traced):
    """The destination merged with the registered transform looks like the destination merged with the true one; merged with the
    initial guess it shows every surface twice."""
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    res = traced[0]
    K = PinholeCameraIntrinsic(sc.CAST_W, sc.CAST_H, *sc.cast_intrinsics())
    casts = {}
    for name, T in (("registered", res.transformation), ("true", sc.T_TRUE), ("init", sc.INIT)):
        dst, src = planted(states[0]), planted(states[1])
        assert dst.integrate_volume(src, T).voxels_updated > 50000
        casts[name] = [dst.ray_cast(K, P, 0.1, 3.0, weight_threshold=3.0, render_attributes=("depth", "mask")) for P in cast_poses()]
    dz_reg, n_reg = sc.depth_difference(casts["registered"], casts["true"])
    dz_init, n_init = sc.depth_difference(casts["init"], casts["true"])
    print(f"|dz| registered {dz_reg:.4f} voxel over {n_reg} pixels (restatement {RECORDED_MERGE_DZ}); init {dz_init:.4f} voxel over {n_init}")
    assert n_reg > 5000 and n_init > 5000
    assert dz_reg <= 2 * RECORDED_MERGE_DZ
    assert dz_init > dz_reg


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_one_unit_source(states):
    """One workgroup in the collect pass, one offset in the scan."""
    src = planted(sc.corner_and_sphere(keys=[(0, -1, 3)]))
    res, lins = check_call(planted(states[0]), src, sc.INIT, "one-unit source")
    assert src.num_blocks() == 1 and 500 < lins[0].candidates < 4096 and lins[0].inliers > 100


@pytest.mark.parametrize("missing", [None, (1, 0, 4), (0, -1, 3)], ids=["all eight", "far unit missing", "own unit missing"])
def test_one_candidate_at_a_unit_corner(missing):
    """A source of one candidate voxel, the high corner of unit (0, -1, 3), carried half a voxel along every axis: the eight
    destination voxels around it lie in eight units.  With one of them missing the sample is invalid - 0 inliers, no fault."""
    units = [(i, j, k) for i in (0, 1) for j in (-1, 0) for k in (3, 4)]
    src = planted(ps.single_voxel((0, -1, 3), (15, 15, 15), tsdf=0.25, weight=5))
    dst = planted(sc.corner_and_sphere(keys=[u for u in units if u != missing]))
    T = ps.with_translation(ps.IDENTITY, (0.5, 0.5, 0.5))
    res, lins = check_call(dst, src, T, f"unit corner, {missing}", residual_trunc=1.0, huber_delta=1.0)
    assert res.candidates == 1 and res.inliers == (1 if missing is None else 0)
    assert not res.success and res.iterations == 1 and res.trace[0]["status"] == 2
    assert res.transformation.tobytes() == T.tobytes()


RIM_INLIERS = {"half": 620, "x+16.5": 0, "z-2.5": 385}  # the restatement's, on the states' as_dump
RIM_SHIFTS = {"half": (0.5, 0.5, 0.5), "x+16.5": (16.5, 0.5, 0.5), "z-2.5": (0.5, 0.5, -2.5)}


@pytest.mark.parametrize("name", list(RIM_SHIFTS))
def test_rim_of_the_key_range(name):
    """Candidates in units at +-2^20 sampled against a destination that holds the same units and the unit (-2^20, 1, -2^20) that
    (2^20, 0, -2^20) would pack to: a corner beyond the rim must find nothing, not the alias (hv_key_in_range in hv_tsdf_unit) -
    the inlier count is the restatement's, whose unit look-up checks the range too."""
    T = ps.with_translation(ps.IDENTITY, RIM_SHIFTS[name])
    src, dst = planted(ps.rim_source(alias=False)), planted(ps.rim_source(alias=True))
    res, lins = check_call(dst, src, T, f"rim {name}", weight_threshold=0.5, tsdf_band=1.0, residual_trunc=1.0, max_iterations=1)
    print(f"rim {name}: {lins[0].inliers} inliers of {lins[0].candidates}")
    assert lins[0].candidates > 5000 and lins[0].inliers == RIM_INLIERS[name]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 513])
def test_wave_tails_and_the_grid_stride_remainder(states, count, monkeypatch):
    """1, 63, 64, 65 candidates: a wave's tail; 513 against a grid capped at two workgroups (512 threads): one more than a full grid
    pass, the grid-stride remainder."""
    monkeypatch.setenv("HV_REGISTER_GRID_BLOCKS", "2")
    src = planted(sc.few_voxels(count))
    res, lins = check_call(planted(states[0]), src, sc.INIT, f"{count} candidates", residual_trunc=0.1, max_iterations=2)
    assert lins[0].candidates == count and lins[0].inliers == count


def test_weight_threshold_zero_against_three():
    """Weights 1..7 with a tenth of the voxels unobserved, in both maps: at threshold 0 every observed voxel counts, at 3 only
    weights 4..7 - in the source's candidates and in all eight voxels of a destination sample."""
    src_states = ps.sphere_and_plane(ps.cluster_keys(), seed=1, special=False)
    n = {}
    for wt in (0.0, 3.0):
        res, lins = check_call(planted(ps.sphere_and_plane(ps.cluster_keys(), seed=2, special=False)), planted(src_states), SMALL, f"threshold {wt}",
                               weight_threshold=wt, max_iterations=2)
        n[wt] = (lins[0].candidates, lins[0].inliers)
    weights = src_states[2]
    print("threshold 0 / 3: (candidates, inliers)", n)
    assert n[3.0][0] < 0.7 * n[0.0][0] and 0 < n[3.0][1] < 0.1 * n[0.0][1]  # (4 / 7)^8 of the samples stay valid
    assert (weights > 0).sum() > (weights > 3).sum() > 0


def test_far_from_the_origin(states):
    """The same pair carried 200 km away (planted_states.FAR_T, rounded to whole units so that the destination's lattice meets the
    field where it did) against the call that poses the same problem at the origin (register_scenes.brought_back: the far anchor is
    rounded to the 3e-11 m a double resolves out there, and the near call is given exactly that problem).  The sums of the first
    linearisation agree within the tolerance that holds the library to the restatement - the anchor keeps y = p - c, and with it J,
    H and g, free of the 2e5 m in p - and the far call ends as close to the ground truth.
    The restatement run on the states' as_dump gives a worst difference of 1.3e-11 of sum |terms| (the rounding of p = c + y)."""
    units = np.rint(np.array(ps.FAR_T) / ps.UNIT).astype(np.int64)
    far_T = sc.INIT.copy()
    far_T[:3, 3] += units * ps.UNIT
    near_T = sc.brought_back(far_T, units, states[1][0])
    assert np.abs(near_T - sc.INIT).max() < 1e-10
    src = planted(states[1])
    res, lins = check_call(planted(sc.shifted(states[0], units)), src, far_T, "far", near_origin=False)
    near, _ = check_call(planted(states[0]), src, near_T, "near")
    a, b, lin = res.trace[0], near.trace[0], lins[0]
    assert (a["inliers"], a["candidates"]) == (b["inliers"], b["candidates"])
    worst = max((np.abs(a["H"] - b["H"]) / lin.H_abs).max(), (np.abs(a["g"] - b["g"]) / lin.g_abs).max(), abs(a["sq_error"] - b["sq_error"]) / lin.e)
    print(f"far against near, first row: worst difference {worst:.3g} of sum |terms|; far {res.iterations} rows, near {near.iterations}")
    assert worst <= SUM_TOL
    assert res.success and np.abs(res.anchor).max() > 1e5 and res.iterations == near.iterations
    back = res.transformation.copy()
    back[:3, 3] -= units * ps.UNIT
    t_err, r_err = sc.pose_error(back, sc.T_TRUE)
    assert t_err <= 2 * RECORDED_TRANSLATION_ERROR and r_err <= 2 * RECORDED_ROTATION_ERROR


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_dyadic_plane_is_degenerate():
    dst, src = planted(sc.dyadic_plane()), planted(sc.dyadic_plane())
    res, lins = check_call(dst, src, sc.DYADIC_INIT, "dyadic plane")
    assert not res.success and res.iterations == 1 and res.trace[0]["status"] == 2 and res.inliers > 1000
    assert res.transformation.tobytes() == sc.DYADIC_INIT.tobytes()
    assert not res.information[2:5].any() and abs(res.inlier_rmse - 0.25 * VOX) < 1e-12


def test_disjoint_and_empty_maps(states):
    dst, src = planted(states[0]), planted(states[1])
    away = planted(sc.shifted(states[0], (100, 0, 0)))
    res, _ = check_call(away, src, sc.INIT, "disjoint")
    assert not res.success and res.inliers == 0 and res.candidates > 20000 and res.fitness == 0.0 and res.inlier_rmse == 0.0
    assert res.transformation.tobytes() == sc.INIT.tobytes()
    for name, d, s in (("empty source", dst, volume(VOX, TRUNC)), ("empty destination", volume(VOX, TRUNC), src),
                       ("no candidate", dst, planted(ps.empty_units([(0, 0, 0)])))):
        res = d.register_volume(s, sc.INIT, trace=True)
        assert not res.success and res.inliers == 0, name
        assert res.transformation.tobytes() == sc.INIT.tobytes()
        assert (res.iterations, len(res.trace), res.candidates) == ((1, 1, 22085) if name == "empty destination" else (0, 0, 0)), name


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_reads_only_and_reproducible(states):
    dst, src = planted(states[0]), planted(states[1])
    src.mark_merged()
    src_before, n_src, n_dst = src.dump(), src.num_blocks(), dst.num_blocks()
    a, b = merges_that_leave_untouched(dst, [lambda: dst.register_volume(src, sc.INIT, trace=True) for _ in range(2)])
    assert_bitwise(src.dump(), src_before)
    assert len(src.dirty_keys()) == 0 and (src.num_blocks(), dst.num_blocks()) == (n_src, n_dst)
    assert a.success and a.iterations == b.iterations and (a.inliers, a.candidates) == (b.inliers, b.candidates)
    for x, y in ((a.transformation, b.transformation), (a.information, b.information), (a.anchor, b.anchor),
                 (np.array([a.fitness, a.inlier_rmse]), np.array([b.fitness, b.inlier_rmse]))):
        assert x.tobytes() == y.tobytes()
    for ra, rb in zip(a.trace, b.trace):
        assert all(np.asarray(ra[k]).tobytes() == np.asarray(rb[k]).tobytes() for k in ra)
    # the untraced call is the traced one
    c = dst.register_volume(src, sc.INIT)
    assert c.trace is None and c.transformation.tobytes() == a.transformation.tobytes() and c.information.tobytes() == a.information.tobytes()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(states):
    from pyslam_amd import _lib as L
    from pyslam_amd._lib import HipVolError
    from pyslam_amd.volumetric import VoxelBlockGrid

    dst, src = planted(states[0]), planted(states[1])
    before, src_before = dst.dump(), src.dump()

    def refused(match, d, s_, T=sc.INIT, **kw):
        with pytest.raises(HipVolError, match=match):
            d.register_volume(s_, T, **kw)

    grid = VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12)
    assert not hasattr(grid, "register_volume")
    refused("TSDF", dst, grid)
    with pytest.raises(HipVolError, match="TSDF"):
        type(dst).register_volume(grid, src)
    tiled = volume(VOX, TRUNC)
    tiled.set_tile(0, 0, 80, 120)
    refused("tile", dst, tiled)
    refused("tile", tiled, src)
    owned = volume(VOX, TRUNC)
    owned.set_owner(0, 2)
    refused("owner", dst, owned)
    refused("owner", owned, src)
    refused("same volume", dst, dst)
    refused("differ", dst, volume(0.01, TRUNC))
    refused("differ", dst, volume(VOX, 0.1))
    refused("differ", volume(VOX, 0.06), src)
    scaled, mirrored, bottom, nan = sc.INIT.copy(), sc.INIT.copy(), sc.INIT.copy(), sc.INIT.copy()
    scaled[:3, :3] *= 1.001
    mirrored[:3, 0] *= -1.0
    bottom[3, 3] = 2.0
    nan[0, 3] = np.nan
    refused("not rigid", dst, src, scaled)
    refused("not rigid", dst, src, mirrored)
    refused("bottom row", dst, src, bottom)
    refused("not finite", dst, src, nan)
    refused("max_iterations", dst, src, max_iterations=0)
    refused("max_iterations", dst, src, max_iterations=10001)
    refused("tsdf_band", dst, src, tsdf_band=0.0)
    refused("tsdf_band", dst, src, tsdf_band=1.01)
    refused("weight_threshold", dst, src, weight_threshold=-1.0)
    refused("residual_trunc", dst, src, residual_trunc=-0.01)
    refused("residual_trunc", dst, src, huber_delta=0.0)
    with pytest.raises(ValueError):
        dst.register_volume(src, np.eye(3))
    with pytest.raises(TypeError):
        dst.register_volume(None)
    with pytest.raises(HipVolError, match="null"):
        L.check(dst._lib.hv_tsdf_register_volume(dst._h, src._h, None, None, None, None, 0, None))
    assert dst.register_volume(src, sc.INIT, tsdf_band=1.0, weight_threshold=0.0, max_iterations=1).iterations == 1
    assert_bitwise(dst.dump(), before)
    assert_bitwise(src.dump(), src_before)
