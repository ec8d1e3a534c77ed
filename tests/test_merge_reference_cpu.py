"""CPU: the volume-to-volume fusion contract (include/hipvol.h, hv_tsdf_integrate_volume) as tests/merge_reference.py restates it,
held to exact shifts and to the closed-form scene's ground truth, and the entry point's presence in the library and the binding.
No GPU.

The maps are fused by the C restatement oracle.PortTsdf from tests/tsdf_closed_form.frames() (640 x 480, 5 mm voxels, stride 4) and
ray-cast by tests/raycast_reference.ray_cast (weight_threshold 0.5) at the three input poses and at NOVEL; a map that lives in
another frame is cast at the pose carried there (T_cw T^-1) and scored in the scene's frame.  The bars are the ones
tests/test_raycast_reference_cpu.py sets for a fused field: >= 97 % hits, |dz| median <= 0.2 voxel, p99 <= 1 voxel, normal error
median <= 3 deg.

Measured when the thresholds were set (poses 0, 1, 2, NOVEL):
    directly fused (frames 0-2)   hits 99.92 / 99.95 / 99.97 / 99.99 %; |dz| median 0.020 / 0.014 / 0.013 / 0.016 voxel; p99 0.49 / 0.49 / 0.62 / 0.53 voxel
    moved by GENERIC (one merge)  hits 99.91 / 99.93 / 99.95 / 99.99 %; |dz| median 0.013 / 0.010 / 0.009 / 0.011 voxel; p99 0.58 / 0.53 / 0.65 / 0.60 voxel
    frames 0-1 joined with frame 2 held in OTHER   hits 99.92 / 99.95 / 99.95 / 99.99 %; median 0.020 / 0.014 / 0.012 / 0.016; p99 0.55 / 0.51 / 0.64 / 0.55;
                                  hit counts within 0.1 % of the directly fused map's at every pose
    2 773 source units with a weight, 7.50 M observed voxels; the moved map holds 3 895 units, 7.06 M voxels from a trilinear
    sample and 0.44 M from a nearest one.  The directly fused map meets every bar at every pose, so the rule for a pose at which
    it does not (its own p99 plus 1.5 x the measured gap) has no case here and its gap constant is 0.
    round trip (GENERIC, then its inverse, fresh volumes): 7.48 M of 7.51 M observed voxels observed in both; |d tsdf| median 1e-4,
    p99 0.052 (0.41 voxel), max 2.0 (a voxel at the back of the truncation band changes sign).  No bar: reported in DESIGN.md.
"""
import ctypes

import numpy as np
import pytest

from tests import raycast_reference as rr
from tests import tsdf_closed_form as cf
from tests.merge_reference import check_rigid, empty_dump, merge_reference
from tests.test_raycast_reference_cpu import NOVEL, check_closed_form_scores, closed_form_scores

THR = 0.5


def rigid(axis, degrees, translation):
    """Rodrigues rotation about `axis` and a translation -> float64 [4,4]."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    a = np.radians(degrees)
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * Kx + (1.0 - np.cos(a)) * (Kx @ Kx)
    T[:3, 3] = translation
    return T


def rigid_inverse(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


GENERIC = rigid((0.3, 1.0, 0.2), 23.0, (0.31, -0.12, 0.23))
OTHER = rigid((1.0, -0.4, 0.5), -17.0, (-0.27, 0.18, 0.12))  # the frame the second map of the overlap case is held in
SHIFT = np.array([3, -2, 5])
CAST_POSES = tuple(cf.POSES) + (NOVEL,)


def translation(voxels, voxel_length):
    T = np.eye(4)
    T[:3, 3] = np.asarray(voxels, np.float64) * voxel_length
    return T


def test_integrate_volume_is_bound_and_exported():
    from pyslam_amd import _lib, build

    assert "hv_tsdf_integrate_volume" in _lib.SIGNATURES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "hv_tsdf_integrate_volume")
    from pyslam_amd.volumetric import MergeStats, ScalableTSDFVolume

    assert hasattr(ScalableTSDFVolume, "integrate_volume")
    assert MergeStats(1, 2, 7, 3, 4).as_tuple() == (1, 2, 7, 3, 4)


def test_argument_rules():
    assert check_rigid(np.eye(4)) is None and check_rigid(GENERIC) is None and check_rigid(rigid_inverse(GENERIC)) is None
    bad = np.eye(4)
    bad[0, 0] = np.nan
    assert check_rigid(bad) == "not finite"
    bad = np.eye(4)
    bad[3, 0] = 1e-3
    assert check_rigid(bad) == "bottom row"
    assert check_rigid(np.diag([1.0, 1.0, -1.0, 1.0])) == "not rigid"
    assert check_rigid(np.diag([1.001, 1.0, 1.0, 1.0])) == "not rigid"
    np.testing.assert_allclose(GENERIC @ rigid_inverse(GENERIC), np.eye(4), atol=1e-15)


# ---- whole-voxel shifts ------------------------------------------------------------------------------------------------------
def tiny_dump(start=0, count=6):
    import oracle
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD("tiny_160x120_2cm")
    vol = oracle.PortTsdf(0.02, 0.08)
    K = np.array(s.intrinsics, np.float64)
    for i in range(start, start + count):
        depth, rgb, T = s[i]
        vol.integrate(depth, rgb, K, T, 1.0, 4.0)
    return vol.dump()


def observed_voxels(dump):
    """-> global voxel indices [n,3] of the voxels with a weight, their tsdf, weight, colour sums (rint(mean * weight))."""
    keys, tsdf, weight, colour = (np.asarray(x) for x in dump)
    u, w = np.nonzero(weight.reshape(len(keys), -1) > 0)
    local = np.stack([w // 256, (w // 16) % 16, w % 16], axis=-1)
    wt = weight.reshape(len(keys), -1)[u, w].astype(np.float64)
    sums = np.rint(np.asarray(colour, np.float64).reshape(len(keys), -1, 3)[u, w] * wt[:, None])
    return keys.astype(np.int64)[u] * 16 + local, tsdf.reshape(len(keys), -1)[u, w], wt, sums


def assert_is_shifted_source(out_dump, src_dump, shift, what):
    """Every observed voxel of out_dump is the source's voxel `shift` voxels away and vice versa: weights and colour sums exactly,
    tsdf within 2^-23 (one float32 rounding of a value in [-1, 1]; the off voxels' trilinear weights are <= 1e-12)."""
    gi, t, w, c = observed_voxels(out_dump)
    sgi, st, sw, sc = observed_voxels(src_dump)
    assert len(gi) == len(sgi) > 0, (what, len(gi), len(sgi))
    a = np.lexsort((gi - shift).T[::-1])
    b = np.lexsort(sgi.T[::-1])
    np.testing.assert_array_equal((gi - shift)[a], sgi[b], err_msg=what)
    np.testing.assert_array_equal(w[a], sw[b], err_msg=what)
    np.testing.assert_array_equal(c[a], sc[b], err_msg=what)
    err = float(np.abs(t[a].astype(np.float64) - st[b].astype(np.float64)).max())
    assert err <= 2.0 ** -23, (what, err)
    # no all-zero unit is left behind
    assert (np.asarray(out_dump[2]).reshape(len(out_dump[0]), -1).max(axis=1) > 0).all(), what
    return err


def assert_is_permuted_source(out_dump, src_dump, T, voxel_length, what):
    """assert_is_shifted_source for a signed-permutation rotation with a whole-voxel translation: every observed voxel of out_dump
    is the source voxel whose centre T carries onto it and vice versa (centre (i + 0.5) voxel_length; exact in float64 for such T) -
    weights and colour sums exactly, tsdf within 2^-23."""
    T = np.asarray(T, np.float64)
    gi, t, w, c = observed_voxels(out_dump)
    sgi, st, sw, sc = observed_voxels(src_dump)
    assert len(gi) == len(sgi) > 0, (what, len(gi), len(sgi))
    moved = (sgi.astype(np.float64) + 0.5) @ T[:3, :3].T + T[:3, 3] / voxel_length - 0.5
    assert np.abs(moved - np.rint(moved)).max() < 1e-6, (what, "not a whole-voxel permutation")
    moved = np.rint(moved).astype(np.int64)
    a = np.lexsort(gi.T[::-1])
    b = np.lexsort(moved.T[::-1])
    np.testing.assert_array_equal(gi[a], moved[b], err_msg=what)
    np.testing.assert_array_equal(w[a], sw[b], err_msg=what)
    np.testing.assert_array_equal(c[a], sc[b], err_msg=what)
    err = float(np.abs(t[a].astype(np.float64) - st[b].astype(np.float64)).max())
    assert err <= 2.0 ** -23, (what, err)
    assert (np.asarray(out_dump[2]).reshape(len(out_dump[0]), -1).max(axis=1) > 0).all(), what  # no all-zero unit is left behind
    return err


def fragile_share(ref_dump, detail):
    """Share of the voxels of a restated merge's result that sit on a boundary of the rules (the figure
    tests/test_gpu_tsdf_merge.py::assert_matches_restatement caps)."""
    fragile = np.zeros(np.asarray(ref_dump[2]).shape, bool)
    index = {tuple(k): i for i, k in enumerate(np.asarray(ref_dump[0]).tolist())}
    for j, k in enumerate(detail["keys"].tolist()):
        if tuple(k) in index:
            fragile[index[tuple(k)]] = detail["fragile"][j]
    return float(fragile.mean()) if fragile.size else 0.0


@pytest.mark.parametrize("shift", [(0, 0, 0), tuple(SHIFT)])
def test_whole_voxel_shift_reproduces_the_source(shift):
    src = tiny_dump()
    out, stats = merge_reference(empty_dump(), src, translation(shift, 0.02), 0.02)
    err = assert_is_shifted_source(out, src, np.array(shift), f"shift {shift}")
    held = int((np.asarray(src[2]).max(axis=1) > 0).sum())
    print(f"shift {shift}: stats {stats}, tsdf err {err:.3g}")
    assert stats[0] == held and stats[1] == len(out[0]) and stats[2] == stats[3] + stats[4] == int((np.asarray(out[2]) > 0).sum())
    if shift == (0, 0, 0):  # the identity keeps the units that hold a weight, where they are
        np.testing.assert_array_equal(out[0], np.asarray(src[0])[np.asarray(src[2]).max(axis=1) > 0])


def test_merge_into_a_map_adds_observation_counts():
    """Identity into a non-empty destination: weights add, colour sums add, tsdf is the weighted mean - and the source is not
    changed by the call (the restatement copies)."""
    a, b = tiny_dump(0, 4), tiny_dump(2, 4)
    b_before = tuple(np.array(x, copy=True) for x in b)
    out, stats = merge_reference(a, b, np.eye(4), 0.02)
    for x, y in zip(b, b_before):
        np.testing.assert_array_equal(x, y)
    gi, t, w, c = observed_voxels(out)
    grid_a, grid_b = rr._Grid(a), rr._Grid(b)
    ra, wa = grid_a.locate(gi[:, 0], gi[:, 1], gi[:, 2])
    rb, wb = grid_b.locate(gi[:, 0], gi[:, 1], gi[:, 2])
    w_a = np.where(ra >= 0, grid_a.weight[np.maximum(ra, 0), wa], 0).astype(np.float64)
    w_b = np.where(rb >= 0, grid_b.weight[np.maximum(rb, 0), wb], 0).astype(np.float64)
    np.testing.assert_array_equal(w, w_a + w_b)
    t_a = np.where(ra >= 0, grid_a.tsdf[np.maximum(ra, 0), wa], 0).astype(np.float64)
    t_b = np.where(rb >= 0, grid_b.tsdf[np.maximum(rb, 0), wb], 0).astype(np.float64)
    assert np.abs(t - (t_a * w_a + t_b * w_b) / (w_a + w_b)).max() <= 2.0 ** -23
    assert stats[1] == len(out[0]) - len(a[0]) and stats[2] == int((w_b > 0).sum())
    assert set(map(tuple, a[0].tolist())) <= set(map(tuple, out[0].tolist()))


# ---- the closed-form scene at 640 x 480 ---------------------------------------------------------------------------------------
def fuse_closed_form(frame_ids, frame_of_map=None):
    """oracle.PortTsdf of the listed closed-form frames; frame_of_map = F: the map is held in the frame p_map = F p_scene."""
    import oracle

    vol = oracle.PortTsdf(cf.VOXEL, cf.TRUNC)
    frames = cf.frames()
    back = np.eye(4) if frame_of_map is None else rigid_inverse(frame_of_map)
    for i in frame_ids:
        depth, rgb, T = frames[i]
        vol.integrate(depth, rgb, cf.K, T @ back, 1.0, cf.DEPTH_TRUNC)
    return vol.dump()


def scores_in_frame(out, T_cw, dump, frame_of_map):
    """closed_form_scores for a cast of a map held in the frame p_map = F p_scene (cast at T_cw F^-1): the observed test looks the
    ground-truth point up at F p, the normals are turned back into the scene's frame."""
    F = np.asarray(frame_of_map, np.float64)
    gt, _ = cf.render(T_cw)
    fx, fy, cx, cy = cf.K
    T_wc = np.linalg.inv(T_cw)
    v, u = np.mgrid[0:cf.H, 0:cf.W].astype(np.float64)
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ T_wc[:3, :3].T
    o = T_wc[:3, 3]
    p = o + gt[..., None].astype(np.float64) * d
    grid = rr._Grid(dump)
    gv = np.floor((p @ F[:3, :3].T + F[:3, 3]) / cf.VOXEL).astype(np.int64)
    row, word = grid.locate(gv[..., 0], gv[..., 1], gv[..., 2])
    observed = (gt > 0) & (row >= 0) & (grid.weight[np.maximum(row, 0), word] > THR)
    mask = np.asarray(out["mask"], bool)
    both = mask & (gt > 0)
    dz = np.abs(np.asarray(out["depth"], np.float64) - gt)[both] / cf.VOXEL
    on_sphere = np.abs(np.linalg.norm(p - cf.SPHERE_C, axis=-1) - cf.SPHERE_R) < np.abs(p @ cf.PLANE_N - cf.PLANE_D)
    n_gt = np.where(on_sphere[..., None], (p - cf.SPHERE_C) / cf.SPHERE_R, cf.PLANE_N)
    n_gt = n_gt * np.sign(((o - p) * n_gt).sum(-1))[..., None]
    n_out = np.asarray(out["normal"], np.float64) @ F[:3, :3]  # rows n_map -> F^T n_map
    ang = np.degrees(np.arccos(np.clip((n_out * n_gt).sum(-1), -1.0, 1.0)))[both]
    return {"hit_frac": float((mask & observed).sum() / observed.sum()), "dz_median": float(np.median(dz)),
            "dz_p99": float(np.percentile(dz, 99)), "normal_median_deg": float(np.median(ang)), "hits": int(mask.sum())}


def cast_and_score(dump, frame_of_map=None):
    F = np.eye(4) if frame_of_map is None else frame_of_map
    out = []
    for T in CAST_POSES:
        cast = rr.ray_cast(dump, cf.VOXEL, cf.TRUNC, cf.K, T @ rigid_inverse(F), cf.H, cf.W, 0.1, 3.0, THR)
        out.append(scores_in_frame(cast, T, dump, F))
    return out


def fmt(scores):
    return "  ".join("%.2f%% %.3f/%.2f" % (100 * s["hit_frac"], s["dz_median"], s["dz_p99"]) for s in scores)


@pytest.fixture(scope="module")
def direct():
    dump = fuse_closed_form((0, 1, 2))
    return dump, cast_and_score(dump)


@pytest.fixture(scope="module")
def moved(direct):
    return merge_reference(empty_dump(), direct[0], GENERIC, cf.VOXEL)


def check_against_direct(merged, direct_scores, what):
    """The fused-field bars; where the directly fused map itself misses the p99 bar at a pose, the merged map is held to the direct
    map's p99 plus 1.5 x the gap measured when the thresholds were set (docstring) instead."""
    for i, (m, d) in enumerate(zip(merged, direct_scores)):
        if d["dz_p99"] > 1.0:
            assert m["hit_frac"] >= 0.97 and m["dz_median"] <= 0.2 and m["normal_median_deg"] <= 3.0, (what, i, m)
            assert m["dz_p99"] <= d["dz_p99"] + 1.5 * P99_GAP_WHERE_DIRECT_MISSES, (what, i, m, d)
        else:
            check_closed_form_scores(m)


P99_GAP_WHERE_DIRECT_MISSES = 0.0  # (no pose of the directly fused map misses a bar: see the docstring)


def test_scores_in_frame_is_closed_form_scores_for_the_identity(direct):
    dump, _ = direct
    T = cf.POSES[0]
    cast = rr.ray_cast(dump, cf.VOXEL, cf.TRUNC, cf.K, T, cf.H, cf.W, 0.1, 3.0, THR)
    a, b = scores_in_frame(cast, T, dump, np.eye(4)), closed_form_scores(cast, T, dump, THR)
    for k, v in b.items():
        assert a[k] == pytest.approx(v, rel=1e-12, abs=1e-12), k


def test_generic_transform_on_the_closed_form_scene(direct, moved):
    dump, direct_scores = direct
    merged, stats = moved
    scores = cast_and_score(merged, GENERIC)
    print("direct  ", fmt(direct_scores))
    print("moved   ", fmt(scores), "stats", stats)
    for s in direct_scores:
        check_closed_form_scores(s)
    check_against_direct(scores, direct_scores, "moved map")
    assert stats[1] == len(merged[0]) and stats[2] == stats[3] + stats[4]
    assert (np.asarray(merged[2]).max(axis=1) > 0).all()  # no all-zero unit


def test_two_overlapping_maps_in_different_frames(direct):
    _, direct_scores = direct
    a = fuse_closed_form((0, 1))
    b = fuse_closed_form((2,), frame_of_map=OTHER)
    merged, stats = merge_reference(a, b, rigid_inverse(OTHER), cf.VOXEL)
    scores = cast_and_score(merged)
    print("direct  ", fmt(direct_scores))
    print("joined  ", fmt(scores), "stats", stats)
    check_against_direct(scores, direct_scores, "joined maps")
    for m, d in zip(scores, direct_scores):
        assert abs(m["hits"] - d["hits"]) <= 1e-3 * d["hits"], (m["hits"], d["hits"])


def test_round_trip_reports_the_resampling_error(direct, moved):
    """T, then T^-1, into fresh volumes: no bar - the figure goes into DESIGN.md (every merge resamples once)."""
    dump, _ = direct
    back, _ = merge_reference(empty_dump(), moved[0], rigid_inverse(GENERIC), cf.VOXEL)
    gi, t, w, _ = observed_voxels(back)
    grid = rr._Grid(dump)
    row, word = grid.locate(gi[:, 0], gi[:, 1], gi[:, 2])
    both = (row >= 0) & (grid.weight[np.maximum(row, 0), word] > 0)
    err = np.abs(t.astype(np.float64) - grid.tsdf[np.maximum(row, 0), word].astype(np.float64))[both]
    n_src = int((np.asarray(dump[2]) > 0).sum())
    print("round trip: %d of %d observed voxels observed in both, |d tsdf| median %.4f p99 %.4f max %.4f (x sdf_trunc / voxel: %.2f / %.2f / %.2f voxel)"
          % (both.sum(), n_src, np.median(err), np.percentile(err, 99), err.max(), np.median(err) * 8, np.percentile(err, 99) * 8, err.max() * 8))
    assert both.sum() > 0.8 * n_src
