"""Inputs shared by the CPU and GPU tests of the cross-view consistency check (tests/depth_consistency_reference.py is the
restatement they are held to)."""
import numpy as np

from pyslam_amd.prep import consistency_views
from tests import depth_consistency_reference as dr
from tests import mvs_cases as mc

F = np.float32
# the tile edges of the kernel's 64 x 4 pixel block (part of a wave, one wave and a pixel, several blocks along x and along y), one
# row and one column
SHAPES = ((1, 50), (50, 1), (7, 9), (5, 65), (37, 83), (3, 257))
BAD_VALUES = (0.0, -1.5, np.nan, np.inf, -np.inf)


def smooth_depth(rng, H, W):
    """A slanted, gently waved surface between about 1.2 and 3.8 m"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    a, b, ph = rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(0, 6.28)
    return 2.5 + a * (x / max(W - 1, 1) - 0.5) + b * (y / max(H - 1, 1) - 0.5) + 0.3 * np.sin(ph + 5.0 * x / max(W, 8) + 3.0 * y / max(H, 8))


def random_case(H, W, N, seed=0):
    """A smooth reference depth and N sources: the reference surface as each source camera sees it (a small rotation and translation
    away, sized in pixels so that a thin image keeps its sources in sight and loses a margin of it), then planted noise: a sixth of a
    source's pixels moved nearer (occluded), a sixth moved farther (violated), a twelfth emptied with 0, negative, NaN and infinite
    values; the same bad values in a twelfth of the reference.  -> (depth [H,W], sources [N,H,W], views, back_views, K, T_ref, T_sources)"""
    rng = np.random.default_rng(1000 * H + 10 * W + N + 7919 * seed)
    f = float(max(H, W, 16))
    K = np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    z = smooth_depth(rng, H, W)
    T_ref = np.eye(4)
    T_src = []
    for s in range(N):
        sx = (1, -1, 1, -1)[s] * min(W / 6.0, 6.0) * rng.uniform(0.6, 1.0)  # the shift of the image in pixels, by rotation
        sy = (1, 1, -1, -1)[s] * min(H / 6.0, 4.0) * rng.uniform(0.6, 1.0)
        r = np.array([-sy / f, sx / f, rng.uniform(-1.0, 1.0) * min(0.5 / max(H, W), 0.01)])
        R = np.eye(3) + np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
        U, _, Vt = np.linalg.svd(R)
        T = np.eye(4)
        T[:3, :3] = U @ Vt
        T[:3, 3] = np.array([0.5 * sx * 2.5 / f, 0.5 * sy * 2.5 / f, 0.02]) * rng.uniform(-1.0, 1.0, 3)  # parallax: half of that at 2.5 m
        T_src.append(T)
    T_src = np.stack(T_src)
    views, back_views = consistency_views(K, T_ref, K, T_src)
    y, x = np.mgrid[0:H, 0:W]
    sources = np.zeros((N, H, W), F)
    for s in range(N):
        m = views[s].astype(np.float64)
        q = [m[i, 0] * x + m[i, 1] * y + m[i, 2] + m[i, 3] / z for i in range(3)]
        u, v = np.rint(q[0] / q[2]).astype(int), np.rint(q[1] / q[2]).astype(int)
        ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        filled = np.full((H, W), 2.5 * float(np.mean(q[2])))  # what no reference pixel lands on: a background near the surface
        filled[v[ok], u[ok]] = (z * q[2])[ok]
        kind = rng.permutation(H * W).reshape(H, W) % 12  # exact shares at every size: no class is left to chance
        filled = np.where(kind < 2, 0.7 * filled, np.where(kind < 4, 1.4 * filled, filled))
        bad = np.asarray(BAD_VALUES)[rng.integers(0, len(BAD_VALUES), (H, W))]
        sources[s] = np.where(kind == 4, bad, filled).astype(F)
    kind = rng.permutation(H * W).reshape(H, W) % 12
    depth = np.where(kind == 0, np.asarray(BAD_VALUES)[rng.integers(0, len(BAD_VALUES), (H, W))], z).astype(F)
    return np.ascontiguousarray(depth), np.ascontiguousarray(sources), views, back_views, K, T_ref, T_src


def class_shares(depth, sources, views, back_views, **kw):
    """The share of the (pixel, view) pairs in each class, by the restatement: agree, occluded, violated, unseen (a valid pixel the
    view does not see), empty (seen, and the source has no depth there) - and the share of pixels that are invalid on input"""
    _, counts, _, parts = dr.depth_consistency(depth, sources, views, back_views, return_parts=True, **kw)
    n = float(depth.size * len(sources))
    c = counts.astype(np.int64).sum(axis=(0, 1))
    unseen = sum(int((parts["valid"] & ~p["seen"]).sum()) for p in parts["views"])
    empty = sum(int((p["seen"] & ~p["has"]).sum()) for p in parts["views"])
    return dict(agree=c[0] / n, occluded=c[1] / n, violated=c[2] / n, unseen=unseen / n, empty=empty / n, invalid=float((~parts["valid"]).mean()))


def shift_view(bx=0.0, by=0.0, bz=0.0, x0=0.0, y0=0.0):
    """u = (x + x0 + w bx) / (1 + w bz), v = (y + y0 + w by) / (1 + w bz): every entry exact in float32"""
    return np.array([[1, 0, x0, bx], [0, 1, y0, by], [0, 0, 1, bz]], F)


IDENTITY = shift_view()
ULP = lambda v, toward: np.nextafter(F(v), F(toward))


def planted():
    """The rule edges, each a few pixels with matrices whose products are exact in float32.
    -> [(name, depth, sources, views, back_views, arguments, check)]: check(out, counts, parts) asserts, on the restatement's result,
    that the case sits on the edge it is planted for."""
    cases = []

    # C2: u = x + w / 2.  Row 0 (z = 1, w = 1): a tie at every x, rounded to even - 0.5 -> 0, 1.5 -> 2, ..., 6.5 -> 6, and 7.5 -> 8,
    # past W - 1 = 7.  Row 1 (z = 2): u = x + 0.25 -> x, and x = 7 lands on W - 1 itself.  The source holds the same depths, the way
    # back is the inverse: every seen pixel whose source pixel holds its own row's depth agrees
    H, W = 2, 8
    depth = np.array([[1.0] * W, [2.0] * W], F)

    def check_ties(out, counts, parts):
        p = parts["views"][0]
        np.testing.assert_array_equal(p["ur"][0][:7], [0, 2, 2, 4, 4, 6, 6])
        assert not p["seen"][0, 7] and p["seen"][1].all() and p["ur"][1, 7] == 7
        assert (counts[0, :7, 3] == 1).all() and counts[0, 7].tolist() == [0, 0, 0, 0] and out[0, 7] == 0

    cases.append(("ties_and_the_right_edge", depth, depth[None].copy(), shift_view(bx=0.5)[None], shift_view(bx=-0.5)[None],
                  dict(max_reproj_error=1.0, inv_depth_tol=0.0, rel_depth_tol=0.01), check_ties))

    # C2: q_2 = 1 - w is 0 at z = 1, negative at z = 0.5, 0.5 at z = 2 (then u = 2 x).  C3: q'_2 = 1 - ws is 0 where the source holds
    # d = 1 and negative where it holds 0.5
    depth = np.array([[1.0, 0.5, 2.0, 2.0, 2.0, 2.0]], F)
    source = np.array([[4.0, 1.0, 0.5, 9.0, 1.0, 9.0]], F)  # x = 2 reads pixel 4 (d = 1), x = 1 would read pixel 2

    def check_behind(out, counts, parts):
        p = parts["views"][0]
        assert p["seen"][0].tolist() == [False, False, True, False, False, False] and p["ur"][0, 2] == 4  # (x = 3.. land past W - 1)
        assert p["q2"][0, 2] == 0 and counts[0, 2].tolist() == [0, 0, 1, 1] and out[0, 2] == 0  # d = 1 = zs: violated

    cases.append(("behind_the_source_camera", depth, source[None], shift_view(bz=-1.0)[None], shift_view(bz=-1.0)[None],
                  dict(max_reproj_error=1.0, inv_depth_tol=0.5, rel_depth_tol=0.0), check_behind))
    depth = np.full((1, 4), 2.0, F)
    source = np.array([[1.0, 0.5, 2.0, 0.25]], F)

    def check_behind_back(out, counts, parts):
        p = parts["views"][0]
        assert p["seen"].all() and p["q2"][0].tolist() == [0.0, -1.0, 0.5, -3.0]
        # with tolerances this wide only q'_2 <= 0 keeps a view from agreeing; those sources hold nearer depths: occluded
        assert counts[0, :, 0].tolist() == [0, 0, 1, 0] and counts[0, :, 1].tolist() == [1, 1, 0, 1] and (counts[0, :, 2] == 0).all()

    cases.append(("behind_the_reference_camera", depth, source[None], IDENTITY[None], shift_view(bz=-1.0)[None],
                  dict(max_reproj_error=100.0, inv_depth_tol=100.0, rel_depth_tol=0.0), check_behind_back))

    # C4: the way back lands (0.5, 0) away through view 0: e2 = 0.25 = 0.5 * 0.5 exactly, and (0.5, 3 * 2^-14) away through view 1:
    # e2 = 0.25 + 1.125 * 2^-25, which rounds to one ulp above 0.25
    depth = np.full((3, 5), 1.5, F)
    backs = np.stack([shift_view(x0=0.5), shift_view(x0=0.5, y0=3.0 * 2.0 ** -14)])

    def check_e2(out, counts, parts):
        a, b = parts["views"]
        assert (a["e2"] == F(0.25)).all() and (b["e2"] == ULP(0.25, 1)).all() and parts["max_e2"] == F(0.25)
        assert a["agree"].all() and b["violated"].all() and (counts == [1, 0, 1, 2]).all()

    cases.append(("reprojection_at_the_bound", depth, np.stack([depth, depth]), np.stack([IDENTITY, IDENTITY]), backs,
                  dict(max_reproj_error=0.5, inv_depth_tol=0.0, rel_depth_tol=0.01, max_violations=1), check_e2))

    # C4: z = 1 against d = 2: |0.5 - 1| = 0.5 = inv_depth_tol; against the float above 2: wb = 0.5 - 2^-24, |wb - w| = 0.5 + 2^-24,
    # one ulp beyond.  The same with the relative tolerance alone, 0.5 * w
    depth = np.ones((1, 2), F)
    source = np.array([[2.0, ULP(2.0, 3)]], F)

    def check_tol(out, counts, parts):
        p = parts["views"][0]
        assert np.abs(p["wb"] - parts["w"])[0].tolist() == [0.5, float(ULP(0.5, 1))] and (parts["tol"] == F(0.5)).all()
        assert counts[0].tolist() == [[1, 0, 0, 1], [0, 0, 1, 1]] and out[0].tolist() == [1.5, 0.0]

    for name, kw in (("inverse_depth_at_the_bound", dict(inv_depth_tol=0.5, rel_depth_tol=0.0)), ("relative_depth_at_the_bound", dict(inv_depth_tol=0.0, rel_depth_tol=0.5))):
        cases.append((name, depth, source[None], IDENTITY[None], IDENTITY[None], dict(max_reproj_error=1.0, **kw), check_tol))

    # C5: the source holds exactly the predicted depth and the way back lands 5 pixels off: d == zs is violated, not occluded; the
    # float below zs is occluded
    depth = np.full((1, 3), 3.0, F)
    source = np.array([[3.0, ULP(3.0, 0), ULP(3.0, 4)]], F)

    def check_equal(out, counts, parts):
        assert (parts["views"][0]["zs"] == F(3.0)).all() and counts[0].tolist() == [[0, 0, 1, 1], [0, 1, 0, 1], [0, 0, 1, 1]]

    cases.append(("predicted_depth_met_exactly", depth, source[None], IDENTITY[None], shift_view(x0=5.0)[None],
                  dict(max_reproj_error=1.0, inv_depth_tol=0.0, rel_depth_tol=0.01, min_consistent=0, max_violations=1), check_equal))

    # C7: z = 1, then 2^24, then 1: (1 + 2^24) + 1 = 2^24 in float32 in ascending s, 2^24 + 2 the other way round
    depth = np.ones((1, 1), F)
    sources = np.array([[[2.0 ** 24]], [[1.0]]], F)

    def check_order(out, counts, parts):
        assert counts[0, 0].tolist() == [2, 0, 0, 2] and out[0, 0] == F(2.0 ** 24) / F(3.0) and out[0, 0] != (F(2.0 ** 24) + F(2.0)) / F(3.0)

    cases.append(("fusion_in_ascending_order", depth, sources, np.stack([IDENTITY, IDENTITY]), np.stack([IDENTITY, IDENTITY]),
                  dict(max_reproj_error=1.0, inv_depth_tol=10.0, rel_depth_tol=0.0, min_consistent=2), check_order))
    return cases


def rule_settings(N):
    """The settings of C6 and C7 that the random case is run with: min_consistent 0, 1 and N, max_violations 0 and N, fuse on and off"""
    return [dict(min_consistent=a, max_violations=b, fuse=f) for a in sorted({0, 1, N}) for b in (0, N) for f in (True, False)]


# ---- the synthetic room: the plane-sweep depth of pose 150 checked against the plane-sweep depths of poses 140 and 130, each made
# with mvs_cases.TRUTH_PARAMS from its own two earlier poses at spacing 10
TRUTH_POSES = (mc.TRUTH_POSE, mc.TRUTH_POSE - mc.TRUTH_SPACING, mc.TRUTH_POSE - 2 * mc.TRUTH_SPACING)
TRUTH_PLANE_STEP = (1.0 / mc.TRUTH_PARAMS["min_depth"]) / (mc.TRUTH_PARAMS["num_planes"] - 1)  # (max_depth is infinite)
TRUTH_CHECK = dict(max_reproj_error=1.0, inv_depth_tol=TRUTH_PLANE_STEP, rel_depth_tol=0.0, min_consistent=1, max_violations=0, fuse=True)
# (share of valid pixels, share of them off by more than one plane step, median error in plane steps) of the restatement, after the
# check with fusion; mvs_cases.TRUTH_MEASURED holds the same figures before it
TRUTH_MEASURED = (0.5092, 0.0148, 0.1929)
TRUTH_MEASURED_NOT_FUSED = (0.5092, 0.0255, 0.2533)


def depth_figures(depth, depth_true):
    """mvs_cases.truth_figures for a depth map (0 = none): valid share, share of the valid off by more than one plane step, median
    error in plane steps, all in inverse depth"""
    depth = np.asarray(depth, np.float64)
    valid = depth > 0
    err = np.abs(1.0 / depth[valid] - 1.0 / np.asarray(depth_true, np.float64)[valid]) / TRUTH_PLANE_STEP
    return float(valid.mean()), float((err > 1.0).mean()), float(np.median(err))


def truth_frames():
    """-> (stream, [(rgb, true depth, T_cw, rgb of the two sources [2,H,W,3], T_cw of the two sources [2,4,4]) for TRUTH_POSES])"""
    out, s = [], None
    for i in TRUTH_POSES:
        rgb, sources, depth, T, T_src, s = mc.synthetic_triple(i)
        out.append((rgb, depth, T, sources, T_src))
    return s, out
