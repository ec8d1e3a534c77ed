"""CPU: the planted voxel states of tests/planted_states.py and the conditions the GPU tests built on them rely on
(tests/test_gpu_tsdf_merge_edges.py, tests/test_gpu_tsdf_raycast_edges.py, tests/test_gpu_tsdf_deintegrate_planted.py,
tests/test_gpu_tsdf_prune_planted.py).  No GPU.

The two restatements (tests/merge_reference.py, tests/raycast_reference.py) are run on every planted input and held to what can
be known without them - exact permutations, the analytic depth and normal of the planted walls - before the GPU is held to them;
the figures they give are asserted, so a change of a builder shows up here first.

Measured when the file was written (voxel 0.02, sdf_trunc 0.08):
    sparse source (26 units), empty destination: stats (units_source, units_claimed, voxels_updated, trilinear, nearest)
        diagonal (26, 92, 95817, 42139, 53678), 129 candidates   z45 (26, 95, 95828, 42056, 53772), 102 candidates
        diag60 (26, 94, 95818, 42120, 53698), 134 candidates     y179 (26, 82, 95908, 42130, 53778), 101 candidates
        generic (26, 82, 95873, 42186, 53687), 90 candidates     far (26, 84, 95841, 42093, 53748), 92 candidates
      fragile share 0.0 for every one of them, into the empty and into the overlapping destination; < 0.4 s per restated merge
    six viewing directions, 32 x 24: 712-753 hits, 484-553 interior rays, every interior ray hit, |dz| <= 6e-8 m, normal error 0;
      without the 2-voxel margin 96.3-99.9 % of the hits are within 1e-4 m of a wall
"""
import numpy as np
import pytest

from tests import deintegrate_reference as dr
from tests import merge_reference as mr
from tests import planted_states as ps
from tests import prune_reference as pr
from tests import raycast_reference as rr
from tests.test_merge_reference_cpu import GENERIC, assert_is_permuted_source, fragile_share, observed_voxels, rigid, rigid_inverse

SPARSE_TRANSFORMS = {name: rigid(axis, degrees, ps.MERGE_T) for name, (axis, degrees) in ps.WORST_CASE_ROTATIONS.items()}
SPARSE_TRANSFORMS["generic"] = GENERIC
SPARSE_TRANSFORMS["far"] = rigid((0.3, 1.0, 0.2), 23.0, ps.FAR_T)  # GENERIC's rotation, 250 km from the origin
SPARSE_STATS = {"diagonal": (26, 92, 95817, 42139, 53678), "z45": (26, 95, 95828, 42056, 53772), "diag60": (26, 94, 95818, 42120, 53698),
                "y179": (26, 82, 95908, 42130, 53778), "generic": (26, 82, 95873, 42186, 53687), "far": (26, 84, 95841, 42093, 53748)}
SPARSE_CANDIDATES = {"diagonal": 129, "z45": 102, "diag60": 134, "y179": 101, "generic": 90, "far": 92}
DESTINATION_SEED = 11
GENERIC_CAST = {"eye": (0.2, -1.1, 0.4), "target": (-0.2, -0.25, -0.2), "intr": (60.0, 60.0, 31.5, 23.5), "height": 48, "width": 64,
                "threshold": 0.5}
# depth ranges on two_walls(2, +1); the interior rays of the front wall take their bracket's samples at z in (0.4995, 0.5] and
# (0.5195, 0.52] (test_depth_range_cases_of_the_reference shows it)
DEPTH_MAX_SHORT, DEPTH_MIN_INSIDE, DEPTH_MIN_CLAMPS, DEPTH_MAX_BETWEEN, DEPTH_MAX_CLAMPS = 0.49, 0.52, 0.49, 0.51, 0.53


def look_at(eye, target, up=(0.1, 1.0, 0.2)):
    """T_cw of a camera at `eye` looking at `target` (a generic rotation: nothing about it is exact)."""
    z = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    T_wc = np.eye(4)
    T_wc[:3, 0], T_wc[:3, 1], T_wc[:3, 2], T_wc[:3, 3] = x, np.cross(z, x), z, eye
    return np.linalg.inv(T_wc)


def overlapping_destination(result_keys):
    """A destination that holds every second unit of a merge's result, with values of its own (the w0 > 0 update formula)."""
    return ps.random_units(ps.every_second_unit(result_keys), DESTINATION_SEED)


@pytest.fixture(scope="module")
def sparse():
    return ps.as_dump(ps.sparse_source())


# ---- builders ------------------------------------------------------------------------------------------------------------------
def test_builders_round_trip_through_the_oracle():
    """states -> oracle.PortTsdf.load_units -> dump() gives the states back; as_dump differs from them by at most the one float32
    rounding of the import's quotient."""
    states = ps.sparse_source()
    keys, tsdf, weight, colour = ps.to_oracle(states).dump()
    np.testing.assert_array_equal(keys, states[0])
    np.testing.assert_array_equal(tsdf.view(np.uint32), states[1].view(np.uint32))  # the sign of -0 included
    np.testing.assert_array_equal(weight, states[2])
    seen = states[2] > 0
    np.testing.assert_array_equal(colour[seen], states[3][seen])
    dump = ps.as_dump(states)
    assert len(keys) == 26 and (np.diff(np.asarray(keys, np.int64) @ [1 << 40, 1 << 20, 1]) > 0).all()
    np.testing.assert_array_equal(dump[2], weight)
    assert np.abs(dump[1].astype(np.float64) - tsdf).max() <= 2.0 ** -24
    assert 0.09 < (weight == 0).mean() < 0.11 and set(np.unique(weight)) == set(range(8))
    # every numerator but tsdf * weight is exact in the float32 payload
    for w in range(1, 8):
        c = np.arange(256, dtype=np.float32) * np.float32(w)
        assert np.array_equal(c.astype(np.float64), np.arange(256) * float(w))


def test_exact_inverse_poses():
    for axis, sign in ps.DIRECTIONS:
        T = ps.camera_pose(axis, sign)
        assert mr.check_rigid(T) is None and np.linalg.det(T[:3, :3]) == 1.0
        assert np.array_equal(np.linalg.inv(T), rigid_inverse(T)), (axis, sign)
        assert np.array_equal(np.linalg.inv(T)[:3, 3], ps.CAMERA) and np.array_equal(ps.CAMERA * 128, np.rint(ps.CAMERA * 128))
        assert np.array_equal(np.linalg.inv(T)[:3, 2], np.eye(3)[axis] * sign)
    for name, T in {**ps.EXACT_ROTATIONS, **ps.RIM_TRANSFORMS, "half": ps.HALF_SHIFT}.items():
        assert mr.check_rigid(T) is None and np.linalg.det(T[:3, :3]) == 1.0, name
        assert set(np.unique(np.abs(T[:3, :3]))) == {0.0, 1.0}, name


# ---- merge: sparse source under worst-case rotations -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SPARSE_TRANSFORMS))
def test_sparse_source_fragile_share_and_figures(sparse, name):
    T = SPARSE_TRANSFORMS[name]
    assert mr.check_rigid(T) is None
    ref, stats, detail = mr.merge_reference(mr.empty_dump(), sparse, T, ps.VOX, detail=True)
    share = fragile_share(ref, detail)
    kept = int(detail["updated"].any(axis=1).sum())
    print(f"{name}: stats {stats}, {len(detail['keys'])} candidates, {kept} kept, fragile share {share:.3g}")
    assert share <= 1e-4
    assert stats == SPARSE_STATS[name] and len(detail["keys"]) == SPARSE_CANDIDATES[name] and kept == stats[1] < len(detail["keys"])
    per_unit = detail["updated"].sum(axis=1)
    assert (per_unit == 0).any() and per_unit[per_unit > 0].min() < 16  # candidates probed and not kept; units kept for less than a row of voxels
    assert (np.asarray(ref[2]).max(axis=1) > 0).all()
    dst = ps.as_dump(overlapping_destination(ref[0]))
    ref2, stats2, detail2 = mr.merge_reference(dst, sparse, T, ps.VOX, detail=True)
    assert fragile_share(ref2, detail2) <= 1e-4
    assert stats2[1] == len(ref[0]) - len(dst[0]) == len(ref[0]) // 2 and stats2[2:] == stats[2:]
    np.testing.assert_array_equal(ref2[0], ref[0])
    both = (ref[2] > 0) & (ref2[2] > ref[2])  # updated voxels the destination had observed already
    assert both.sum() > 0.25 * stats[2] and not np.array_equal(ref2[1][both], ref[1][both])


def test_the_cube_diagonal_rotation_reaches_three_units_per_axis(sparse):
    """The candidate boxes of the diagonal rotation span 3 destination units on some axis (n[a] == 3 in k_merge_candidates)."""
    T = SPARSE_TRANSFORMS["diagonal"]
    held = sparse[0][sparse[2].max(axis=1) > 0].astype(np.int64)
    corners = np.stack([(held + np.array([c & 1, (c >> 1) & 1, c >> 2])) * ps.UNIT for c in range(8)], axis=1) @ T[:3, :3].T + T[:3, 3]
    lo = np.floor(np.ceil(corners.min(1) / ps.VOX - 0.5 - 1e-3) / 16)
    hi = np.floor(np.floor(corners.max(1) / ps.VOX - 0.5 + 1e-3) / 16)
    assert (hi - lo).max() == 2 and ((hi - lo) == 2).all(axis=1).any()  # a full 3 x 3 x 3 for some unit


def test_huge_translations_update_nothing(sparse):
    for x in (2.1e7, 1.0e8):
        T = np.eye(4)
        T[0, 3] = x
        assert x / ps.VOX >= 1.0e9 and mr.merge_reference(mr.empty_dump(), sparse, T, ps.VOX)[1] == (26, 0, 0, 0, 0)


# ---- merge: exact rotations ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.EXACT_ROTATIONS))
def test_exact_rotations(sparse, name):
    T = ps.EXACT_ROTATIONS[name]
    ref, stats = mr.merge_reference(mr.empty_dump(), sparse, T, ps.VOX)
    print(f"{name}: stats {stats}")
    if name.endswith("half"):
        assert stats == (26, 52, 95689, 42119, 53570)
        return
    assert stats[2] == int((sparse[2] > 0).sum()) == 95866
    assert_is_permuted_source(ref, sparse, T, ps.VOX, name)
    # the restatement's nearest voxel is the exact permuted index, and r stays within 1e-13 of the lattice (|g| < 128 voxels here:
    # the few roundings behind g are each at most ulp(128) / 2 = 1.4e-14), five orders inside merge_reference.FRAGILE_BAND
    sgi = observed_voxels(sparse)[0]
    g0, r, ok = mr.locate(T, ps.permuted_index(T, sgi), ps.VOX)
    assert ok.all()
    near = np.stack([g0[a] + (r[a] >= 0.5) for a in range(3)], axis=-1)
    np.testing.assert_array_equal(near, sgi)
    off = max(float(np.minimum(r[a], 1.0 - r[a]).max()) for a in range(3))
    print(f"{name}: |r| off the lattice <= {off:.3g}")
    assert off <= 1e-13


# ---- merge: single voxels, the rim ---------------------------------------------------------------------------------------------------
SINGLE_TRANSFORMS = {"identity": np.eye(4), "diagonal": SPARSE_TRANSFORMS["diagonal"], "half": ps.HALF_SHIFT}
SINGLE_EXPECTED = {("face", "diagonal"): (2, 2), ("face", "half"): (0, 0)}  # (voxels, units); every other case (1, 1)


@pytest.mark.parametrize("transform", list(SINGLE_TRANSFORMS))
@pytest.mark.parametrize("source", list(ps.SINGLE_VOXELS))
def test_single_voxel_sources(source, transform):
    src = ps.as_dump(ps.single_voxel(*ps.SINGLE_VOXELS[source]))
    ref, stats, detail = mr.merge_reference(mr.empty_dump(), src, SINGLE_TRANSFORMS[transform], ps.VOX, detail=True)
    voxels, units = SINGLE_EXPECTED.get((source, transform), (1, 1))
    if transform == "diagonal":  # (the other two put every voxel on a boundary by construction)
        assert fragile_share(ref, detail) == 0.0
    assert stats == (1, units, voxels, 0, voxels) and len(ref[0]) == units and int((ref[2] > 0).sum()) == voxels
    if voxels:
        assert set(np.unique(ref[2])) == {0.0, 5.0} and set(np.unique(ref[1])) == {0.0, 0.25}


RIM_EXPECTED = {"identity": 3, "x+16": 1, "z-3": 4}  # units the three rim units end in (the alias unit adds its own)


@pytest.mark.parametrize("name", list(ps.RIM_TRANSFORMS))
def test_rim_of_the_key_range(name):
    T = ps.RIM_TRANSFORMS[name]
    plain, stats = mr.merge_reference(mr.empty_dump(), ps.as_dump(ps.rim_source(alias=False)), T, ps.VOX)
    assert stats[:2] == (3, RIM_EXPECTED[name]) and np.abs(plain[0]).max() <= ps.B
    ref, stats = mr.merge_reference(mr.empty_dump(), ps.as_dump(ps.rim_source(alias=True)), T, ps.VOX)
    alone, _ = mr.merge_reference(mr.empty_dump(), ps.as_dump(ps.random_units(np.array([ps.RIM_ALIAS]), 7)), T, ps.VOX)
    assert stats[0] == 4 and len(ref[0]) == len(plain[0]) + len(alone[0])
    # the alias unit feeds no voxel that is not its own: the units of the other three are what they are without it
    rows = [i for i, k in enumerate(ref[0].tolist()) if tuple(k) in set(map(tuple, plain[0].tolist()))]
    for a, b in zip(plain[1:3], ref[1:3]):
        np.testing.assert_array_equal(a, b[rows])
    assert ps.B * 16 + 15 < 2 ** 24 + 2 ** 4  # every voxel index is exact in float32, let alone float64


def test_merging_twice_doubles_the_observations(sparse):
    T = GENERIC
    once, _ = mr.merge_reference(mr.empty_dump(), sparse, T, ps.VOX)
    twice, stats = mr.merge_reference(once, sparse, T, ps.VOX)
    assert stats[1] == 0
    assert_doubled(once, twice)


def assert_doubled(once, twice):
    """Weights and colour sums exactly double; tsdf moves by at most one float32 rounding."""
    np.testing.assert_array_equal(once[0], twice[0])
    np.testing.assert_array_equal(twice[2], 2 * once[2])
    s1 = np.rint(np.asarray(once[3], np.float64) * np.asarray(once[2], np.float64)[..., None])
    s2 = np.rint(np.asarray(twice[3], np.float64) * np.asarray(twice[2], np.float64)[..., None])
    np.testing.assert_array_equal(s2, 2 * s1)
    assert np.abs(twice[1].astype(np.float64) - once[1].astype(np.float64)).max() <= 2.0 ** -23


# ---- ray cast ------------------------------------------------------------------------------------------------------------------------
def cast(dump, T, depth_min=0.1, depth_max=3.0, threshold=3.0, **kw):
    return rr.ray_cast(dump, ps.VOX, ps.TRUNC, ps.INTR, T, ps.H, ps.W, depth_min, depth_max, threshold, **kw)


def check_interior_rays(out, scene, what):
    """Every interior ray returns its wall's depth within 1e-4 m and its normal within 0.5 deg.  -> number of interior rays."""
    depth, interior, normal = ps.analytic_walls(scene)
    assert out["mask"][interior].all(), (what, "an interior ray missed")
    dz = np.abs(out["depth"].astype(np.float64) - depth)[interior]
    ang = np.degrees(np.arccos(np.clip(out["normal"].astype(np.float64)[interior] @ normal, -1.0, 1.0)))
    print(f"{what}: {int(out['mask'].sum())} hits, {int(interior.sum())} interior rays, max |dz| {dz.max():.3g} m, max normal error {ang.max():.3g} deg")
    assert dz.max() <= 1e-4 and ang.max() <= 0.5, (what, float(dz.max()), float(ang.max()))
    return int(interior.sum())


@pytest.mark.parametrize("axis,sign", ps.DIRECTIONS)
def test_six_viewing_directions_interior_rays_are_exact(axis, sign):
    states, scene = ps.two_walls(axis, sign)
    dump = ps.as_dump(states)
    assert len(dump[0]) == 11 and not (np.asarray(dump[0])[:, axis] == (0 if sign > 0 else -1)).any()  # nothing next to the camera
    out = cast(dump, ps.camera_pose(axis, sign))
    n = check_interior_rays(out, scene, f"axis {axis} sign {sign:+d}")
    depth, interior, _ = ps.analytic_walls(scene)
    assert n >= 480 and (depth[interior] == ps.FRONT).sum() >= 390 and (depth[interior] == ps.BACK).sum() >= 45
    assert 700 <= out["mask"].sum() <= 760
    # the centre column and row are rays with a zero direction component; they run along the hole's edge, so part of them is interior
    assert interior[:, 16].sum() >= 5 and interior[12, :].sum() >= 5


@pytest.fixture(scope="module")
def patterned():
    states, scene = ps.two_walls(2, 1)
    return ps.as_dump(ps.weight_pattern(states, scene)), scene


def check_weight_pattern(outs, scene):
    """outs: casts of the patterned scene at thresholds 2.5, 3.0, 4.0."""
    depth, interior, _ = ps.analytic_walls(scene)
    behind = ps.behind_the_front_wall(scene)
    weak, split = (ps.front_columns(scene, c) & behind for c in (ps.WEAK_COLUMNS, ps.SPLIT_COLUMNS))
    rest = interior & ~ps.front_columns(scene, (ps.SPLIT_COLUMNS[0], ps.WEAK_COLUMNS[1]), margin_voxels=-2.0)
    assert weak.sum() >= 10 and split.sum() >= 10 and rest.sum() >= 100
    check_interior_rays(outs[2.5], scene, "threshold 2.5")  # a weight of 3 is observed: the plain scene
    o = outs[3.0]
    for name, rays in (("weak", weak), ("split", split)):
        assert o["mask"][rays].all() and np.abs(o["depth"][rays] - ps.BACK).max() <= 1e-4, name  # the surface behind is found instead
    assert np.abs(o["depth"].astype(np.float64) - depth)[rest].max() <= 1e-4
    assert not outs[4.0]["mask"].any()
    return int(o["mask"].sum())


def test_weight_threshold_pattern_on_the_reference(patterned):
    dump, scene = patterned
    assert set(np.unique(dump[2])) == {0.0, 3.0, 4.0}
    outs = {thr: cast(dump, ps.camera_pose(2, 1), threshold=thr) for thr in (2.5, 3.0, 4.0)}
    check_weight_pattern(outs, scene)
    assert outs[2.5]["mask"].sum() == 738 and (outs[3.0]["depth"] > 0.9).sum() > (outs[2.5]["depth"] > 0.9).sum() + 60


def check_depth_range_cases(outs, scene):
    """outs: casts of two_walls(2, +1) keyed by (depth_min, depth_max)."""
    depth, interior, _ = ps.analytic_walls(scene)
    front = interior & (depth == ps.FRONT)
    behind = ps.behind_the_front_wall(scene)
    assert not outs[(0.1, DEPTH_MAX_SHORT)]["mask"].any()
    o = outs[(DEPTH_MIN_INSIDE, 3.0)]  # a start inside the front wall: it is not reported, the back wall is
    assert o["mask"][behind].all() and np.abs(o["depth"][behind] - ps.BACK).max() <= 1e-4 and o["depth"][o["mask"]].min() > 0.9
    o = outs[(DEPTH_MIN_CLAMPS, 3.0)]  # the bracket's near end cannot move a voxel outwards: max(z_prev - voxel, depth_min)
    assert o["mask"][front].all() and np.abs(o["depth"][front] - ps.FRONT).max() <= 1e-4
    assert not outs[(0.1, DEPTH_MAX_BETWEEN)]["mask"][front].any()  # depth_max between the bracket's two samples
    o = outs[(0.1, DEPTH_MAX_CLAMPS)]  # the bracket's far end is clamped: min(z + voxel, depth_max)
    assert o["mask"][front].all() and np.abs(o["depth"][front] - ps.FRONT).max() <= 1e-4


DEPTH_RANGES = ((0.1, DEPTH_MAX_SHORT), (DEPTH_MIN_INSIDE, 3.0), (DEPTH_MIN_CLAMPS, 3.0), (0.1, DEPTH_MAX_BETWEEN), (0.1, DEPTH_MAX_CLAMPS))


def test_depth_range_cases_of_the_reference():
    states, scene = ps.two_walls(2, 1)
    dump, T = ps.as_dump(states), ps.camera_pose(2, 1)
    check_depth_range_cases({r: cast(dump, T, *r) for r in DEPTH_RANGES}, scene)
    depth, interior, _ = ps.analytic_walls(scene)
    front = interior & (depth == ps.FRONT)
    # the far sample of every interior front ray's bracket lies in (0.5195, 0.5205], the near one a voxel before it
    assert not cast(dump, T, 0.1, 0.5195)["mask"][front].any() and cast(dump, T, 0.1, 0.5205)["mask"][front].all()
    assert 0.5205 - ps.VOX < DEPTH_MAX_BETWEEN <= 0.5195 and 0.5205 < DEPTH_MAX_CLAMPS < 0.5195 + ps.VOX
    scaled, plain = cast(dump, T, depth_scale=1000.0), cast(dump, T)
    np.testing.assert_array_equal(scaled["depth"], plain["depth"] * np.float32(1000.0))
    np.testing.assert_array_equal(scaled["vertex"], plain["vertex"])


def incomplete_hits(out, dump, threshold=3.0):
    """-> per hit (in row-major order of the mask): is the trilinear neighbourhood of its vertex incomplete?"""
    p = out["vertex"][out["mask"]]
    ok, _ = rr._tri_tsdf(rr._Grid(dump), [p[:, a] for a in range(3)], np.float32(ps.VOX), np.float32(threshold))
    return ~ok


def test_tilted_wall_at_a_missing_unit_on_the_reference():
    dump = ps.as_dump(ps.tilted_wall_at_a_missing_unit())
    assert dump[0].tolist() == [[0, -1, 0], [0, -1, 1], [0, 0, 0], [0, 0, 1]]
    out = cast(dump, ps.camera_pose(2, 1))
    bad = incomplete_hits(out, dump)
    fx, _, cx, _ = ps.INTR
    u = np.mgrid[0:ps.H, 0:ps.W][1].astype(np.float64)
    z_true = 0.8 * ps.FRONT / (0.6 * (u - cx) / fx + 0.8)  # the plane 0.6 x + 0.8 z = const through the point FRONT ahead
    dz = np.abs(out["depth"] - z_true)[out["mask"]]
    print(f"tilted wall: {int(out['mask'].sum())} hits, {int(bad.sum())} with an incomplete neighbourhood; |dz| complete {dz[~bad].max():.3g}, incomplete {dz[bad].max():.3g}")
    assert out["mask"].sum() == 408 and bad.sum() == 24
    assert dz[~bad].max() <= 1e-4 < dz[bad].max()  # an incomplete hit left the refinement early; the others are exact
    # colour of an incomplete hit: the nearest voxel's mean
    grid = rr._Grid(dump)
    p = out["vertex"][out["mask"]][bad]
    row, word = grid.locate(*(np.floor(p[:, a] / np.float32(ps.VOX)).astype(np.int64) for a in range(3)))
    np.testing.assert_array_equal(out["color"][out["mask"]][bad], grid.colour[row, word] / np.float32(255))


def test_generic_pose_sees_the_sparse_source():
    dump = ps.as_dump(ps.sparse_source(special=False))
    g = GENERIC_CAST
    out = rr.ray_cast(dump, ps.VOX, ps.TRUNC, g["intr"], look_at(g["eye"], g["target"]), g["height"], g["width"], 0.1, 3.0, g["threshold"])
    assert out["mask"].sum() == 1919


# ---- de-integration and prune targets --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.REMOVALS))
def test_deintegration_targets_hold_every_branch_inside_single_quads(name):
    """The conditions tests/test_gpu_tsdf_deintegrate_planted.py relies on, from the builders and the restatement alone: >= 200
    voxels in each branch of the removal rule, >= 50 quads (one lane's 16-byte access) that hold all three, >= 1 unit of the touch
    sets absent; the restatement's stats follow from the class counts; voxels no frame samples come back untouched."""
    s, frames, samples, states, scale, stride = ps.removal_case(name)
    dump = ps.as_dump(states)
    first = samples[:ps.CHUNK]
    n, csum, missing = ps.sample_counts(dump[0], first)
    under, fresh, rest = ps.removal_classes(dump[2], n)
    quads = ps.quads_with_all_classes(under, fresh, rest)
    print(f"{name}: {len(dump[0])} units, underflow {under.sum()}, fresh {fresh.sum()}, remaining {rest.sum()}, quads {quads}, missing {missing}")
    assert min(under.sum(), fresh.sum(), rest.sum()) >= 200 and quads >= 50 and missing >= 1
    assert dump[2].max() > 7 or len(samples) == 1
    after, stats = dr.deintegrate_reference(dump, first)
    assert stats == (sum(len(f.keys) for f in first), missing, int(n[fresh | rest].sum()), int(under.sum()))
    same = (n == 0) | under
    for a, b in zip(after[1:], dump[1:]):
        assert np.array_equal(a[same], b[same])
    assert np.all(after[2][fresh] == 0) and np.all(after[1][fresh] == 0) and np.all(after[3][fresh] == 0)
    np.testing.assert_array_equal(after[2][rest], (dump[2].astype(np.int64) - n)[rest])
    assert after[3].min() >= 0.0 and after[3].max() <= 255.0
    low, high = ps.clamp_ends(dump, n, csum)
    if ps.REMOVALS[name][3] == "foreign":
        assert low >= 100 and high >= 100, (low, high)
    elif len(samples) <= ps.CHUNK:
        assert (low, high) == (0, 0)  # consistent colours: the clamp never acts, the sums are those of the frames that remain
        left = np.rint(dump[3] * dump[2][..., None]).astype(np.int64) - csum
        np.testing.assert_array_equal(np.rint(after[3] * after[2][..., None]).astype(np.int64)[rest], left[rest])


def test_chunk_boundary_target_separates_the_per_chunk_decision_from_a_per_call_one():
    s, frames, samples, states, scale, stride = ps.removal_case("chunk70")
    assert len(samples) == 70
    dump = ps.as_dump(states)
    per_chunk, st_chunk = dr.deintegrate_reference(dump, samples)
    per_call, st_call = dr.deintegrate_reference(dump, samples, max_frames=70)
    differ = int((per_chunk[2] != per_call[2]).sum())
    print(f"chunk70: {differ} voxels differ, stats per chunk {st_chunk}, per call {st_call}")
    assert differ >= 200 and st_chunk[3] != st_call[3] and st_chunk[2] != st_call[2]
    # where they differ the per-call decision left the voxel alone and the per-chunk one removed the first chunk's observations
    n1 = ps.sample_counts(dump[0], samples[:ps.CHUNK])[0]
    m = per_chunk[2] != per_call[2]
    np.testing.assert_array_equal(per_call[2][m], dump[2][m])
    np.testing.assert_array_equal(per_chunk[2][m], (dump[2].astype(np.int64) - n1)[m])


def test_one_voxel_units_visit_every_lane_component_and_group_of_the_emptiness_reader():
    """hv_tsdf_unit_has_weight reads the weight plane in 16 iterations of 64 lanes x 16 bytes, with an exit test per group of four
    iterations: library word = ((iteration * 64 + lane) * 4 + component)."""
    words = np.array(ps.ONE_VOXEL_WORDS)
    assert 320 <= len(words) <= 340 and {0, ps.NV - 1} | set(ps.CORNER_WORDS) <= set(words.tolist())
    lib = np.array([ps.library_word(int(i)) for i in words])
    assert len(set(lib.tolist())) == len(words)
    assert set(lib & 3) == set(range(4)) and set((lib >> 2) & 63) == set(range(64)) and set(lib >> 8) == set(range(16))
    assert {(int(w) >> 10, int(w) & 3) for w in lib} == {(g, c) for g in range(4) for c in range(4)}
    assert {(int(w) >> 10, (int(w) >> 2) & 63) for w in lib} == {(g, l) for g in range(4) for l in range(64)}
    states, order = ps.one_voxel_units()
    keys, tsdf, weight, colour = states
    assert len(keys) == len(words) and sorted(order.tolist()) == sorted(words.tolist())
    assert (np.diff(np.asarray(keys, np.int64) @ [1 << 40, 1 << 20, 1]) > 0).all() and keys[:, 0].min() < 0 < keys[:, 0].max()
    assert ((weight > 0).sum(axis=1) == 1).all()
    np.testing.assert_array_equal(np.argmax(weight, axis=1), order)
    ref, stats = pr.prune_reference(ps.as_dump(states), True)
    assert stats == (len(keys), 0, 0, len(keys))


def test_empty_units_are_what_prune_releases():
    keys = ps.one_voxel_keys(5, first=-2) + [0, 7, 0]
    states = ps.empty_units(keys)
    assert all(not np.any(x) for x in states[1:]) and len(states[0]) == 5
    ref, stats = pr.prune_reference(ps.as_dump(states), True)
    assert stats == (5, 0, 5, 0) and len(ref[0]) == 0
    assert pr.prune_reference(ps.as_dump(states), False)[1] == (5, 0, 0, 5)


def test_finish_admits_weights_up_to_the_exactness_limit():
    w = np.float32(ps.MAX_WEIGHT)
    c = np.arange(256, dtype=np.float32) * w
    assert np.array_equal(c.astype(np.float64), np.arange(256) * float(w)) and float(c.max()) < 2.0 ** 24
    keys, tsdf, weight, colour = ps.finish([(0, 0, 0)], np.full(ps.NV, 0.5), np.full(ps.NV, ps.MAX_WEIGHT), np.full((ps.NV, 3), 255), max_weight=ps.MAX_WEIGHT)
    assert weight.max() == ps.MAX_WEIGHT
    with pytest.raises(AssertionError):
        ps.finish([(0, 0, 0)], np.zeros(ps.NV), np.full(ps.NV, 8), np.zeros((ps.NV, 3)))  # the default stays 7
