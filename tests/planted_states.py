"""Voxel states that no depth image produces, for the two kernels that read the map at arbitrary positions (hv_merge.hip,
hv_raycast.hip) and the two that rewrite it in place (hv_deintegrate.hip, hv_prune.hip) - test infrastructure, no GPU.

A STATE is (keys [U,3] int32 sorted by (x, y, z), tsdf [U,4096] float32, weight [U,4096] float32, colour [U,4096,3] float64) in
dump order (x * 256 + y * 16 + z).  Weights are integers <= 7 (finish(max_weight=...) admits up to 65 000) and colours integers
0..255, so every numerator of the float32 payload of hv_tsdf_import_numerators (tsdf * weight aside) is exact: colour * weight <=
255 * 65 000 < 2^24 is an integer float32 holds.  The tsdf goes through one float32 product and one float32 quotient, which
as_dump() repeats, so as_dump(states) IS the dump of a volume the states were planted into, bit for bit.  The GPU tests still run
the restatements on the planted volume's own dump(), never on the arrays that were planted.

The de-integration and prune builders (deintegration_target, chunk_boundary_target, one_voxel_units, empty_units) plant what a map
fused from the frames that are then removed never holds: all three branches of the removal rule inside one 16-byte quad, weights
between a voxel's count in the first 64-frame chunk and its count over the call, colours the removed frames never contributed,
units with one observed voxel, all-zero units.

Poses: EXACT-INVERSE camera poses (a signed-permutation rotation of determinant +1 and a translation in multiples of 2^-7 m) have
an inverse that every method computes without rounding, so the ray-cast reference and the library start from the same float32
rays.  Merge transforms that are signed permutations are written with literal 0 / +-1 entries.
"""
import functools
import itertools

import numpy as np

R = 16
NV = R ** 3
VOX, TRUNC = 0.02, 0.08
UNIT = VOX * R
B = 1 << 20  # unit indices live in [-B, B)
_IDX = np.stack(np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij"), -1).reshape(NV, 3)  # x * 256 + y * 16 + z


def centres(keys, voxel=VOX):
    """-> voxel centres [U, 4096, 3] float64 of the units `keys`."""
    return (np.asarray(keys, np.int64).reshape(-1, 1, 3) * R + _IDX[None] + 0.5) * voxel


MAX_WEIGHT = 65000  # 255 * 65 000 < 2^24: colour * weight stays an exact float32 integer


def finish(keys, tsdf, weight, colour, max_weight=7):
    """Sort by key, cast, and put unobserved voxels into the fresh state (tsdf 0, colour 0)."""
    assert max_weight <= MAX_WEIGHT
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    weight = np.asarray(weight, np.float32).reshape(len(keys), NV)[order]
    assert (weight == np.rint(weight)).all() and weight.min() >= 0 and weight.max() <= max_weight
    tsdf = np.where(weight > 0, np.asarray(tsdf, np.float32).reshape(len(keys), NV)[order], np.float32(0))
    colour = np.asarray(colour, np.float64).reshape(len(keys), NV, 3)[order]
    assert (colour == np.rint(colour)).all() and colour.min() >= 0 and colour.max() <= 255
    return keys[order].astype(np.int32), tsdf, weight, np.where(weight[..., None] > 0, colour, 0.0)


def as_dump(states):
    """What dump() of a volume gives after plant(volume, states): the import's tsdf = (float)(tsdf * weight) / weight in float32."""
    keys, tsdf, weight, colour = states
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(weight > 0, (tsdf * weight) / weight, np.float32(0)).astype(np.float32)
    return keys.copy(), t, weight.copy(), colour.copy()


def plant(volume, states):
    """Hand the states to a ScalableTSDFVolume through import_numerators (payload {tsdf * w, w, r * w, g * w, b * w} float32 in the
    library's voxel order z * 256 + x * 16 + y, as tests/test_gpu_tsdf.py)."""
    keys, tsdf, weight, colour = states
    n = len(keys)
    word = lambda a: a.reshape(n, R, R, R).transpose(0, 3, 1, 2).reshape(n, NV)
    payload = np.zeros((n, NV, 5), np.float32)
    payload[..., 0] = word(tsdf * weight)
    payload[..., 1] = word(weight)
    for c in range(3):
        payload[..., 2 + c] = word(colour[..., c].astype(np.float32) * weight)
    volume.import_numerators(np.ascontiguousarray(keys, dtype=np.int32), payload)
    return volume


def to_oracle(states, voxel=VOX, trunc=TRUNC):
    """The same states in an oracle.PortTsdf (its load hook takes [U,R,R,R] (x, y, z) arrays)."""
    import oracle

    keys, tsdf, weight, colour = states
    cpu = oracle.PortTsdf(voxel, trunc)
    cpu.load_units(keys, tsdf.reshape(-1, R, R, R), weight.reshape(-1, R, R, R), colour.reshape(-1, R, R, R, 3))
    return cpu


# ---- builders ----------------------------------------------------------------------------------------------------------------
def cluster_keys(seed=1, isolated=((4, 5, -3),)):
    """A 3 x 3 x 3 cluster of units at indices -2..0 with about 20 % removed, plus isolated units."""
    rng = np.random.default_rng(100 + seed)
    return np.array([k for k in itertools.product(range(-2, 1), repeat=3) if rng.random() > 0.2] + [tuple(k) for k in isolated], np.int64)


def sphere_and_plane(keys, seed=1, special=True, voxel=VOX, trunc=TRUNC):
    """tests/test_gpu_tsdf.py's _synthetic_unit_states at this voxel size: a sphere and a tilted plane crossing unit borders along
    every axis; `special`: 8 % of the voxels overwritten with values on decision boundaries (+-0, +-0.98, +-1 ...).  Weights random
    1..7 with 10 % of the voxels unobserved, colours random."""
    rng = np.random.default_rng(seed)
    p = centres(keys, voxel)
    s = voxel / 0.01
    centre, radius = np.array([-0.07, -0.10, -0.06]) * s, 0.13 * s
    n = np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
    d = np.minimum(np.linalg.norm(p - centre, axis=-1) - radius, p @ n + 0.02 * s)
    tsdf = np.clip(d / trunc, -1.0, 1.0).astype(np.float32)
    if special:
        b = np.float32(0.98)
        values = np.array([-1.0, -b, np.nextafter(-b, np.float32(0)), np.nextafter(-b, np.float32(-2)), -0.5, -1e-3, -0.0, 0.0, 1e-3, 0.5,
                           np.nextafter(b, np.float32(0)), b, np.nextafter(b, np.float32(2)), 1.0], np.float32)
        m = rng.random(tsdf.shape) < 0.08
        tsdf[m] = rng.choice(values, int(m.sum()))
    weight = rng.integers(1, 8, tsdf.shape).astype(np.float32)
    weight[rng.random(tsdf.shape) < 0.10] = 0.0
    colour = rng.integers(0, 256, tsdf.shape + (3,)).astype(np.float64)
    return finish(keys, tsdf, weight, colour)


def sparse_source(seed=1, special=True):
    return sphere_and_plane(cluster_keys(seed), seed, special)


def random_units(keys, seed, unobserved=0.3):
    """Units with arbitrary values: tsdf uniform in [-1, 1], weights 1..7 (a share unobserved), random colours.  A unit's values
    depend on `seed` and its key alone, not on which other units are built with it."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    tsdf, weight, colour = np.zeros((len(keys), NV), np.float32), np.zeros((len(keys), NV), np.float32), np.zeros((len(keys), NV, 3))
    for i, key in enumerate(keys):
        rng = np.random.default_rng([seed] + (key + B).tolist())
        tsdf[i] = rng.uniform(-1.0, 1.0, NV)
        weight[i] = rng.integers(1, 8, NV)
        weight[i][rng.random(NV) < unobserved] = 0.0
        colour[i] = rng.integers(0, 256, (NV, 3))
    return finish(keys, tsdf, weight, colour)


def every_second_unit(keys):
    """About half of a sorted key list: what an overlapping destination holds of a merge's result."""
    return np.asarray(keys, np.int64).reshape(-1, 3)[::2]


def single_voxel(unit, local, tsdf=0.25, weight=5, colour=(10, 200, 77)):
    """One observed voxel `local` (x, y, z) in unit `unit`, the rest of the unit unobserved."""
    t, w, c = np.zeros((1, NV), np.float32), np.zeros((1, NV), np.float32), np.zeros((1, NV, 3))
    i = (local[0] * R + local[1]) * R + local[2]
    t[0, i], w[0, i], c[0, i] = tsdf, weight, colour
    return finish([unit], t, w, c)


SINGLE_VOXELS = {"low corner": ((-1, -1, -1), (0, 0, 0)), "high corner": ((0, 0, 0), (15, 15, 15)), "face": ((-3, 2, 0), (15, 0, 7))}
RIM_UNITS = ((B - 1, 0, -B), (B - 1, -1, -B), (-B, B - 1, 5))
RIM_ALIAS = (-B, 1, -B)  # what (B, 0, -B) packs to when nothing checks the range


def rim_source(alias=True, seed=7):
    return random_units(np.array(RIM_UNITS + ((RIM_ALIAS,) if alias else ()), np.int64), seed)


# ---- transforms --------------------------------------------------------------------------------------------------------------
def with_translation(rot, voxels=(0, 0, 0), metres=None):
    T = np.eye(4)
    T[:3, :3] = np.array(rot, np.float64)
    T[:3, 3] = np.asarray(voxels, np.float64) * VOX if metres is None else np.asarray(metres, np.float64)
    return T


ROT_X90 = ((1, 0, 0), (0, 0, -1), (0, 1, 0))     # 90 deg about x
ROT_111_120 = ((0, 0, 1), (1, 0, 0), (0, 1, 0))  # 120 deg about (1, 1, 1): x -> y -> z -> x
ROT_Y180 = ((-1, 0, 0), (0, 1, 0), (0, 0, -1))   # 180 deg about y
IDENTITY = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
EXACT_ROTATIONS = {
    "x90": with_translation(ROT_X90, (3, -2, 5)),
    "diag120": with_translation(ROT_111_120, (-7, 18, 1)),
    "y180": with_translation(ROT_Y180, (16, 0, -33)),
    "x90 half": with_translation(ROT_X90, (2.5, -0.5, 4.5)),
}
HALF_SHIFT = with_translation(IDENTITY, (0.5, 0.5, 0.5))
RIM_TRANSFORMS = {"identity": np.eye(4), "x+16": with_translation(IDENTITY, (16, 0, 0)), "z-3": with_translation(IDENTITY, (0, 0, -3))}
MERGE_T = (0.313, -0.127, 0.2381)
FAR_T = (200000.013, -150000.127, 1000.2381)
DIAGONAL_DEG = float(np.degrees(np.arccos(1.0 / np.sqrt(3.0))))
WORST_CASE_ROTATIONS = {"diagonal": ((1, -1, 0.02), DIAGONAL_DEG), "z45": ((0.05, -0.03, 1), 45.0), "diag60": ((1, 0.9, 1.1), 60.0),
                        "y179": ((0.2, 1, -0.1), 179.0)}


def permuted_index(T, gi, voxel=VOX):
    """Where a signed-permutation transform with a whole-voxel translation carries the source voxels gi [n,3] (global indices):
    centre (i + 0.5) voxel -> T centre; exact in float64 for |i| < 2^24."""
    T = np.asarray(T, np.float64)
    out = (np.asarray(gi, np.float64) + 0.5) @ T[:3, :3].T + T[:3, 3] / voxel - 0.5
    assert np.abs(out - np.rint(out)).max() < 1e-6, "not a whole-voxel permutation"
    return np.rint(out).astype(np.int64)


# ---- ray-cast scenes ---------------------------------------------------------------------------------------------------------
CAMERA = np.array([2.0, -3.0, 5.0]) / 128.0  # a dyadic offset from the origin
INTR = (40.0, 40.0, 16.0, 12.0)  # 32 x 24: column 16 and row 12 are rays with a zero direction component
H, W = 24, 32
FRONT, BACK = 0.5, 0.95
DIRECTIONS = tuple((axis, sign) for axis in range(3) for sign in (1, -1))


def camera_pose(axis, sign, camera=CAMERA):
    """T_cw of a camera at `camera` looking along sign * e_axis: camera z -> sign e_axis, camera x -> e_(axis+1), camera y ->
    sign e_(axis+2) (determinant +1).  Literal 0 / +-1 entries."""
    T_wc = np.eye(4)
    T_wc[:3, :3] = 0.0
    T_wc[(axis + 1) % 3, 0] = 1.0
    T_wc[(axis + 2) % 3, 1] = float(sign)
    T_wc[axis, 2] = float(sign)
    T_wc[:3, 3] = camera
    T_cw = np.eye(4)
    T_cw[:3, :3] = T_wc[:3, :3].T
    T_cw[:3, 3] = -(T_wc[:3, :3].T @ T_wc[:3, 3])
    return T_cw


def two_walls(axis, sign, seed=3, camera=CAMERA, hole=(0, 0)):
    """Two walls across the viewing axis, FRONT and BACK metres ahead of `camera`, over the 2 x 2 lateral units -1..0; the front
    wall's lateral unit `hole` is missing.  Only the truncation band is observed (weight 4); a unit no band reaches is absent - the
    unit layer next to the camera among them.  -> (states, scene) with scene = {axis, sign, camera, front, back, hole}."""
    rng = np.random.default_rng(seed)
    a, l0, l1 = axis, (axis + 1) % 3, (axis + 2) % 3
    keys = []
    for which, dist in (("front", FRONT), ("back", BACK)):
        q = camera[a] + sign * dist
        for layer in range(int(np.floor((q - TRUNC) / UNIT)), int(np.floor((q + TRUNC) / UNIT)) + 1):
            for i, j in itertools.product((-1, 0), repeat=2):
                if which == "front" and (i, j) == tuple(hole):
                    continue
                k = [0, 0, 0]
                k[a], k[l0], k[l1] = layer, i, j
                keys.append(tuple(k))
    keys = np.array(sorted(set(keys)), np.int64)
    p = centres(keys)[..., a]
    tsdf, weight = np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)
    for dist in (FRONT, BACK):
        q = camera[a] + sign * dist
        sdf = sign * (q - p)
        band = np.abs(sdf) <= TRUNC
        tsdf[band] = (sdf[band] / TRUNC).astype(np.float32)
        weight[band] = 4.0
    colour = rng.integers(0, 256, p.shape + (3,)).astype(np.float64)
    scene = {"axis": axis, "sign": sign, "camera": np.asarray(camera, np.float64), "hole": tuple(hole)}
    return finish(keys, tsdf, weight, colour), scene


def analytic_walls(scene, margin_voxels=2.0, intr=INTR, height=H, width=W):
    """Per pixel of camera_pose(axis, sign): the depth (FRONT, BACK or 0) a ray must return, and whether the ray is INTERIOR: its
    analytic hit, and where it passes the front wall, lies >= margin_voxels inside the lateral edges of the planted footprint and of
    the hole - only those are held to the analytic depth.  -> (depth [H,W], interior [H,W], normal [3])."""
    fx, fy, cx, cy = intr
    v, u = np.mgrid[0:height, 0:width].astype(np.float64)
    a, l0, l1 = scene["axis"], (scene["axis"] + 1) % 3, (scene["axis"] + 2) % 3
    m = margin_voxels * VOX
    lat = lambda z: (scene["camera"][l0] + z * (u - cx) / fx, scene["camera"][l1] + z * scene["sign"] * (v - cy) / fy)
    h0, h1 = scene["hole"]

    def inside(x, y, lo0, hi0, lo1, hi1, pad):
        return (x >= lo0 + pad) & (x <= hi0 - pad) & (y >= lo1 + pad) & (y <= hi1 - pad)

    xf, yf = lat(FRONT)
    xb, yb = lat(BACK)
    hole = (h0 * UNIT, (h0 + 1) * UNIT, h1 * UNIT, (h1 + 1) * UNIT)
    on_front = inside(xf, yf, -UNIT, UNIT, -UNIT, UNIT, m) & ~inside(xf, yf, *hole, -m)
    # through the hole: over the whole depth of the front band, then onto the back wall
    through = np.ones(u.shape, bool)
    for z in (FRONT - TRUNC - 2 * VOX, FRONT + TRUNC + 2 * VOX):
        x, y = lat(z)
        through &= inside(x, y, *hole, m)
    on_back = through & inside(xb, yb, -UNIT, UNIT, -UNIT, UNIT, m)
    depth = np.where(on_front, FRONT, np.where(on_back, BACK, 0.0))
    normal = np.zeros(3)
    normal[a] = -scene["sign"]
    return depth, on_front | on_back, normal


def behind_the_front_wall(scene, margin_voxels=2.0, intr=INTR, height=H, width=W):
    """Interior rays of the front wall that reach the back wall >= margin_voxels inside its footprint: where the front wall is made
    unobserved they must return BACK."""
    fx, fy, cx, cy = intr
    v, u = np.mgrid[0:height, 0:width].astype(np.float64)
    l0, l1 = (scene["axis"] + 1) % 3, (scene["axis"] + 2) % 3
    x, y = scene["camera"][l0] + BACK * (u - cx) / fx, scene["camera"][l1] + BACK * scene["sign"] * (v - cy) / fy
    m = UNIT - margin_voxels * VOX
    depth, interior, _ = analytic_walls(scene, margin_voxels, intr, height, width)
    return interior & (depth == FRONT) & (np.abs(x) <= m) & (np.abs(y) <= m)


def front_columns(scene, columns, margin_voxels=2.0, intr=INTR, height=H, width=W):
    """Rays that pass the front wall >= margin_voxels inside the voxel columns [columns[0], columns[1]) of the first lateral axis."""
    fx, _, cx, _ = intr
    _, u = np.mgrid[0:height, 0:width].astype(np.float64)
    g = (scene["camera"][(scene["axis"] + 1) % 3] + FRONT * (u - cx) / fx) / VOX
    return (g >= columns[0] + margin_voxels) & (g <= columns[1] - margin_voxels)


# the weight pattern of the threshold tests, on two_walls(2, +1): lateral x columns of the front wall
WEAK_COLUMNS = (3, 8)      # voxel columns x in [3, 8): the whole front band has weight 3
SPLIT_COLUMNS = (-5, 0)    # voxel columns x in [-5, 0): ONE layer, the last with tsdf > 0 before the front wall, has weight 3


def weight_pattern(states, scene):
    """Weights 3 among the 4s.  At threshold 3.0 a weight of 3 is unobserved: the front wall is gone over WEAK_COLUMNS, and over
    SPLIT_COLUMNS its sign change is split by one unobserved voxel (no hit: the march forgets its previous sample); at 2.5 every
    planted voxel is observed; at 4.0 none."""
    assert scene["axis"] == 2 and scene["sign"] == 1
    keys, tsdf, weight, colour = (np.array(x, copy=True) for x in states)
    p = centres(keys)
    gx = np.floor(p[..., 0] / VOX).astype(np.int64)
    q = scene["camera"][2] + FRONT
    front = np.abs(p[..., 2] - q) <= TRUNC
    weak = front & (gx >= WEAK_COLUMNS[0]) & (gx < WEAK_COLUMNS[1])
    last_positive = front & (p[..., 2] < q) & (p[..., 2] + VOX > q)
    split = last_positive & (gx >= SPLIT_COLUMNS[0]) & (gx < SPLIT_COLUMNS[1])
    weight[(weak | split) & (weight > 0)] = 3.0
    return finish(keys, tsdf, weight, colour)


def tilted_wall_at_a_missing_unit(seed=5, camera=CAMERA):
    """A wall tilted about y (its normal towards the camera, which looks along +z, is (-0.6, 0, -0.8)) planted only for x >= 0: its
    band touches the unit face x = 0 and the unit beyond is absent, so hits near x = 0 have an incomplete trilinear neighbourhood -
    the refinement ends at its first invalid sample, the colour is the nearest voxel's and the gradient reads missing neighbours."""
    rng = np.random.default_rng(seed)
    n, d = np.array([0.6, 0.0, 0.8]), 0.6 * camera[0] + 0.8 * (camera[2] + FRONT)
    keys = np.array([(i, j, k) for i in (0,) for j in (-1, 0) for k in range(0, 4)], np.int64)
    p = centres(keys)
    sdf = d - p @ n
    band = np.abs(sdf) <= TRUNC
    keep = band.any(axis=1)
    keys, sdf, band = keys[keep], sdf[keep], band[keep]
    tsdf = np.where(band, sdf / TRUNC, 0.0).astype(np.float32)
    weight = np.where(band, 4.0, 0.0).astype(np.float32)
    return finish(keys, tsdf, weight, rng.integers(0, 256, tsdf.shape + (3,)).astype(np.float64))


# ---- de-integration targets ----------------------------------------------------------------------------------------------------
SPECIAL_TSDF = (-1.0, -0.98, -0.5, -1e-3, -0.0, 0.0, 1e-3, 0.5, 0.98, 1.0)
CHUNK = 64  # HV_TSDF_DEINTEGRATE_MAX_FRAMES


def sample_counts(keys, samples):
    """Per voxel of the units `keys` [U,3]: how many of the frames `samples` (FrameSamples) sample it, and the sum of their colour
    bytes.  -> (n [U,4096] int64, bytes [U,4096,3] int64, units the frames list that `keys` does not hold)."""
    index = {tuple(int(x) for x in k): i for i, k in enumerate(np.asarray(keys))}
    n, csum, missing = np.zeros((len(index), NV), np.int64), np.zeros((len(index), NV, 3), np.int64), 0
    for fs in samples:
        for j, k in enumerate(fs.keys):
            i = index.get(tuple(int(x) for x in k))
            if i is None:
                missing += 1
                continue
            n[i] += fs.sampled[j]
            csum[i] += fs.colour[j] * fs.sampled[j][:, None]
    return n, csum, missing


def removal_classes(weight, n):
    """The three branches of the removal rule for voxels of weight `weight` that n frames of one chunk sample.
    -> (underflow, fresh, remaining) bool masks."""
    w = np.asarray(weight).astype(np.int64)
    return (n > 0) & (w < n), (n > 0) & (w == n), (n > 0) & (w > n)


def quads_with_all_classes(under, fresh, rest):
    """How many quads (four consecutive y at fixed x, z of one unit: one lane's 16-byte access) hold all three classes."""
    q = lambda m: m.reshape(-1, R, R // 4, 4, R).any(axis=3)
    return int((q(under) & q(fresh) & q(rest)).sum())


def clamp_ends(dump, n, csum):
    """Voxels of a single-chunk removal (n, csum = sample_counts of the dump's keys) at which the clamp of the colour sums acts:
    (sum - bytes < 0 in some channel, sum - bytes > 255 (w - n) in some channel), counted over the remaining class."""
    _, _, weight, colour = dump
    rest = removal_classes(weight, n)[2]
    w = np.asarray(weight).astype(np.int64)
    left = np.rint(np.asarray(colour) * np.asarray(weight, np.float64)[..., None]).astype(np.int64) - csum
    return int((rest & (left < 0).any(-1)).sum()), int((rest & (left > 255 * (w - n)[..., None]).any(-1)).sum())


def _target_keys(samples, rng, drop):
    keys = np.unique(np.concatenate([np.asarray(fs.keys, np.int64).reshape(-1, 3) for fs in samples]), axis=0)
    gone = rng.random(len(keys)) < drop
    gone[rng.integers(len(keys))] = True  # at least one unit of the touch sets is absent
    return keys[~gone]


def _arbitrary_tsdf(rng, shape):
    tsdf = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    m = rng.random(shape) < 0.08
    tsdf[m] = rng.choice(np.array(SPECIAL_TSDF, np.float32), int(m.sum()))
    return tsdf


def _consistent_colour(rng, colour, weight, n, csum):
    """Where weight > n: an integer mean c with bytes <= c * weight <= bytes + 255 (weight - n) - the sum holds the bytes that are
    removed, and what is left is the sum of weight - n bytes.  (The range is 255 (weight - n) / weight >= 255 / 65 wide.)"""
    rest = weight > n
    w = np.maximum(weight, 1)[..., None]
    lo = -((-csum) // w)
    hi = (csum + 255 * (weight - n)[..., None]) // w
    assert (lo <= hi)[rest].all() and (lo >= 0).all() and (hi[rest] <= 255).all()
    c = lo + np.floor(rng.random(csum.shape) * (hi - lo + 1)).astype(np.int64)
    return np.where(rest[..., None], np.minimum(c, hi), colour)


def _foreign_colour(rng, shape):
    colour = rng.integers(0, 256, shape + (3,))
    u = rng.random(shape + (3,))
    colour[u < 0.2] = 0
    colour[u > 0.8] = 255
    return colour


def deintegration_target(samples, seed, colours="consistent", drop=0.15):
    """A state for the removal of the frames `samples` (FrameSamples of ONE chunk: <= 64 frames).  Units: the union of the frames'
    touch sets less a share `drop` (at least one unit; each absence counts once per frame that lists it in units_missing).  A
    voxel that n >= 1 frames sample gets a weight drawn evenly from {0, n - 1, n, n + 1, n + k} (k in 2..6; n - 1 = 0 when n = 1):
    underflow, underflow, fresh, one observation left, several left - placed at random, so all branches meet inside single quads.
    Voxels no frame samples hold weights 0..7.  tsdf arbitrary in [-1, 1] with special values.  colours = "consistent": where
    observations remain the planted sum holds the removed bytes and leaves at most 255 per remaining observation (the clamp never
    acts); "foreign": random colours with 0 and 255 over-represented (both ends of the clamp are reached)."""
    assert 1 <= len(samples) <= CHUNK and colours in ("consistent", "foreign")
    rng = np.random.default_rng(seed)
    keys = _target_keys(samples, rng, drop)
    n, csum, _ = sample_counts(keys, samples)
    pick = rng.integers(0, 5, n.shape)
    weight = np.select([pick == 0, pick == 1, pick == 2, pick == 3], [0, n - 1, n, n + 1], n + rng.integers(2, 7, n.shape))
    free = rng.integers(1, 8, n.shape)
    free[rng.random(n.shape) < 0.3] = 0
    weight = np.where(n > 0, weight, free)
    assert quads_with_all_classes(*removal_classes(weight, n)) > 0  # random placement: the three branches share quads
    colour = _foreign_colour(rng, n.shape)
    if colours == "consistent":
        colour = _consistent_colour(rng, colour, weight, n, csum)
    return finish(keys, _arbitrary_tsdf(rng, n.shape), weight, colour, max_weight=CHUNK + 6)


def chunk_boundary_target(samples, seed, drop=0.1):
    """A state for the removal of more than 64 frames in one call.  n1 = a voxel's count in the first chunk, nt = over the whole
    call.  Where n1 >= 1 and nt - n1 >= 2, half of the voxels get a weight strictly between n1 and nt: decided per chunk the first
    chunk's observations leave and the second chunk underflows; decided per call nothing would be removed.  Every other voxel is
    drawn as in deintegration_target with n = nt.  Colours are consistent where the weight exceeds the count."""
    assert CHUNK < len(samples) <= 2 * CHUNK
    rng = np.random.default_rng(seed)
    keys = _target_keys(samples, rng, drop)
    n1, csum1, _ = sample_counts(keys, samples[:CHUNK])
    n2, csum2, _ = sample_counts(keys, samples[CHUNK:])
    nt = n1 + n2
    pick = rng.integers(0, 5, nt.shape)
    weight = np.select([pick == 0, pick == 1, pick == 2, pick == 3], [0, nt - 1, nt, nt + 1], nt + rng.integers(2, 7, nt.shape))
    free = rng.integers(1, 8, nt.shape)
    free[rng.random(nt.shape) < 0.3] = 0
    weight = np.where(nt > 0, weight, free)
    between = (n1 >= 1) & (n2 >= 2) & (rng.random(nt.shape) < 0.5)
    weight = np.where(between, n1 + 1 + np.floor(rng.random(nt.shape) * np.maximum(n2 - 1, 1)).astype(np.int64), weight)
    assert ((weight > n1) & (weight < nt))[between].all()
    colour = _consistent_colour(rng, _foreign_colour(rng, nt.shape), weight, nt, csum1 + csum2)
    colour = np.where(between[..., None], _consistent_colour(rng, colour, weight, n1, csum1), colour)
    return finish(keys, _arbitrary_tsdf(rng, nt.shape), weight, colour, max_weight=2 * CHUNK + 6)


# the removals the de-integration tests plant for: name -> (camera, first frame, frames, colours, seed).  "tiny": 160 x 120, float32
# depth, stride 4; "odd": 97 x 61, uint16 depth (scale 5000), stride 1.
REMOVALS = {"single": ("tiny", 2, 1, "consistent", 5), "single odd": ("odd", 2, 1, "consistent", 6), "batch5": ("tiny", 10, 5, "consistent", 7),
            "batch64": ("tiny", 0, 64, "consistent", 8), "foreign": ("tiny", 20, 5, "foreign", 9), "chunk70": ("tiny", 0, 70, "consistent", 10)}


@functools.lru_cache(maxsize=None)
def _removal_frames(camera, count):
    from tests.deintegrate_reference import frame_samples
    from tests.test_gpu_tsdf_edges import frames_of, intrinsic, odd_config

    odd = camera == "odd"
    s, frames = frames_of(odd_config(97, 61) if odd else "tiny_160x120_2cm", 0, count, depth_dtype="uint16" if odd else "float32")
    scale, stride = (5000.0, 1) if odd else (1.0, 4)
    K = intrinsic(s).as_array()
    return s, frames, [frame_samples(VOX, TRUNC, d, c, K, T, scale, 4.0, stride) for d, c, T in frames], scale, stride


@functools.lru_cache(maxsize=None)
def removal_case(name):
    """-> (camera, frames [(depth, colour, T_cw)], their FrameSamples, the planted states, depth_scale, stride) of REMOVALS[name].
    Shared between the tests: nothing of it may be written to."""
    camera, first, count, colours, seed = REMOVALS[name]
    s, frames, samples, scale, stride = _removal_frames(camera, 70 if camera == "tiny" else first + count)
    frames, samples = frames[first:first + count], samples[first:first + count]
    # (foreign: a quarter of the units - the test extracts a mesh from arbitrary tsdf values)
    states = (chunk_boundary_target(samples, seed) if count > CHUNK else
              deintegration_target(samples, seed, colours, drop=0.75 if colours == "foreign" else 0.15))
    return s, frames, samples, states, scale, stride


# ---- prune targets -----------------------------------------------------------------------------------------------------------
CORNER_WORDS = tuple((x * R + y) * R + z for x in (0, R - 1) for y in (0, R - 1) for z in (0, R - 1))
ONE_VOXEL_WORDS = tuple(sorted(set(range(0, NV, 13)) | {0, NV - 1} | set(CORNER_WORDS)))  # 13 is coprime to 4096


def library_word(i):
    """Dump-order voxel index i = x * 256 + y * 16 + z -> the library's word z * 256 + x * 16 + y inside a plane of the unit."""
    x, y, z = i >> 8, (i >> 4) & 15, i & 15
    return z * 256 + x * 16 + y


def one_voxel_keys(count, first=-150):
    """`count` distinct unit keys on a line through negative and positive indices."""
    j = np.arange(count, dtype=np.int64)
    return np.stack([first + j, j % 5 - 2, 1 - j % 3], axis=1)


def one_voxel_units(words=ONE_VOXEL_WORDS, keys=None):
    """For each word index i (dump order) a unit whose only observed voxel is i.  -> (states, words in the states' key order)."""
    keys = one_voxel_keys(len(words)) if keys is None else np.asarray(keys, np.int64).reshape(-1, 3)
    assert len(keys) == len(words)
    parts = [single_voxel(tuple(int(v) for v in key), (i >> 8, (i >> 4) & 15, i & 15), tsdf=((i % 9) - 4) / 4.0, weight=1 + i % 7,
                          colour=(i % 256, (i * 7) % 256, (i * 31) % 256)) for key, i in zip(keys, words)]
    states = finish(*(np.concatenate([p[k] for p in parts]) for k in range(4)))
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return states, np.asarray(words, np.int64)[order]


def empty_units(keys):
    """All-zero units: claimed, never updated."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    return finish(keys, np.zeros((len(keys), NV), np.float32), np.zeros((len(keys), NV), np.float32), np.zeros((len(keys), NV, 3)))
