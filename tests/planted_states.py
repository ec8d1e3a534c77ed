"""Voxel states that no depth image produces, for the two kernels that read the map at arbitrary positions (hv_merge.hip,
hv_raycast.hip) - test infrastructure, no GPU.

A STATE is (keys [U,3] int32 sorted by (x, y, z), tsdf [U,4096] float32, weight [U,4096] float32, colour [U,4096,3] float64) in
dump order (x * 256 + y * 16 + z).  Weights are integers <= 7 and colours integers 0..255, so every numerator of the float32
payload of hv_tsdf_import_numerators (tsdf * weight aside) is exact; the tsdf goes through one float32 product and one float32
quotient, which as_dump() repeats, so as_dump(states) IS the dump of a volume the states were planted into, bit for bit.  The GPU
tests still run the restatements on the planted volume's own dump(), never on the arrays that were planted.

Poses: EXACT-INVERSE camera poses (a signed-permutation rotation of determinant +1 and a translation in multiples of 2^-7 m) have
an inverse that every method computes without rounding, so the ray-cast reference and the library start from the same float32
rays.  Merge transforms that are signed permutations are written with literal 0 / +-1 entries.
"""
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


def finish(keys, tsdf, weight, colour):
    """Sort by key, cast, and put unobserved voxels into the fresh state (tsdf 0, colour 0)."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    weight = np.asarray(weight, np.float32).reshape(len(keys), NV)[order]
    assert (weight == np.rint(weight)).all() and weight.min() >= 0 and weight.max() <= 7
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
