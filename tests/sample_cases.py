"""The planted maps, point sets and frames the point-query tests share (tests/test_sample_reference_cpu.py on the CPU,
tests/test_gpu_tsdf_sample.py and tests/test_gpu_tsdf_check_frame.py on the GPU) - test infrastructure, no GPU.  Everything is built
from fixed seeds; the CPU file asserts that no point of these sets is fragile, which is what lets the GPU files compare bit for bit.
"""
import functools

import numpy as np

from tests import planted_states as ps

VOX, TRUNC, UNIT, B = ps.VOX, ps.TRUNC, ps.UNIT, ps.B
POINT_COUNTS = (1, 63, 64, 65, 4097)
THRESHOLDS = (0.0, 3.0)


def concat(*parts):
    return ps.finish(*(np.concatenate([np.asarray(p[k]) for p in parts]) for k in range(4)))


# ---- the sparse cluster -----------------------------------------------------------------------------------------------------------
ONE_VOXEL_UNITS = (((1, -1, -1), (0, 15, 7)), ((-3, 0, -2), (15, 15, 15)), ((-1, 1, 0), (8, 0, 0)))
CLUSTER_BOX = (-3 * UNIT, 2 * UNIT)  # the cluster's units -2..0 grown by one unit: [-3, 2) units per axis


@functools.lru_cache(maxsize=None)
def cluster_states():
    """planted_states' sparse source (a 3 x 3 x 3 cluster with about 20 % of the units missing, an isolated unit, weights 0..7 with
    10 % unobserved) plus units that hold one observed voxel each."""
    return concat(ps.sparse_source(), *(ps.single_voxel(unit, local, tsdf=0.25 - 0.1 * i, weight=1 + 3 * i)
                                        for i, (unit, local) in enumerate(ONE_VOXEL_UNITS)))


def cluster_points(n):
    """n float64 points drawn uniformly in CLUSTER_BOX (seed 1000 + n)."""
    return np.random.default_rng(1000 + n).uniform(CLUSTER_BOX[0], CLUSTER_BOX[1], (n, 3))


# ---- hand-made cases --------------------------------------------------------------------------------------------------------------
def at(gx, gy, gz):
    """The point whose lattice coordinate g is (gx, gy, gz): p = (g + 0.5) voxel."""
    return (np.array([gx, gy, gz], np.float64) + 0.5) * VOX


@functools.lru_cache(maxsize=None)
def hand_states():
    """Unit (0, 0, 0) fully observed except voxel (5, 5, 5); unit (2, 0, 0) with the one observed voxel (3, 3, 3); the units on the rim
    of the key range and the unit a key beyond the rim aliases to, fully observed."""
    keys, tsdf, weight, colour = ps.random_units(np.array([(0, 0, 0)], np.int64), 11, unobserved=0.0)
    weight = weight.copy()
    weight[0, (5 * 16 + 5) * 16 + 5] = 0.0
    full = ps.finish(keys, tsdf, weight, colour)
    rim = ps.random_units(np.array(ps.RIM_UNITS + (ps.RIM_ALIAS,), np.int64), 7, unobserved=0.0)
    return concat(full, ps.single_voxel((2, 0, 0), (3, 3, 3)), rim)


OUTSIDE, UNOBSERVED, NEAREST, TRILINEAR = 0, 1, 2, 3
X_RIM, Z_RIM = 16 * B, -16 * B  # the first voxel index beyond the rim in x; the first voxel index inside it in z
HAND_POINTS = (
    ("missing unit", at(7 * 16 + 5.3, 7 * 16 + 5.3, 7 * 16 + 5.3), OUTSIDE),
    ("nearest voxel in a missing neighbour unit", at(15.7, 8.2, 8.2), OUTSIDE),
    ("a corner in a missing neighbour unit", at(15.3, 8.2, 8.2), NEAREST),
    ("held unit, unobserved nearest voxel", at(40.1, 8.1, 8.1), UNOBSERVED),
    ("the one observed voxel of a unit", at(35.1, 3.2, 2.8), NEAREST),
    ("seven of eight observed", at(4.3, 4.8, 4.9), NEAREST),
    ("the nearest is the unobserved one of eight", at(4.7, 4.8, 4.9), UNOBSERVED),
    ("all eight observed", at(9.3, 9.4, 9.2), TRILINEAR),
    ("inside a rim unit", at(X_RIM - 8.7, 5.3, Z_RIM + 5.3), TRILINEAR),
    ("rim: a corner beyond the key range", at(X_RIM - 0.8, 5.3, Z_RIM + 5.3), NEAREST),
    ("rim: the nearest voxel beyond the key range", at(X_RIM - 0.3, 5.3, Z_RIM + 5.3), OUTSIDE),
    ("rim: a corner below the key range in z", at(X_RIM - 8.7, 5.3, Z_RIM - 0.3), NEAREST),
    ("rim: the nearest voxel below the key range in z", at(X_RIM - 8.7, 5.3, Z_RIM - 0.8), OUTSIDE),
    ("NaN", np.array([np.nan, 0.107, 0.107]), OUTSIDE),
    ("+inf", np.array([0.107, np.inf, 0.107]), OUTSIDE),
    ("-inf", np.array([0.107, 0.107, -np.inf]), OUTSIDE),
    ("|g| >= 1e9", np.array([0.107, 2.0e7 + 1.0, 0.107]), OUTSIDE),
    ("|g| just below 1e9", np.array([-1.9e7 + 0.0046, 0.107, 0.107]), OUTSIDE),
)


def hand_points():
    return np.stack([p for _, p, _ in HAND_POINTS]), np.array([s for _, _, s in HAND_POINTS], np.uint8)


# ---- the linear field -------------------------------------------------------------------------------------------------------------
X0 = 0.003
LINEAR_SDF_BOUND = TRUNC * 2.0 ** -22
LINEAR_GRADIENT_BOUND = 2.0 ** -19


@functools.lru_cache(maxsize=None)
def linear_states():
    """tsdf = (x - X0) / TRUNC over the 2 x 2 x 2 units -1..0, every voxel observed (weights 1..7)."""
    keys = np.array([(i, j, k) for i in (-1, 0) for j in (-1, 0) for k in (-1, 0)], np.int64)
    x = ps.centres(keys)[..., 0]
    rng = np.random.default_rng(21)
    return ps.finish(keys, ((x - X0) / TRUNC).astype(np.float32), rng.integers(1, 8, x.shape).astype(np.float32),
                     rng.integers(0, 256, x.shape + (3,)).astype(np.float64))


def linear_points(n=2000):
    """Interior points: all eight voxels around them lie in the block and hold |tsdf| < 1 (x within 0.05 m of X0, so that the
    voxels are within 0.07 m: the planted float32 values then carry roundings of at most 2^-25 each)."""
    rng = np.random.default_rng(22)
    return np.stack([rng.uniform(X0 - 0.05, X0 + 0.05, n), rng.uniform(-0.29, 0.29, n), rng.uniform(-0.29, 0.29, n)], axis=1)


# ---- frames for check_frame -------------------------------------------------------------------------------------------------------
IMAGE_SIZES = ((1, 1), (5, 3), (8, 8), (9, 70), (70, 9))  # (H, W): partial tiles at the right edge, the bottom edge and both
DEPTH_KINDS = (("float32", 1.0), ("uint16", 5000.0))


def generic_pose():
    """A rigid T_cw that is no signed permutation: planted_states.camera_pose(2, +1) turned by 0.3 rad about (1, -2, 0.5) and shifted."""
    k = np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rm = np.eye(3) + np.sin(0.3) * K + (1 - np.cos(0.3)) * (K @ K)
    T = np.eye(4)
    T[:3, :3] = Rm
    T[:3, 3] = (0.013, -0.021, 0.034)
    return T @ ps.camera_pose(2, 1)


POSES = {"+x": (0, 1), "-y": (1, -1), "+z": (2, 1), "generic": None}


def wall_scene(pose):
    """-> (states, T_cw): planted_states.two_walls seen along the pose's axis (the generic pose looks at the +z walls)."""
    axis, sign = POSES[pose] or (2, 1)
    states, _scene = ps.two_walls(axis, sign)
    return states, (generic_pose() if POSES[pose] is None else ps.camera_pose(axis, sign))


def intrinsics(H, W):
    """fx, fy, cx, cy with the principal point off centre and fx != fy; the image sees about +-0.3 m of the walls at 0.95 m."""
    f = 1.5 * max(H, W) + 10.0
    return (f, 1.07 * f, 0.5 * W - 0.25, 0.5 * H + 0.125)


def wall_depth(H, W, kind, scale, seed=0):
    """A depth image whose pixels lie on, before, behind and between the walls (FRONT 0.5, BACK 0.95), with invalid pixels among
    them; in the units of `scale`."""
    rng = np.random.default_rng([H, W, seed])
    pick = rng.integers(0, 8, (H, W))
    d = np.select([pick == 0, pick <= 2, pick <= 4, pick == 5],
                  [0.0, ps.FRONT + rng.uniform(-0.1, 0.1, (H, W)), ps.BACK + rng.uniform(-0.1, 0.1, (H, W)), rng.uniform(2.9, 3.2, (H, W))],
                  rng.uniform(0.05, 1.2, (H, W)))
    return np.rint(d * scale).astype(np.uint16) if kind == "uint16" else (d * scale).astype(np.float32)


# ---- the fused scene --------------------------------------------------------------------------------------------------------------
FUSED_FRAMES, FUSED_FRAME = 8, 4
PULL, PULL_RECT = 0.3, (slice(40, 80), slice(50, 110))  # rows, columns of tiny_160x120_2cm's frame FUSED_FRAME


def pulled(depth):
    """The frame's depth with PULL_RECT moved PULL metres nearer the camera (invalid pixels stay invalid)."""
    out = np.array(depth, np.float32, copy=True)
    rect = out[PULL_RECT]
    out[PULL_RECT] = np.where(rect > 0, rect - np.float32(PULL), rect)
    return out
