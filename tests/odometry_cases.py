"""Planted frames for the tests of rgbd_odometry - test infrastructure, no GPU: small target depths that exercise every clause of
the model rule (include/hipvol.h, hv_rgbd_odometry: `model`), closed-form surfaces for the normals, and the textured wall of
tests/test_gpu_tsdf_track_color.py rendered at any pose."""
import numpy as np

from tests import track_reference as tr
from tests import tsdf_closed_form as cf

_f32 = np.float32

# every shape at which the model kernel takes another path: no pixel off the border (1x1, 2x5), exactly one (3x3), interior rows
# that cross the 64-lane wave (5x67) and the 256-thread workgroup (3x130) boundaries, and odd sizes halved twice (11x13)
SHAPES = [(1, 1, 0), (2, 5, 0), (3, 3, 0), (5, 67, 0), (3, 130, 0), (11, 13, 0), (11, 13, 1), (11, 13, 2)]  # (h, w, level)


def intrinsics(h, w):
    return np.array([0.9 * w + 3.0, 0.8 * w + 5.0, 0.5 * (w - 1) + 0.25, 0.5 * (h - 1) - 0.125])


def surface(h, w, seed=0, holes=True):
    """A smooth tilted surface about 1.2 m away with millimetre noise, a few invalid pixels planted: float32 [h,w]."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 1.2 + 0.004 * u - 0.003 * v + 0.02 * np.sin(0.7 * u + 0.3 * v) + 1e-3 * rng.standard_normal((h, w))
    if holes and h * w > 9:  # (a 3x3 frame keeps its one interior pixel)
        z[rng.random((h, w)) < 0.05] = 0.0
    return z.astype(_f32)


def image(h, w, seed=0):
    return np.random.default_rng(seed + 100).integers(0, 256, (h, w, 3), dtype=np.uint8)


def neighbour_invalid(k):
    """A 5x5 fronto-parallel plane whose centre pixel's neighbour k (right, left, below, above) is invalid: the centre and that
    neighbour's other neighbours lose their mask, the rest of the interior keeps it."""
    z = np.full((5, 5), 1.0, _f32)
    dv, du = ((0, 1), (0, -1), (1, 0), (-1, 0))[k]
    z[2 + dv, 2 + du] = 0.0
    return z


def trunc_edge(z0=1.0, z1=1.07):
    """-> (trunc, kept, dropped): two 3x3 depths whose right neighbour differs from the centre by exactly trunc in double (the mask
    keeps the centre) and by the next float32 above (it drops it).  trunc is the double difference of two float32 numbers, exact."""
    a, b = _f32(z0), _f32(z1)
    trunc = float(b) - float(a)
    kept = np.full((3, 3), a, _f32)
    kept[1, 2] = b
    dropped = kept.copy()
    dropped[1, 2] = np.nextafter(b, _f32(np.inf))
    assert float(dropped[1, 2]) - float(a) > trunc
    return trunc, kept, dropped


def bad_values(dtype=_f32):
    """A 7x9 frame with every kind of depth the level-0 rule turns into 0: NaN, +-inf, negative, zero, at and below depth_min,
    above depth_max; depth_max itself is valid.  -> (depth, depth_min, depth_max)"""
    z = np.full((7, 9), 1.5, _f32)
    z[1, 1], z[1, 4], z[1, 7] = np.nan, np.inf, -np.inf
    z[3, 2], z[3, 4], z[3, 6] = -1.0, 0.0, 0.5       # 0.5 == depth_min: invalid
    z[5, 2], z[5, 4], z[5, 6] = 3.0, np.nextafter(_f32(3.0), _f32(4.0)), 0.25  # 3.0 == depth_max: valid
    return z, 0.5, 3.0


# ---- closed-form surfaces for the normals ----------------------------------------------------------------------------------------

def plane_frame(T_cw, W=cf.W, H=cf.H, K=cf.K):
    """cf's plane seen from T_cw: -> (depth float32 [H,W], unit normal in the camera frame facing the camera)."""
    T_wc = np.linalg.inv(T_cw)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1) @ T_wc[:3, :3].T
    t = (cf.PLANE_D - T_wc[:3, 3] @ cf.PLANE_N) / (d @ cf.PLANE_N)
    n = T_cw[:3, :3] @ cf.PLANE_N
    return np.where(t > 0.05, t, 0.0).astype(_f32), (-n if n[2] > 0 else n)


def sphere_frame(W=320, H=240, K=(262.5, 262.5, 159.5, 119.5), centre=(0.05, -0.03, 1.2), radius=0.35):
    """A sphere in the camera frame: -> (depth float32 [H,W], 0 off the sphere; normals [H,W,3] (P - centre) / radius of the near hit)."""
    c = np.asarray(centre, np.float64)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1)
    a, b, cc = (d * d).sum(-1), d @ c, c @ c - radius * radius
    disc = b * b - a * cc
    with np.errstate(invalid="ignore"):
        t = np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0.0))) / a, 0.0)
    n = (t[..., None] * d - c) / radius
    return t.astype(_f32), np.where((t > 0)[..., None], n, 0.0)


# ---- the textured wall ---------------------------------------------------------------------------------------------------------

def perturbed(T_cw, axis_r, axis_t, deg, metres):
    """The camera moved by `deg` about axis_r and `metres` along axis_t (camera frame): the start rule of the tracking tests."""
    xi = np.concatenate([np.radians(deg) * np.asarray(axis_r, float) / np.linalg.norm(axis_r),
                         metres * np.asarray(axis_t, float) / np.linalg.norm(axis_t)])
    return np.linalg.inv(np.linalg.inv(T_cw) @ tr.exp_twist(xi))


WALL_STARTS = [((0, 0, 1), (1, 0, 0), 1.0, 0.02), ((1, 1, 0), (-1, 1, 0), 2.0, 0.03)]  # == tests/test_gpu_tsdf_track_color.py


def texture(p):
    """The wall's colour at world points p [...,3] (== tests/test_gpu_tsdf_track_color.texture)."""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    r = 0.5 + 0.25 * np.sin(9.0 * x + 2.0 * y) + 0.2 * np.sin(5.0 * y - 3.0 * z + 1.0)
    g = 0.5 + 0.25 * np.sin(7.0 * y + 3.0 * z + 0.5) + 0.2 * np.sin(11.0 * x + 0.3)
    b = 0.5 + 0.25 * np.sin(6.0 * x - 8.0 * y + 2.0) + 0.2 * np.sin(4.0 * z + 13.0 * x)
    return np.clip(np.stack([r, g, b], -1), 0.0, 1.0)


def wall_intrinsics(scale):
    """-> (K, W, H) of cf's camera at 1 / scale of its size"""
    return (np.array([cf.K[0] / scale, cf.K[1] / scale, (cf.K[2] + 0.5) / scale - 0.5, (cf.K[3] + 0.5) / scale - 0.5]), cf.W // scale,
            cf.H // scale)


def wall_frame(T_cw, scale):
    """cf's plane alone with the texture, seen from T_cw at (cf.W / scale) x (cf.H / scale): -> (depth float32, rgb uint8)"""
    K, W, H = wall_intrinsics(scale)
    T_wc = np.linalg.inv(T_cw)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1) @ T_wc[:3, :3].T
    t = (cf.PLANE_D - T_wc[:3, 3] @ cf.PLANE_N) / (d @ cf.PLANE_N)
    depth = np.where(t > 0.05, t, 0.0)
    rgb = np.rint(texture(T_wc[:3, 3] + depth[..., None] * d) * 255).astype(np.uint8)
    return depth.astype(_f32), rgb


def wall_cases():
    """[(name, scale, target pose, source pose)]: 160x120 and 320x240, cf.POSES[0] and [1], the source the target moved by WALL_STARTS"""
    return [("%dx%d pose %d start %d" % (cf.W // scale, cf.H // scale, p, s), scale, cf.POSES[p], perturbed(cf.POSES[p], *WALL_STARTS[s]))
            for scale in (4, 2) for p in (0, 1) for s in (0, 1)]


ROOM_PAIRS = [(40, 41), (40, 44), (100, 108)]  # (target, source) frames of SyntheticRGBD("synthetic_640x480_5mm")
