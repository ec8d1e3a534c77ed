"""Planted scenes for map-to-map registration (hv_register.hip, tests/register_reference.py) - test infrastructure, no GPU.
States are tests/planted_states.py's (keys, tsdf, weight, colour) tuples at VOX, TRUNC = 0.02, 0.08.

corner_and_sphere: the minimum of three mutually non-parallel tilted planes (a room corner) and a sphere - a field that fixes all
six degrees of freedom (planted_states.sphere_and_plane is symmetric about the axis through the sphere's centre along the plane's
normal).  Every voxel is observed (weights 4..7), nothing is overwritten with special values.  `frame` = F evaluates the same
analytic function in a frame moved by F (a point p of the map is the scene's F^-1 p) on the map's own lattice, so between a source
built with the identity and a destination built with T_true the ground truth T_dst_src = T_true is exact in the continuum.  The
cluster sits where tests/test_merge_reference_cpu.CAST_POSES look.

dyadic_plane: one axis-aligned plane, tsdf = (z0 - z) / sdf_trunc with z0 on a voxel face - multiples of 1/8, exact in float32 -
whose trilinear samples have gradients exactly along z: H has rank 3 (t_z and the two tilts), whatever the rounding.
"""
import itertools

import numpy as np

from tests import planted_states as ps
from tests.test_merge_reference_cpu import rigid

VOX, TRUNC = ps.VOX, ps.TRUNC
R_UNIT = ps.R  # voxels per unit side
CLUSTER = np.array(list(itertools.product(range(-1, 2), range(-2, 1), range(2, 5))), np.int64)  # 3 x 3 x 3 units
CENTRE = np.array([0.16, -0.16, 1.12])  # of the cluster's box

_PLANES = (((0.15, -0.25, 1.0), (0.0, 0.0, 0.28)), ((0.1, 1.0, 0.15), (0.0, 0.27, 0.0)), ((1.0, 0.2, 0.25), (0.29, 0.0, 0.0)))
_SPHERE = ((-0.12, -0.08, -0.10), 0.2)

# the destination's frame, the 1-voxel / 1-degree error of the initial guess (about the cluster's centre: what a pose graph hands
# over is wrong where the maps are, not at the world origin), and the guess
T_TRUE = rigid((0.3, 1.0, 0.2), 5.0, (0.037, -0.026, 0.019))


def about(centre, T):
    """T applied about `centre`: Tr(centre) T Tr(-centre)."""
    out = np.array(T, np.float64)
    out[:3, 3] = centre + T[:3, 3] - T[:3, :3] @ centre
    return out


PERTURBATION = about(CENTRE, rigid((-0.4, 0.5, 1.0), 1.0, np.array([1.0, -0.7, 0.5]) / np.linalg.norm([1.0, -0.7, 0.5]) * VOX))
INIT = T_TRUE @ PERTURBATION


def scene_sdf(p):
    """The analytic field in metres at scene points p [..., 3]: positive in free space."""
    d = np.linalg.norm(p - (CENTRE + _SPHERE[0]), axis=-1) - _SPHERE[1]
    for normal, through in _PLANES:
        n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
        d = np.minimum(d, (CENTRE + through) @ n - p @ n)
    return d


def corner_and_sphere(keys=CLUSTER, frame=None, seed=11):
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    p = ps.centres(keys)
    if frame is not None:
        F = np.asarray(frame, np.float64)
        p = (p - F[:3, 3]) @ F[:3, :3]  # F^-1 p, rows
    tsdf = np.clip(scene_sdf(p) / TRUNC, -1.0, 1.0).astype(np.float32)
    weight = rng.integers(4, 8, tsdf.shape).astype(np.float32)
    colour = rng.integers(0, 256, tsdf.shape + (3,)).astype(np.float64)
    return ps.finish(keys, tsdf, weight, colour)


DYADIC_KEYS = np.array([(i, j, 0) for i in range(-1, 2) for j in range(-1, 2)], np.int64)
DYADIC_Z0 = 8  # the plane is the lower face of voxel layer 8
DYADIC_INIT = ps.with_translation(ps.IDENTITY, (0.37, 0.61, 0.25))  # a quarter of a voxel along the normal, off the lattice across it


def dyadic_plane(keys=DYADIC_KEYS, seed=12):
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    iz = (keys[:, None, 2] * ps.R + ps._IDX[None, :, 2]).astype(np.float64)
    tsdf = np.clip((DYADIC_Z0 - (iz + 0.5)) * 0.25, -1.0, 1.0).astype(np.float32)  # (z0 - z) / TRUNC with VOX / TRUNC = 1 / 4
    weight = rng.integers(4, 8, tsdf.shape).astype(np.float32)
    colour = rng.integers(0, 256, tsdf.shape + (3,)).astype(np.float64)
    return ps.finish(keys, tsdf, weight, colour)


def shifted(states, units):
    """The same voxel values in units moved by `units` (whole unit indices)."""
    keys, tsdf, weight, colour = states
    return ps.finish(np.asarray(keys, np.int64) + np.asarray(units, np.int64), tsdf, weight, colour)


def brought_back(far_T, units, src_keys, voxel=VOX):
    """The guess that poses, near the origin, the problem `far_T` poses for a destination moved by `units` whole units.  At 2e5 m a
    double resolves 3e-11 m, so the far call's anchor c = T c_s is ROUNDED there, by up to 1.5e-11 m - a change of the problem, the
    same for every candidate, that moves g by H times as much (2e-9 of sum |terms| in this scene: it would drown what the
    comparison is about).  The translation returned makes the near call's anchor that rounded anchor less the shift, evaluated in
    rational arithmetic: both calls then linearise the same problem to 1e-17 m and differ by their own rounding only."""
    from fractions import Fraction

    far_T = np.asarray(far_T, np.float64)
    keys = np.asarray(src_keys, np.int64).reshape(-1, 3)
    cs = ((keys.min(0) + keys.max(0) + 1).astype(np.float64) * 0.5) * (16.0 * np.float64(voxel))
    out = far_T.copy()
    for a in range(3):
        r_cs = (far_T[a, 0] * cs[0] + far_T[a, 1] * cs[1]) + far_T[a, 2] * cs[2]
        c = r_cs + far_T[a, 3]
        out[a, 3] = float(Fraction(float(c)) - Fraction(int(units[a]) * R_UNIT) * Fraction(float(voxel)) - Fraction(float(r_cs)))
    return out


def few_voxels(count, unit=(0, -1, 3), tsdf=0.125, weight=5, seed=13):
    """One unit with exactly `count` observed voxels (tsdf inside every band), spread over the unit's words; the rest unobserved."""
    rng = np.random.default_rng(seed)
    t, w, c = np.zeros((1, ps.NV), np.float32), np.zeros((1, ps.NV), np.float32), np.zeros((1, ps.NV, 3))
    at = rng.choice(ps.NV, count, replace=False)
    t[0, at], w[0, at] = tsdf, weight
    return ps.finish([unit], t, w, c)


def pose_error(T, T_ref):
    """-> (translation error in metres at CENTRE, rotation error in degrees) of T against T_ref."""
    D = np.linalg.inv(T_ref) @ T
    cos = np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(D[:3, :3] @ CENTRE + D[:3, 3] - CENTRE)), float(np.degrees(np.arccos(cos)))


# ---- what a merge looks like afterwards ------------------------------------------------------------------------------------------
# tests/test_merge_reference_cpu.CAST_POSES through an 80 x 60 camera (the closed-form scene's 640 x 480 one, 8 times coarser)
CAST_H, CAST_W = 60, 80


def cast_intrinsics():
    from tests import tsdf_closed_form as cf

    return (cf.K[0] / 8.0, cf.K[1] / 8.0, (cf.K[2] + 0.5) / 8.0 - 0.5, (cf.K[3] + 0.5) / 8.0 - 0.5)


def depth_difference(casts, reference):
    """Mean |dz| in voxels over the pixels both lists of casts (one dict with depth and mask per pose) hit, and their number."""
    dz, n = 0.0, 0
    for a, b in zip(casts, reference):
        both = np.asarray(a["mask"], bool) & np.asarray(b["mask"], bool)
        dz += float(np.abs(np.asarray(a["depth"], np.float64)[both] - np.asarray(b["depth"], np.float64)[both]).sum())
        n += int(both.sum())
    return dz / max(n, 1) / VOX, n
