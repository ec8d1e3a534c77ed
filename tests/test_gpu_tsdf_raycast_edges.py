"""GPU: ScalableTSDFVolume.ray_cast (hv_raycast.hip) on planted voxel states (tests/planted_states.py) - the branches a camera
in front of a fused surface never takes.  Everything is held to tests/raycast_reference.py run on the planted volume's OWN dump.

The planted fields are smooth (planes, one sphere), so a last-bit difference cannot send a ray into another voxel: the edges are
structural.  On EXACT-INVERSE poses (a signed-permutation rotation, a dyadic translation: numpy's inverse and the library's
cofactor inverse are the same numbers, tests/test_planted_states_cpu.py) the 0.1 % allowance of
tests/test_gpu_tsdf_raycast.py::assert_agrees has no cause - the build does not contract and the reference follows the kernel
operation by operation - so there the masks are identical on EVERY pixel and EVERY common hit is inside the bars (|dz| <= 1e-4 m,
0.5 deg, colour 1e-4).  The one generic pose keeps assert_agrees as it is.  The analytic depths the interior rays are also held to
are shown for the reference in tests/test_planted_states_cpu.py.

Measured on the MI355X when the file was written: on every exact-inverse pose the masks are identical, depth is BITWISE equal to the
reference's (max dz 0), colour differs by 0 and normals by <= 0.02 deg; no ray is outside the bars.
"""
import numpy as np
import pytest

from tests import planted_states as ps
from tests import raycast_reference as rr
from tests.test_gpu_tsdf_deintegrate import assert_bitwise
from tests.test_gpu_tsdf_edges import volume
from tests.test_gpu_tsdf_raycast import assert_agrees
from tests.test_planted_states_cpu import (DEPTH_RANGES, GENERIC_CAST, check_depth_range_cases, check_interior_rays, check_weight_pattern,
                                           incomplete_hits, look_at)

pytestmark = pytest.mark.gpu

VOX, TRUNC = ps.VOX, ps.TRUNC


def planted(states):
    vol = volume(VOX, TRUNC)
    ps.plant(vol, states)
    assert_bitwise(vol.dump(), ps.as_dump(states))
    return vol


def K(intr=ps.INTR, height=ps.H, width=ps.W):
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    return PinholeCameraIntrinsic(width, height, *intr)


def assert_exact(gpu, ref, what, expect_hits=True):
    """assert_agrees without its allowance: identical masks, every common hit inside the bars."""
    mg, mr = np.asarray(gpu["mask"], bool), np.asarray(ref["mask"], bool)
    assert np.array_equal(mg, mr), (what, "masks differ on", int((mg != mr).sum()), "pixels")
    assert not gpu["depth"][~mg].any() and not gpu["normal"][~mg].any() and not gpu["color"][~mg].any() and not gpu["vertex"][~mg].any()
    if not mg.any():
        assert not expect_hits, (what, "no hit at all")
        print(f"{what}: no hits on either side")
        return
    dz = np.abs(gpu["depth"].astype(np.float64) - ref["depth"].astype(np.float64))[mg]
    cosang = np.clip((gpu["normal"].astype(np.float64) * ref["normal"].astype(np.float64)).sum(-1), -1.0, 1.0)[mg]
    ang = np.degrees(np.arccos(cosang))
    dc = np.abs(gpu["color"] - ref["color"]).max(-1)[mg]
    bitwise = np.array_equal(gpu["depth"].view(np.uint32), ref["depth"].view(np.uint32))
    print(f"{what}: {int(mg.sum())} hits, depth bitwise {'yes' if bitwise else 'no'}, max dz {dz.max():.3g} m, max normal {ang.max():.3g} deg, "
          f"max colour {dc.max():.3g}")
    assert dz.max() <= 1e-4 and ang.max() <= 0.5 and dc.max() <= 1e-4, (what, float(dz.max()), float(ang.max()), float(dc.max()))


def both_casts(vol, T, depth_min=0.1, depth_max=3.0, threshold=3.0, depth_scale=1.0):
    dump = vol.dump()
    gpu = vol.ray_cast(K(), T, depth_min, depth_max, weight_threshold=threshold, depth_scale=depth_scale)
    ref = rr.ray_cast(dump, VOX, TRUNC, ps.INTR, T, ps.H, ps.W, depth_min, depth_max, threshold, depth_scale)
    return gpu, ref, dump


# a ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,sign", ps.DIRECTIONS)
def test_six_viewing_directions(axis, sign):
    """The d[a] < 0 and d[a] == 0 arms of the unit-exit step (cameras looking along -x, -y, -z; the centre row and column have a
    zero direction component), absent units on the way to a surface (the unit layer next to the camera, the hole in the front
    wall), gv >> 4 on negative voxel indices."""
    states, scene = ps.two_walls(axis, sign)
    vol = planted(states)
    T = ps.camera_pose(axis, sign)
    gpu, ref, _ = both_casts(vol, T)
    what = f"axis {axis} sign {sign:+d}"
    assert_exact(gpu, ref, what)
    check_interior_rays(gpu, scene, what + " (GPU against the walls)")


# b ---------------------------------------------------------------------------------------------------------------------------
def test_weight_threshold():
    """The strict weight > threshold test at equality (threshold 3.0 on weights of 3; 4.0 on weights of 4: nothing is observed),
    a fractional threshold (2.5), and the have_prev reset across ONE unobserved voxel that splits a sign change: no hit there,
    the surface behind is found instead."""
    states, scene = ps.two_walls(2, 1)
    vol = planted(ps.weight_pattern(states, scene))
    T = ps.camera_pose(2, 1)
    outs = {}
    for thr in (2.5, 3.0, 4.0):
        outs[thr], ref, _ = both_casts(vol, T, threshold=thr)
        assert_exact(outs[thr], ref, f"threshold {thr}", expect_hits=thr < 4.0)
    check_weight_pattern(outs, scene)


# c ---------------------------------------------------------------------------------------------------------------------------
def test_depth_range_and_scale():
    """z < depth_max before a sample is taken (depth_max short of the wall; between the bracket's two samples), a start inside
    the surface (depth_min behind the front wall: f <= 0 without a previous sample is no hit), the depth_min clamp on za_out and
    the depth_max clamp on zb_out, and depth_scale != 1 (depth only; the vertex stays in metres)."""
    states, scene = ps.two_walls(2, 1)
    vol = planted(states)
    T = ps.camera_pose(2, 1)
    outs = {}
    for r in DEPTH_RANGES:
        outs[r], ref, _ = both_casts(vol, T, *r)
        assert_exact(outs[r], ref, f"depth range {r}", expect_hits=r != DEPTH_RANGES[0])
    check_depth_range_cases(outs, scene)
    plain, _, _ = both_casts(vol, T)
    scaled, ref, _ = both_casts(vol, T, depth_scale=1000.0)
    assert_exact(scaled, ref, "depth_scale 1000")
    np.testing.assert_array_equal(scaled["depth"], plain["depth"] * np.float32(1000.0))
    for a in ("vertex", "normal", "color", "mask"):
        np.testing.assert_array_equal(scaled[a], plain[a])


# d ---------------------------------------------------------------------------------------------------------------------------
def test_incomplete_neighbourhoods():
    """rc_tsdf_tri returning false inside the refinement (the loop ends at its first invalid sample), rc_color's nearest-voxel
    fallback and hv_tsdf_gradient with missing neighbour units: a tilted wall whose band touches the unit face x = 0, the unit
    beyond it absent."""
    vol = planted(ps.tilted_wall_at_a_missing_unit())
    gpu, ref, dump = both_casts(vol, ps.camera_pose(2, 1))
    assert_exact(gpu, ref, "tilted wall at a missing unit")
    bad = incomplete_hits(gpu, dump)
    assert bad.sum() == incomplete_hits(ref, dump).sum() == 24
    grid = rr._Grid(dump)
    p = gpu["vertex"][gpu["mask"]][bad]
    row, word = grid.locate(*(np.floor(p[:, a] / np.float32(VOX)).astype(np.int64) for a in range(3)))
    np.testing.assert_allclose(gpu["color"][gpu["mask"]][bad], grid.colour[row, word] / np.float32(255), rtol=0, atol=1e-6)


# e ---------------------------------------------------------------------------------------------------------------------------
def test_generic_pose_on_the_sparse_source():
    """A non-permutation pose on the sparse random source (20 % of the units missing, 10 % of the voxels unobserved, weights
    1..7 against a threshold of 0.5): unit skipping in every direction at once and resets inside the band; assert_agrees as is."""
    g = GENERIC_CAST
    vol = planted(ps.sparse_source(special=False))
    T = look_at(g["eye"], g["target"])
    dump = vol.dump()
    gpu = vol.ray_cast(K(g["intr"], g["height"], g["width"]), T, 0.1, 3.0, weight_threshold=g["threshold"])
    ref = rr.ray_cast(dump, VOX, TRUNC, g["intr"], T, g["height"], g["width"], 0.1, 3.0, g["threshold"])
    assert ref["mask"].sum() == 1919
    assert_agrees(gpu, ref, "generic pose on the sparse source")
