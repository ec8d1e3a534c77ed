"""Case builders for the VOXEL_GRID queries, carving and removal - numpy only, no GPU.

A case is a dict: name, voxel, bs, batches [(points f32 [N,3], colours f32 [N,3] | None)], steps.  Integrating the batches in order
IS the planting: a voxel that received one point holds that point bit for bit, one that received k points their ordered float32 sum.
Steps run in order on the same grid:

    ("all", min_count)   ("box", bb f64 [6], min_count)   ("frustum", frustum, min_count)        - queries, read only
    ("carve", frustum, depth f32 [H,W], threshold)   ("remove", min_count)   ("integrate", points, colours)   - edits

with frustum = dict(intr f32 [4], W, H, T_cw f64 [4,4], dmax, dmin).  A query step may carry a last element {"expect": n}: the number
of rows it must return.  run_case() drives any grid (oracle or GPU) through a case next to the numpy restatement
(tests/grid_query_reference.py), which always starts from the grid's own dump().
"""
import functools
import itertools

import numpy as np

from tests import grid_query_reference as qr
from tests import planted_states as ps
from tests.conftest import sort_rows

F32, F64 = np.float32, np.float64
SIZES = ((0.05, 5), (0.05, 4), (0.015, 8), (0.005, 16))
BOX_A = np.array([-0.31, -0.2, 0.1, 0.47, 0.33, 0.9])  # no bound is a float32
BOX_R = np.array([-0.5, -0.25, 0.25, 0.5, 0.375, 1.0])  # every bound is a float32


def prev32(x):
    return np.nextafter(F32(x), F32(-np.inf))


def next32(x):
    return np.nextafter(F32(x), F32(np.inf))


def keys32(points, voxel):
    """The voxel keys integrate() gives float32 points: floor(x * inv) in float32."""
    inv = F32(1.0) / F32(voxel)
    return np.floor(np.asarray(points, F32) * inv).astype(np.int64)


def assert_own_voxels(points, voxel):
    k = keys32(points, voxel)
    assert len(np.unique(k, axis=0)) == len(k), "two planted points share a voxel"


def colours(rng, n):
    return rng.random((n, 3), dtype=F32)


def frustum(intr, W, H, T_cw, dmax, dmin):
    return dict(intr=np.asarray(intr, F32), W=int(W), H=int(H), T_cw=np.ascontiguousarray(T_cw, F64).reshape(4, 4), dmax=float(F32(dmax)),
                dmin=float(F32(dmin)))


def min_counts(max_count):
    return (-1, 0, 1, 2, max_count, max_count + 1)


# ---- boxes ------------------------------------------------------------------------------------------------------------------------
def face_points(bb, voxel):
    """18 float32 points: prev / at / next float32 of each of the six bounds on its axis, the other two coordinates well inside the
    box and 1.5 voxels apart within a face's triple, so that every point has a voxel of its own."""
    lo, hi = bb[:3], bb[3:]
    mid = (lo + hi) / 2
    pts = []
    for a, bound in itertools.product(range(3), (0, 3)):
        at = F32(bb[bound + a])
        for j, x in enumerate((prev32(at), at, next32(at))):
            p = mid.copy()
            p[(a + 1) % 3] += (j - 1) * 1.5 * voxel
            p[(a + 2) % 3] += (0.37 if bound else -0.41) * voxel
            p = p.astype(F32)
            p[a] = x
            pts.append(p)
    pts = np.array(pts, F32)
    assert_own_voxels(pts, voxel)
    return pts


def counted_points(rng, centre, voxel, n_voxels=12):
    """Voxels with counts 1..4 around `centre`: count k = one point repeated (even voxels) or k distinct points of the voxel (odd
    ones: the mean is then no sample).  -> list of 4 batches; batch i holds the i-th point of every voxel that has one."""
    inv = F64(F32(1.0) / F32(voxel))
    base = np.floor(np.asarray(centre, F64) * inv).astype(np.int64)
    batches = [[] for _ in range(4)]
    for i in range(n_voxels):
        cell = base + np.array([i % 3 + 1, (i // 3) % 3 + 1, i // 9 + 1])
        k = i % 4 + 1
        first = ((cell + 0.3 + 0.4 * rng.random(3)) / inv).astype(F32)
        for j in range(k):
            p = first if i % 2 == 0 else ((cell + 0.3 + 0.4 * rng.random(3)) / inv).astype(F32)
            assert (keys32(p, voxel) == cell).all()
            batches[j].append(p)
    return [np.array(b, F32) for b in batches]


def box_faces_case(voxel, bs, bb, tag):
    rng = np.random.default_rng(11)
    faces = face_points(bb, voxel)
    extra = counted_points(rng, (bb[:3] + bb[3:]) / 2, voxel)
    batches = [(np.concatenate([faces, extra[0]]), colours(rng, 18 + len(extra[0])))] + [(e, colours(rng, len(e))) for e in extra[1:]]
    steps = []
    for mc in min_counts(4):
        steps += [("box", bb, mc), ("all", mc)]
    # a box on one planted position (float32 and float64 keys of that coordinate agree), inverted, off the map, around everything
    inv32, inv64 = F32(1.0) / F32(voxel), qr.inv_voxel(voxel)
    one = next(p for p in faces if (np.floor(p * inv32) == np.floor(p.astype(F64) * inv64)).all())
    steps += [("box", np.concatenate([one, one]).astype(F64), 1, {"expect": 1}),
              ("box", np.concatenate([bb[3:], bb[:3]]), 1, {"expect": 0}),
              ("box", np.array([50.0, 50.0, 50.0, 51.0, 51.0, 51.0]), 1, {"expect": 0}),
              ("box", np.array([-9000.0] * 3 + [9000.0] * 3), 1, {"expect": 18 + 12})]
    return dict(name=f"box_faces_{tag}_{voxel}_{bs}", voxel=voxel, bs=bs, batches=batches, steps=steps)


def box_origin_case(voxel, bs):
    """Blocks keyed -1 and 0 on every axis; boxes across the origin, on exact voxel and block multiples and off them."""
    rng = np.random.default_rng(12)
    v = F64(F32(voxel))
    idx = sorted({-bs, 1 - bs, -2, -1, 0, 1, bs - 2, bs - 1})
    cells = np.array(list(itertools.product(idx, repeat=3)), F64)
    pts = ((cells + 0.25 + 0.5 * rng.random(cells.shape)) * v).astype(F32)
    assert (keys32(pts, voxel) == cells).all()
    steps = [("all", 1)]
    for lo, hi in (((-1.5, -0.5, -2.0), (0.5, 1.5, 1.0)), ((-2.0, -2.0, -2.0), (1.0, 1.0, 1.0)), ((-bs, -bs, -bs), (0, 0, 0)),
                   ((-1.0, -float(bs), 0.0), (float(bs), 0.0, 2.0)), ((-0.001, -0.001, -0.001), (0.001, 0.001, 0.001)),
                   ((-bs + 0.5, -1.5, -1.5), (-0.5, 1.5, bs - 1.5))):
        steps.append(("box", np.array(lo + hi, F64) * v, 1))
    steps.append(("frustum", frustum((64, 48, 16, 12), 32, 24, ps.camera_pose(2, 1, np.array([0.0, 0.0, -2.0 * bs * v])), 3.0 * bs * v, 0.0), 1))
    return dict(name=f"box_origin_{voxel}_{bs}", voxel=voxel, bs=bs, batches=[(pts, colours(rng, len(pts)))], steps=steps)


def key_disagreements(voxel, limit=4):
    """float32 coordinates a hair below / above voxel multiples whose float32 key (what integrate() files them under) differs from
    the float64 key (what a box bound equal to them becomes).  -> [(x, key32, key64)], at most `limit`.  Always key32 == key64 + 1:
    the float64 product of two float32 numbers is exact, rounding it to float32 is monotonic and the integers in reach are float32
    numbers, so the float32 product can be rounded UP onto an integer the exact product lies below, never down past one."""
    inv32, inv64 = F32(1.0) / F32(voxel), qr.inv_voxel(voxel)
    k = np.arange(-4000, 4001, dtype=np.int64)
    at = (k.astype(F64) * F64(F32(voxel))).astype(F32)
    cand = np.concatenate([at, np.nextafter(at, F32(-np.inf)), np.nextafter(at, F32(np.inf)), (k.astype(F64) / inv64).astype(F32)])
    cand = cand[np.abs(cand) > 4 * voxel]
    k32 = np.floor(cand * inv32).astype(np.int64)
    k64 = np.floor(cand.astype(F64) * inv64).astype(np.int64)
    assert (k32 >= k64).all()
    pick = np.nonzero(k32 > k64)[0]
    pick = np.concatenate([pick[:limit // 2], pick[-(limit - limit // 2):]])  # negative and positive coordinates
    return [(cand[i], int(k32[i]), int(k64[i])) for i in pick]


def box_hair_case(voxel, bs):
    """Boxes whose UPPER bound on one axis IS the coordinate of a planted point found by key_disagreements(): the point is inside the
    box by position (closed faces) and outside it by key (its float32 key is one above the bound's float64 key), so the query must
    drop it.  The same coordinate as a LOWER bound keeps it (the bound's key is one below): both boxes are asked.  The CPU search finds
    such coordinates at every SIZES voxel size, also at 0.005 where float32(1 / 0.005) == 200 exactly."""
    rng = np.random.default_rng(13)
    found = key_disagreements(voxel)
    pts, steps = [], []
    for i, (x, k32, k64) in enumerate(found):
        a = i % 3
        p = np.array([0.31, -0.27, 0.43]) + 0.11 * rng.random(3)
        p[a] = x
        p = p.astype(F32)
        pts.append(p)
        bb = np.concatenate([p.astype(F64) - 0.2, p.astype(F64) + 0.2])
        for side in (3, 0):
            b = bb.copy()
            b[side + a] = F64(x)
            steps.append(("box", b, 1))
    pts = np.array(pts, F32).reshape(-1, 3)
    if len(pts):
        assert_own_voxels(pts, voxel)
    cloud = ((rng.random((60, 3)) - 0.5) * min(1.2, 40 * voxel)).astype(F32)  # a few blocks of bystanders around the origin
    return dict(name=f"box_hair_{voxel}_{bs}", voxel=voxel, bs=bs,
                batches=[(np.concatenate([pts, cloud]), colours(rng, len(pts) + 60))], steps=steps + [("all", 1)])


# ---- launch tails -------------------------------------------------------------------------------------------------------------------
def _tail_steps(pts):
    lo, hi = pts.min(axis=0).astype(F64), pts.max(axis=0).astype(F64)
    mid = (lo + hi) / 2
    cam = ps.camera_pose(2, 1, np.array([mid[0], mid[1], lo[2] - 1.0]))
    fr = frustum((64, 48, 16, 12), 32, 24, cam, 1.0 + (hi[2] - lo[2]) * 0.75, 0.5)
    depth = np.full((24, 32), 1.0 + (hi[2] - lo[2]) * 0.5, F32)
    return [("all", 1), ("all", 0), ("box", np.concatenate([lo, mid]), 1), ("box", np.concatenate([lo - 1, hi + 1]), 1), ("frustum", fr, 1),
            ("carve", fr, depth, 0.0), ("all", 1), ("remove", 2), ("all", 0)]


def tail_cases():
    rng = np.random.default_rng(14)
    out = []
    # 1 block, bs 5
    pts = ((np.array([[0, 0, 0], [4, 4, 4], [2, 3, 1], [4, 0, 2]]) + 0.5) * 0.05).astype(F32)
    out.append(dict(name="tail_one_block", voxel=0.05, bs=5, batches=[(pts, colours(rng, 4)), (pts[:2], colours(rng, 2))], steps=_tail_steps(pts)))
    # 3 blocks at bs 5: 375 voxels, one workgroup and a tail
    cells = np.concatenate([rng.integers(0, 5, (30, 3)) + 5 * np.array(b) for b in ((0, 0, 0), (-1, 0, 0), (0, -1, 1))])
    pts = ((cells + 0.5) * F64(F32(0.05))).astype(F32)
    assert (keys32(pts, 0.05) == cells).all()
    out.append(dict(name="tail_three_blocks_bs5", voxel=0.05, bs=5, batches=[(pts, colours(rng, len(pts)))], steps=_tail_steps(pts)))
    # one bs 8 block with all 512 voxels observed
    cells = np.array(list(itertools.product(range(8), repeat=3)), F64)
    pts = ((cells + 0.25 + 0.5 * rng.random(cells.shape)) * F64(F32(0.015))).astype(F32)
    assert (keys32(pts, 0.015) == cells).all()
    out.append(dict(name="tail_full_block_bs8", voxel=0.015, bs=8, batches=[(pts, colours(rng, 512)), (pts[::3], colours(rng, len(pts[::3])))],
                    steps=_tail_steps(pts)))
    # exactly one observed voxel in every 64 consecutive pool slots (bs 8: 8 groups of 64 per block, whatever the block order)
    cells = []
    for b, key in enumerate(((0, 0, 0), (1, 0, 0), (-1, -1, 0), (0, 2, -1), (3, -2, 1))):
        for g in range(8):
            l = 64 * g + (g * 9 + b * 5) % 64
            cells.append(np.array(key) * 8 + np.array([l % 8, (l // 8) % 8, l // 64]))
    cells = np.array(cells, F64)
    pts = ((cells + 0.5) * F64(F32(0.015))).astype(F32)
    assert (keys32(pts, 0.015) == cells).all()
    out.append(dict(name="tail_one_per_64", voxel=0.015, bs=8, batches=[(pts, colours(rng, len(pts)))], steps=_tail_steps(pts)))
    return out


def scattered_batches(rng, voxel, bs, n_blocks=40):
    """About 40 blocks with negative and positive keys, 12 observed voxels each with counts 1..4 from distinct points."""
    keys = np.unique(rng.integers(-6, 6, (n_blocks, 3)), axis=0)
    cells = np.concatenate([k * bs + rng.integers(0, bs, (12, 3)) for k in keys])
    cells = np.unique(cells, axis=0)
    count = rng.integers(1, 5, len(cells))
    v = F64(F32(voxel))
    batches = []
    for j in range(4):
        c = cells[count > j]
        p = ((c + 0.25 + 0.5 * rng.random(c.shape)) * v).astype(F32)
        assert (keys32(p, voxel) == c).all()
        batches.append((p, colours(rng, len(p))))
    return batches


def scattered_case(voxel=0.05, bs=5):
    rng = np.random.default_rng(15)
    batches = scattered_batches(rng, voxel, bs)
    span = 6 * bs * voxel
    steps = []
    for mc in min_counts(4):
        steps += [("all", mc), ("box", np.array([-0.4 * span, -span, -0.3 * span, 0.5 * span, 0.6 * span, span]), mc),
                  ("frustum", frustum((9.7, 7.3, 16.4, 8.1), 33, 17, generic_pose(), 2.0 * span, 0.1), mc)]
    return dict(name=f"scattered_{voxel}_{bs}", voxel=voxel, bs=bs, batches=batches, steps=steps)


def remove_cases(voxel=0.05, bs=5):
    out = []
    for mc in (-1, 0, 1, 2, 4, 5, 2 ** 31 - 1):
        rng = np.random.default_rng(16)
        batches = scattered_batches(rng, voxel, bs, n_blocks=12)
        steps = [("remove", mc), ("all", 1), ("all", 0), ("integrate",) + batches[0], ("all", 1), ("remove", 2), ("all", 1)]
        out.append(dict(name=f"remove_{mc}", voxel=voxel, bs=bs, batches=batches, steps=steps))
    return out


# ---- frusta -----------------------------------------------------------------------------------------------------------------------
EXACT_INTR, EXACT_W, EXACT_H = (64.0, 48.0, 16.0, 12.0), 32, 24


def generic_pose():
    """A rigid pose with no special entry: rotation by 0.7 rad about (1, 2, 3) / |.|, translation (0.13, -0.21, 0.37)."""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)
    T[:3, 3] = (0.13, -0.21, 0.37)
    return T


def to_world(T_cw, pc):
    """float32 world points of float64 camera points under a rigid T_cw."""
    R, t = T_cw[:3, :3], T_cw[:3, 3]
    return ((np.asarray(pc, F64) - t) @ R).astype(F32)  # R^T (pc - t), row form


def edge_points(T_cw, dmin, dmax, scale=1.0):
    """Camera points of the 32 x 24 exact camera at u in {just below 0, 0, 31, prev(32), 32} (each on a pixel row of its own), the
    same for v against 24, depths {prev(min), min, max, next(max)} (each on a pixel of its own), behind the camera, and each with its
    float32 neighbours along every world axis: under the identity pose the projections are exact, under another pose the neighbours
    put a point to each side of the edge.  "Just below 0" is u = -2^-19: u is computed in float64 and then narrowed, and no float32
    point of this camera projects onto the float32 below 0, so the lower image edge is pinned by u == 0 (inside) and this point (outside)."""
    fx, fy, cx, cy = EXACT_INTR
    pc = []
    for i, u in enumerate((-2.0 ** -19, 0.0, 31.0, float(prev32(32)), 32.0)):
        for z in (1.0 * scale, 2.0 * scale):
            pc.append(((u - cx) / fx * z, (2.0 + 4 * i + (z > scale) * 2 + 0.5 - cy) / fy * z, z))
    for i, v in enumerate((-2.0 ** -19, 0.0, 23.0, float(prev32(24)), 24.0)):
        for z in (1.0 * scale, 2.0 * scale):
            pc.append(((3.0 + 6 * i + (z > scale) * 3 + 0.5 - cx) / fx * z, (v - cy) / fy * z, z))
    for i, z in enumerate((prev32(dmin), F32(dmin), F32(dmax), next32(dmax))):
        pc.append(((4.0 + 6 * i - cx) / fx * float(z), (5.0 + 3 * i - cy) / fy * float(z), float(z)))
    pc.append((0.0, 0.0, -1.0 * scale))
    pc.append((0.1 * scale, -0.1 * scale, -0.5 * scale))
    w = to_world(T_cw, np.array(pc, F64))
    out = [w]
    for a in range(3):
        for toward in (-np.inf, np.inf):
            n = w.copy()
            n[:, a] = np.nextafter(w[:, a], F32(toward))
            out.append(n)
    return np.concatenate(out)


def frustum_case(name, T_cw, voxel, bs, scale=1.0):
    """`scale` (a power of two, so that the projections stay exact) shrinks the scene to keep a fine grid small."""
    rng = np.random.default_rng(17)
    dmin, dmax = 0.5 * scale, 2.0 * scale
    pts = edge_points(T_cw, dmin, dmax, scale)
    # z_c == 0 (the camera centre's plane) for the depth_min == 0 query: x / 0 and 0 / 0 must end as "outside"
    zero = to_world(T_cw, np.array([[0.1, 0.05, 0.0], [0.0, 0.0, 0.0], [-0.2, 0.0, 0.0]]) * scale)
    cloud = to_world(T_cw, np.stack([(rng.random(300) - 0.5) * 1.4, (rng.random(300) - 0.5) * 1.4, rng.random(300) * 2.6 - 0.3], axis=1) * scale)
    allp = np.concatenate([pts, zero, cloud])
    fr = frustum(EXACT_INTR, EXACT_W, EXACT_H, T_cw, dmax, dmin)
    fr0 = frustum(EXACT_INTR, EXACT_W, EXACT_H, T_cw, dmax, 0.0)
    steps = [("frustum", fr, 1), ("frustum", fr0, 1), ("frustum", fr, 2), ("frustum", fr, 0), ("all", 1)]
    return dict(name=name, voxel=voxel, bs=bs, batches=[(allp, colours(rng, len(allp)))], steps=steps)


def generic_frustum_case(voxel=0.05, bs=4):
    """One generic rigid pose at 33 x 17 with non-dyadic intrinsics over a cloud that overflows the frustum on every side."""
    rng = np.random.default_rng(18)
    T = generic_pose()
    pc = np.stack([(rng.random(2500) - 0.5) * 1.2, (rng.random(2500) - 0.5) * 0.8, rng.random(2500) * 1.1 - 0.1], axis=1)
    pts = to_world(T, pc)
    fr = frustum((31.7, 29.3, 16.4, 8.1), 33, 17, T, 0.85, 0.15)
    depth = (0.5 + 0.25 * rng.random((17, 33))).astype(F32)
    steps = [("frustum", fr, 1), ("frustum", fr, 2), ("carve", fr, depth, 0.03), ("frustum", fr, 1), ("all", 1)]
    return dict(name="frustum_generic_33x17", voxel=voxel, bs=bs, batches=[(pts, colours(rng, len(pts)))], steps=steps)


# ---- carving ----------------------------------------------------------------------------------------------------------------------
def solve_image_depth(target, thr):
    """A float32 image depth d with float32(d - thr) == target, or None."""
    thr = F32(thr)
    d = F32(F32(target) + thr)
    for _ in range(8):
        got = F32(d - thr)
        if got == F32(target):
            return d
        d = next32(d) if got < F32(target) else prev32(d)
    return None


def just_below(pixel, c, f, z):
    """(Within a quarter ulp of) the largest float32 camera coordinate x at depth z whose projection float32(f * (x / z) + c), computed as the frustum test does,
    is still below the integer `pixel`: the point then reads pixel - 1 at "pixel - 1 + 0.999...".  (The exact preimage of
    prev32(pixel) is in general no float32.)"""
    pixel = np.asarray(pixel, F64)
    x = ((pixel - c) / f * z).astype(F32)
    step = (np.spacing(pixel.astype(F32)).astype(F64) * z / f / 4).astype(F32)  # a quarter of a pixel-coordinate ulp: x may be 0
    for _ in range(32):
        over = (F64(f) * (x.astype(F64) / F64(z)) + F64(c)).astype(F32) >= pixel
        if not over.any():
            return x.astype(F64)
        x = np.where(over, np.minimum(np.nextafter(x, F32(-np.inf)), x - step), x)
    raise AssertionError("no float32 coordinate found below the pixel edge")


def carve_case(voxel, bs, thr, T_cw=None, tag="identity"):
    """The exact 32 x 24 camera over two sheets of points and a row of singletons:

    * sheet 1, depth Z: one point per pixel at (k + 0.5, r + 0.5) under a per-pixel checkerboard of a value that keeps it (0.75 Z) and
      one that carves it (1.25 Z): reading a neighbouring or the transposed pixel flips the voxel's fate;
    * sheet 2, depth 1.5 Z: points at the last float32 coordinates that project below k + 1 and r + 1 ("k + 0.999...", just_below())
      for every third column and row, last
      column and row included.  The image is rewritten around them: pixel (r, k) holds 1.25 Z, which keeps the sheet-2 voxel (and
      carves the sheet-1 voxel under it), and (r, k + 1), (r + 1, k), (r + 1, k + 1), where they exist, hold 1.75 Z, which carves
      both sheets.  The rule keeps every sheet-2 voxel; rounding u or v to the next pixel carves it (case["sheet2"] holds the points);
    * singletons at depth 0.75 Z on rows 1, 4, 7 whose pixel holds d with float32(d - thr) == point_depth, and the float32 to each side;
    * pixels set to 0, -1, NaN, +inf, -inf and the smallest positive float32 under points of sheet 1.  Of these only +inf can change a
      voxel's fate when the validity test is dropped: an image depth <= 0 (or NaN, or 1e-45) never exceeds point_depth + thr at
      thresholds above -depth_min, so a kernel without the `<= 0` test is NOT told apart here, one without the finiteness test is.
    Z = 4 at voxel 0.05, 1 at 0.015 (pixel pitch 1 / 64 m), 0.25 at 0.005 (pitch below the voxel: sheet-1 neighbours share voxels
    and their mean's pixel decides)."""
    rng = np.random.default_rng(19)
    T_cw = np.eye(4) if T_cw is None else T_cw
    fx, fy, cx, cy = EXACT_INTR
    W, H = EXACT_W, EXACT_H
    Z = 4.0 if voxel > 0.02 else 1.0 if voxel > 0.01 else 0.25
    kk, rr = np.meshgrid(np.arange(W), np.arange(H))
    sheet1 = np.stack([(kk + 0.5 - cx) / fx * Z, (rr + 0.5 - cy) / fy * Z, np.full(kk.shape, Z)], axis=-1).reshape(-1, 3)
    depth = np.where((kk + rr) % 2 == 0, 0.75 * Z, 1.25 * Z).astype(F32)
    Z2 = 1.5 * Z
    ks, rs = np.unique(np.concatenate([np.arange(1, W, 3), [W - 1]])), np.unique(np.concatenate([np.arange(2, H, 3), [H - 1]]))
    k2, r2 = np.meshgrid(ks, rs)
    for r, k in zip(r2.ravel(), k2.ravel()):
        depth[r:r + 2, k:k + 2] = 1.75 * Z  # the pixels a rounded u or v would read (clipped at the last column and row)
        depth[r, k] = 1.25 * Z
    # invalid pixels, on rows and columns sheet 2 does not use (sheet 1 points underneath would otherwise be carved or kept)
    for (r, k), val in zip(((1, 5), (1, 6), (4, 5), (4, 8), (7, 9), (7, 11), (22, 30), (1, 0)),
                           (0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45, np.nan, np.inf)):
        depth[r, k] = val
    sheet2 = np.stack([just_below(k2 + 1, cx, fx, Z2), just_below(r2 + 1, cy, fy, Z2), np.full(k2.shape, Z2)], axis=-1).reshape(-1, 3)
    Z3 = F32(0.75 * Z)
    single, targets = [], (prev32(Z3), Z3, next32(Z3))
    for j in range(9):
        r, k = 1 + 3 * (j // 3), 12 + 2 * (j % 3) + 7 * (j // 3 % 2)
        single.append(((k + 0.5 - cx) / fx * float(Z3), (r + 0.5 - cy) / fy * float(Z3), float(Z3)))
        d = solve_image_depth(targets[j % 3], thr)
        if d is not None and np.isfinite(d) and d > 0:
            depth[r, k] = d
    pts = to_world(T_cw, np.concatenate([sheet1, sheet2, np.array(single)]))
    cols = colours(rng, len(pts))
    fr = frustum(EXACT_INTR, W, H, T_cw, 3.0 * Z, 0.25 * Z)
    steps = [("all", 1), ("carve", fr, depth, thr), ("all", 1), ("carve", fr, depth, thr), ("integrate", pts, cols), ("all", 1),
             ("frustum", fr, 1), ("carve", fr, depth.T.copy().reshape(H, W), thr), ("all", 1)]
    return dict(name=f"carve_{tag}_{voxel}_{bs}_thr{thr}", voxel=voxel, bs=bs, batches=[(pts, cols)], steps=steps,
                sheet2=pts[len(sheet1):len(sheet1) + len(sheet2)])


def voxels_holding(dump, points):
    """-> bool [B, nvox]: the voxels with count 1 whose position is one of `points`, bit for bit."""
    want = {p.tobytes() for p in np.ascontiguousarray(points, F32)}
    pos = np.ascontiguousarray(dump[3][..., :3])
    hit = np.array([p.tobytes() in want for p in pos.reshape(-1, 3)]).reshape(dump[2].shape)
    return hit & (dump[2] == 1)


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = []
    for voxel, bs in SIZES:
        cases.append(box_faces_case(voxel, bs, BOX_A, "nonrep"))
        cases.append(box_hair_case(voxel, bs))
    cases += [box_faces_case(0.05, 5, BOX_R, "rep"), box_faces_case(0.015, 8, BOX_R, "rep")]
    cases += [box_origin_case(0.05, 5), box_origin_case(0.05, 4), box_origin_case(0.015, 8)]
    cases += tail_cases()
    cases += [scattered_case()] + remove_cases()
    cases.append(frustum_case("frustum_identity", np.eye(4), 0.015, 8))
    for axis, sign in ((0, 1), (1, -1), (2, -1)):
        cases.append(frustum_case(f"frustum_perm_{axis}_{sign}", ps.camera_pose(axis, sign), 0.05, 5))
    cases.append(frustum_case("frustum_identity_bs16", np.eye(4), 0.005, 16, scale=0.125))
    cases.append(generic_frustum_case())
    for thr in (0.0, 0.03, -0.01, 1e9):
        cases.append(carve_case(0.015, 8, thr))
    cases += [carve_case(0.05, 5, 0.03), carve_case(0.005, 16, 0.03), carve_case(0.05, 4, 0.03, ps.camera_pose(1, -1), "perm_1_-1")]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


CASE_NAMES = tuple(c["name"] for c in all_cases())


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


# ---- running a case -------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def sorted_rows(points, colors):
    """Rows [n,6] sorted lexicographically (NaN rows last)."""
    r = np.hstack([np.asarray(points, F32).reshape(-1, 3), np.asarray(colors, F32).reshape(-1, 3)])
    return sort_rows(r)[0]


def assert_rows_equal(a, b, what=""):
    """Two sorted row sets are equal bit for bit; NaN (the 0 / 0 of an empty voxel) equals NaN whatever its payload."""
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), what
    assert np.array_equal(bits(a)[~na], bits(b)[~nb]), what


def assert_dumps_equal(a, b, what=""):
    assert a[0].shape == b[0].shape, (what, a[0].shape, b[0].shape)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), what
    assert np.array_equal(bits(a[3]), bits(b[3])), what


class OracleFront:
    """oracle.PortGrid / RefGrid behind the step vocabulary."""

    def __init__(self, grid):
        self.grid = grid

    def integrate(self, pts, cols):
        self.grid.integrate(pts, cols)

    def dump(self):
        return self.grid.dump()

    def size(self):
        return self.grid.size()

    def apply(self, step):
        g, kind = self.grid, step[0]
        if kind == "all":
            return g.get_voxels(step[1])
        if kind == "box":
            return g.get_voxels_in_bb(step[1], step[2])
        if kind == "frustum":
            f = step[1]
            return g.get_voxels_in_camera_frustrum(f["intr"], f["W"], f["H"], f["T_cw"], f["dmax"], f["dmin"], step[2])
        if kind == "carve":
            f = step[1]
            return g.carve(f["intr"], f["W"], f["H"], f["T_cw"], f["dmax"], f["dmin"], step[2], F32(step[3]))
        if kind == "remove":
            return g.remove_low_count_voxels(step[1])
        return g.integrate(step[1], step[2])


def run_case(c, front, others=(), on_step=None):
    """Drive `front` (and the fronts in `others`, kept in lock step) through case `c`.  Before every step the restatement is run on
    front's own dump(); after it: a query's rows equal the restatement's and every other front's, bit for bit as sorted sets, and the
    dump is unchanged; an edit's dump equals the restatement's and every other front's, and voxels the restatement does not reset are
    bitwise untouched.  on_step(i, step, dump_before, restated) is called for every step.  -> number of steps run."""
    fronts = (front,) + tuple(others)
    for pts, cols in c["batches"]:
        for f in fronts:
            f.integrate(pts, cols)
    voxel, bs = c["voxel"], c["bs"]
    before = front.dump()
    for o in fronts[1:]:
        assert_dumps_equal(before, o.dump(), (c["name"], "planting"))
    for i, step in enumerate(c["steps"]):
        what = (c["name"], i, step[0])
        want = qr.apply_step(before, step, voxel, bs)
        got = [f.apply(step) for f in fronts]
        after = front.dump()
        if on_step is not None:
            on_step(i, step, before, want)
        if want is None:  # integrate
            pass
        elif want[0] == "rows":
            rows = sorted_rows(want[2], want[3])
            for g in got:
                assert_rows_equal(sorted_rows(*g), rows, what)
            if isinstance(step[-1], dict):
                assert len(rows) == step[-1]["expect"], (what, len(rows))
            assert_dumps_equal(after, before, what + ("read only",))
        else:
            assert_dumps_equal(after, want[1], what)
            kept = want[1][2] == before[2]
            assert np.array_equal(after[2][kept], before[2][kept]) and np.array_equal(bits(after[3])[kept], bits(before[3])[kept]), what
        for o in fronts[1:]:
            assert_dumps_equal(after, o.dump(), what + ("oracle",))
        assert front.size() == int((after[2] > 0).sum()), what
        before = after
    return len(c["steps"])
