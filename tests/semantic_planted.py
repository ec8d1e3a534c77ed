"""TEST INFRASTRUCTURE ONLY - planted states for the semantic association, carving and segment tests.

Every state is planted through `integrate` point streams and every operation is a call of the grids' common interface, so the GPU
grid, oracle.semantic.PortSemGrid2 and RefSemGrid2 take the same `Case`.  The arithmetic is kept exact: voxel size 1/16, identity or
axis-swapping poses, fx = fy = 32, cx = 32, cy = 24 on a 64 x 48 image, one to four points per voxel at ONE position (the average is
that position), dyadic positions, depths and thresholds - a projection that is meant to land on a frustum plane lands on it in every
implementation, and nothing else is near one.

`count_votes` restates the visit predicate of iterate_voxels_in_camera_frustrum and process_point
(voxel_semantic_data_association.h:181-235) in numpy on a grid dump: with tests/assoc_rules_reference.py it predicts a call's map
without any of the code under test."""
import numpy as np

from tests.assoc_rules_reference import PENDING, SEEN

VOXEL = 0.0625
W, H = 64, 48
INTR = (32.0, 32.0, 32.0, 24.0)
IDENTITY = np.eye(4)
SWAP = np.array([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])  # camera (x, y, z) = world (y, z, x)
EPS = 2.0 ** -23
KINDS = (0, 1, 2, 3)  # voting, probabilistic, voting "2", probabilistic "2" (RefSemGrid2's kinds)


def pose_for(bs):
    return IDENTITY if bs in (4, 8) else SWAP


def to_world(pc, T):
    """Camera -> world for a pose whose rotation is a permutation (exact)."""
    return (np.asarray(pc, np.float64) - T[:3, 3]) @ T[:3, :3]


def block_keys(pw, bs):
    return np.floor(np.floor(np.asarray(pw) * 16.0) / bs).astype(np.int64)


def images(cls=-1, inst=-1):
    return np.full((H, W), cls, np.int32), np.full((H, W), inst, np.int32)


class Case:
    """A list of steps on one grid.  Steps: ("integrate", points f64 [n,3], colours f32 [n,3], class ids, object ids),
    ("assoc", dict), ("carve", dict)."""

    def __init__(self, name, bs, T=IDENTITY, depth_max=4.0, depth_min=0.25, next_id=1):
        self.name, self.bs, self.T, self.depth_max, self.depth_min, self.next_id = name, int(bs), T, depth_max, depth_min, next_id
        self.steps = []

    def integrate(self, pc, cls, obj, repeat=1):
        """Points in CAMERA coordinates of the case's pose; `repeat` (scalar or per point) = how many points land in each voxel."""
        pc = np.asarray(pc, np.float64).reshape(-1, 3)
        n = len(pc)
        cls = np.broadcast_to(np.asarray(cls, np.int32), (n,)).copy()
        obj = np.broadcast_to(np.asarray(obj, np.int32), (n,)).copy()
        rep = np.broadcast_to(np.asarray(repeat), (n,))
        pw = to_world(pc, self.T)
        col = np.stack([np.full(n, 0.25), np.full(n, 0.5), (np.arange(n) % 4) * 0.25], 1).astype(np.float32)
        for k in range(int(rep.max())):
            m = rep > k
            self.steps.append(("integrate", np.ascontiguousarray(pw[m]), np.ascontiguousarray(col[m]), cls[m], obj[m]))
        return self

    def assoc(self, cls_img, inst_img, depth=None, depth_threshold=0.25, do_carving=False, min_vote_ratio=0.5, min_votes=1):
        self.steps.append(("assoc", dict(cls_img=cls_img, inst_img=inst_img, depth=depth, depth_threshold=depth_threshold, do_carving=do_carving,
                                         min_vote_ratio=min_vote_ratio, min_votes=min_votes)))
        return self

    def carve(self, depth, depth_threshold=0.25):
        self.steps.append(("carve", dict(depth=depth, depth_threshold=depth_threshold)))
        return self

    def upto(self, n_assoc):
        """The case cut after its n-th association call (so that the state after EVERY call can be compared, not only the last)."""
        seen = 0
        for k, s in enumerate(self.steps if n_assoc > 0 else []):
            seen += s[0] == "assoc"
            if seen == n_assoc:
                self.steps = self.steps[: k + 1]
                break
        return self

    def n_assoc(self):
        return sum(s[0] == "assoc" for s in self.steps)

    def n_blocks(self):
        keys = {tuple(k) for s in self.steps if s[0] == "integrate" for k in block_keys(s[1], self.bs)}
        return len(keys)


def usable_depth(depth):
    """A depth image of the wrong shape counts as absent (voxel_semantic_data_association.h:114-124)."""
    return depth if depth is not None and np.asarray(depth).shape == (H, W) else None


def run_case(grid, case, before_assoc=None, raw_depth=False):
    """Drive `grid` (the oracle.semantic._Sem2Base interface) through the case.  -> [(map, next id before, next id after)] of the assoc
    steps.  raw_depth: hand a mis-shaped depth image on as it is (the GPU front checks shapes itself; the oracles take pointers)."""
    intr = np.array(INTR, np.float32)
    grid.set_next_object_id(case.next_id)
    out = []
    for step in case.steps:
        if step[0] == "integrate":
            grid.integrate(step[1], step[2], step[3], step[4], None)
            continue
        a = step[1]
        depth = a["depth"] if raw_depth else usable_depth(a["depth"])
        if step[0] == "carve":
            grid.carve(intr, W, H, case.T, case.depth_max, case.depth_min, depth, a["depth_threshold"])
            continue
        if before_assoc is not None:
            before_assoc(grid, a)
        before = grid.peek_next_object_id()
        m = grid.assign_object_ids_to_instance_ids(intr, W, H, case.T, case.depth_max, case.depth_min, a["cls_img"], a["inst_img"], depth,
                                                   a["depth_threshold"], a["do_carving"], a["min_vote_ratio"], a["min_votes"])
        out.append((dict(m), before, grid.peek_next_object_id()))
    return out


# ---- the visit predicate and process_point in numpy ---------------------------------------------------------------------------------
PLANES = ("depth_min", "depth_max", "u_low", "u_high", "v_low", "v_high")


def project(case, dump):
    """Every occupied voxel of a dump through CameraFrustrum::contains (camera_frustrum.cpp:175-196: double arithmetic, depth / u / v
    rounded to float32).  -> dict of flat arrays over the occupied voxels: block, cell, u, v, depth, inside, and per plane the
    voxels that plane alone rejects."""
    keys, ints, pos, _, conf = dump
    b, l = np.nonzero((ints[..., 0] >= 1) & (conf >= 0.0))
    p = pos[b, l] / ints[b, l, 0][:, None].astype(np.float64)
    R, t = case.T[:3, :3], case.T[:3, 3]
    pc = np.stack([(R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1] + R[r, 2] * p[:, 2]) + t[r] for r in range(3)], 1)
    fx, fy, cx, cy = (np.float64(np.float32(x)) for x in INTR)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = pc[:, 2].astype(np.float32)
        u = (fx * (pc[:, 0] / pc[:, 2]) + cx).astype(np.float32)
        v = (fy * (pc[:, 1] / pc[:, 2]) + cy).astype(np.float32)
    rej = dict(depth_min=depth < np.float32(case.depth_min), depth_max=depth > np.float32(case.depth_max), u_low=u < 0, u_high=u >= np.float32(W),
               v_low=v < 0, v_high=v >= np.float32(H))
    # the key range of the frustum's bounding box (voxel_block_grid.hpp:1339-1349)
    Rwc, twc = R.T, -(R.T @ t)
    corners = []
    for cu, cv in ((0.0, 0.0), (W, 0.0), (W, H), (0.0, H)):
        for d in (float(np.float32(case.depth_min)), float(np.float32(case.depth_max))):
            corners.append(Rwc @ np.array([(cu - cx) / fx * d, (cv - cy) / fy * d, d]) + twc)
    corners = np.array(corners)
    vmin, vmax = np.floor(corners.min(0) * 16.0), np.floor(corners.max(0) * 16.0)
    bs = case.bs
    vk = keys[b].astype(np.int64) * bs + np.stack([l % bs, (l // bs) % bs, l // (bs * bs)], 1)
    in_range = ((vk >= vmin) & (vk <= vmax)).all(1)
    inside = in_range & ~np.any(list(rej.values()), 0)
    return dict(block=b, cell=l, u=u, v=v, depth=depth, inside=inside, rejected=rej, in_range=in_range)


def count_votes(case, dump, a):
    """process_point on the voxels `project` lets through.  -> dict(pairs=[(instance, object | PENDING | SEEN, votes)] sorted,
    visited, pending (voxels waiting for an id), carved)."""
    _, ints, _, _, _ = dump
    pr = project(case, dump)
    depth_img = usable_depth(a["depth"])
    thr = np.float32(a["depth_threshold"])
    votes, n_pending, n_carved = {}, 0, 0
    for k in np.nonzero(pr["inside"])[0]:
        px = (int(pr["v"][k]), int(pr["u"][k]))
        _, obj, cls, _ = ints[pr["block"][k], pr["cell"][k]]
        ic, inst = a["cls_img"][px], a["inst_img"][px]
        if ic < 0 or cls < 0 or cls != ic or inst < 0:
            continue
        if depth_img is not None:
            d = np.float32(depth_img[px])
            if d <= 0 or not np.isfinite(d):
                continue
            if a["do_carving"] and pr["depth"][k] < d - thr:
                n_carved += 1
                continue
            if pr["depth"][k] > d + thr:
                continue
        if obj < 0:
            if inst == 0:
                obj = 0
            else:
                obj = PENDING
                n_pending += 1
        votes[(int(inst), int(obj))] = votes.get((int(inst), int(obj)), 0) + 1
    for inst in np.unique(a["inst_img"][(a["inst_img"] >= 0) & (a["cls_img"] >= 0)]):
        votes[(int(inst), SEEN)] = 1
    return dict(pairs=sorted((i, o, n) for (i, o), n in votes.items()), visited=int(pr["inside"].sum()), pending=n_pending, carved=n_carved,
                projection=pr)


def drive(grid, case, raw_depth=False, to_canon=None):
    """run_case with every association call PREDICTED from the grid's own dump just before it (count_votes + the rules reference) and
    checked: same instances, same next id, same objects - new ids up to a permutation among the ids handed out in that call (the
    reference hands them out in visit order, the rules reference and the GPU in ascending instance order).
    -> (records [dict(map=, next_id=, votes=)] with the maps in CANONICAL ids (the rules reference's), to_canon {grid id: canonical})."""
    from tests.assoc_rules_reference import decide

    to_canon = {} if to_canon is None else to_canon
    predicted = []

    def before(g, a):
        predicted.append(count_votes(case, g.dump(), a))

    records = []
    calls = [s[1] for s in case.steps if s[0] == "assoc"]
    for (got, nid0, nid1), cv, a in zip(run_case(grid, case, before, raw_depth), predicted, calls):
        exp, exp_next = decide(cv["pairs"], a["min_vote_ratio"], a["min_votes"], nid0)
        assert nid1 == exp_next, (case.name, nid0, nid1, exp_next)
        assert set(got) == set(exp), (case.name, got, exp)
        perm = {}
        for inst in exp:
            g, e = got[inst], exp[inst]
            if g != e:  # only ids new in this call may differ, and then one for one
                assert nid0 <= g < nid1 and nid0 <= e < nid1 and perm.get(g, e) == e, (case.name, inst, got, exp)
                perm[g] = e
        assert len(set(perm.values())) == len(perm), (case.name, perm)
        to_canon.update(perm)
        records.append(dict(map={i: to_canon.get(o, o) for i, o in got.items()}, next_id=nid1, votes=cv))
    return records, to_canon


def canonical_dump(dump, to_canon):
    keys, ints, pos, col, conf = dump[:5]
    ints = ints.copy()
    flat = ints[..., 1].copy()
    for a, b in to_canon.items():
        ints[..., 1][flat == a] = b
    return keys, ints, pos, col, conf


# ---- builders -------------------------------------------------------------------------------------------------------------------------
def frustum_edge_case(bs):
    """One voxel per frustum plane exactly on it (inside: u = 0, v = 0, depth = depth_min, depth = depth_max; outside: u = W, v = H),
    one at the float32 value next to each plane on the other side, every voxel alone in its block, blocks on both sides of the
    origin.  Half of the voxels carry object id 2, the others wait for one; all face instance 5."""
    T = pose_for(bs)
    c = Case(f"frustum_edge-bs{bs}", bs, T, depth_max=2.0, depth_min=0.5, next_id=7)
    # (what is fixed, as a function of the free lane value f and the depth z = 0.5, 1 or 2) - x / z and y / z stay exact
    specs = [
        ("u_on_0", lambda f, z: (-z, f * z, z), True), ("u_below_0", lambda f, z: (-(1 + EPS) * z, f * z, z), False),
        ("u_below_W", lambda f, z: ((1 - EPS) * z, f * z, z), True), ("u_on_W", lambda f, z: (z, f * z, z), False),
        ("v_on_0", lambda f, z: (f * z, -0.75 * z, z), True), ("v_below_0", lambda f, z: (f * z, -(0.75 + EPS) * z, z), False),
        ("v_below_H", lambda f, z: (f * z, (0.75 - EPS) * z, z), True), ("v_on_H", lambda f, z: (f * z, 0.75 * z, z), False),
        ("d_on_min", lambda f, z: (f * 0.5, -f * 0.5, 0.5), True), ("d_below_min", lambda f, z: (f * 0.5, -f * 0.5, 0.5 - 2.0 ** -25), False),
        ("d_on_max", lambda f, z: (f * 2.0, -f * 2.0, 2.0), True), ("d_above_max", lambda f, z: (f * 2.0, -f * 2.0, 2.0 + 2.0 ** -22), False),
    ]
    used, pts, names, inside = set(), [], [], []

    def place(make):  # the first (depth, lane) whose block is still empty
        for z in (1.0, 2.0, 0.5):
            for f in (0.15625, -0.15625, 0.40625, -0.40625, 0.65625, -0.65625):
                pc = np.array(make(f, z))
                key = tuple(block_keys(to_world(pc, T), bs))
                if key not in used:
                    used.add(key)
                    return pc
        raise AssertionError("no free block")

    for name, make, ok in specs:
        pts.append(place(make))
        names.append(name)
        inside.append(ok)
    pts = np.array(pts)
    c.points = pts
    assert len(used) == len(pts) and any(min(k) < 0 for k in used) and any(min(k) >= 0 for k in used)
    obj = np.where(np.arange(len(pts)) % 2 == 0, 2, -1)
    c.integrate(pts, 3, obj)
    cls_img, inst_img = images(3, 5)
    c.assoc(cls_img, inst_img)
    c.assoc(cls_img, inst_img)
    c.names, c.expected_inside = names, inside
    return c


DEPTH_KINDS = (0.0, -1.0, np.nan, np.inf, 0.75, 1.25, np.nextafter(np.float32(0.75), np.float32(0)), np.nextafter(np.float32(0.75), np.float32(1)),
               np.nextafter(np.float32(1.25), np.float32(1)), np.nextafter(np.float32(1.25), np.float32(2)))
DEPTH_VARIANTS = ("filter", "carve", "no_depth", "wrong_shape")


def _depth_filter_layout():
    i = np.arange(len(DEPTH_KINDS))
    x = (i - 5 + 0.5) / 16.0
    u = 32 + 2 * (i - 5) + 1
    return x, u


def depth_filter_image():
    _, u = _depth_filter_layout()
    img = np.ones((H, W), np.float32)
    img[:, u] = np.array(DEPTH_KINDS, np.float32)[None, :]
    return img


def depth_filter_case(bs, variant):
    """Voxels at depth exactly 1 facing image depths 0, -1, NaN, +inf, 1 -+ 0.25 and their float32 neighbours, depth_threshold 0.25:
    one row of voxels with object id 2 (two points each), one row waiting for an id."""
    c = Case(f"depth_filter-bs{bs}-{variant}", bs, pose_for(bs), next_id=7)
    x, _ = _depth_filter_layout()
    n = len(x)
    pts = np.concatenate([np.stack([x, np.full(n, 0.03125), np.ones(n)], 1), np.stack([x, np.full(n, -0.03125), np.ones(n)], 1)])
    c.integrate(pts, 3, np.r_[np.full(n, 2), np.full(n, -1)], repeat=np.r_[np.full(n, 2), np.full(n, 1)])
    cls_img, inst_img = images(3, 5)
    depth = dict(filter=depth_filter_image(), carve=depth_filter_image(), no_depth=None, wrong_shape=np.ones((H, W + 1), np.float32))[variant]
    for _ in range(2):
        c.assoc(cls_img, inst_img, depth, depth_threshold=0.25, do_carving=(variant == "carve"))
    return c


def carve_case(bs, which):
    """hv_carve on the depth-filter voxels / on the frustum-edge voxels (facing a far wall: everything in view is carved)."""
    if which == "depth":
        c = depth_filter_case(bs, "filter")
        c.steps = [s for s in c.steps if s[0] == "integrate"]
        return c.carve(depth_filter_image(), 0.25)
    c = frustum_edge_case(bs)
    c.steps = [s for s in c.steps if s[0] == "integrate"]
    return c.carve(np.full((H, W), 3.0, np.float32), 0.25)


def _label_layout():
    """-> x index i in [-12, 12), y index j in [-4, 4) of every voxel site at z = 1 (pixel u = 33 + 2 i, v = 25 + 2 j)."""
    i, j = np.meshgrid(np.arange(-12, 10), np.arange(-4, 4), indexing="ij")
    return i.ravel(), j.ravel()


def label_case(bs):
    """Column groups at depth 1: image class -1 | image instance -1 | instance 0 on voxels without an object id | class mismatch |
    voxels with object ids 2 and 9 | voxels without id (both facing instance 6) | voxels of class -1; instance 8 occurs in the image
    only where no voxel is.  One, two or four points per voxel; every block has empty cells."""
    c = Case(f"label-bs{bs}", bs, pose_for(bs), next_id=5)
    i, j = _label_layout()
    pts = np.stack([(i + 0.5) / 16.0, (j + 0.5) / 16.0, np.ones(len(i))], 1)
    cls = np.where((i >= -3) & (i < 0), 4, 3)
    cls = np.where(i >= 8, -1, cls)
    obj = np.full(len(i), -1)
    obj[(i >= 0) & (i < 2)] = 2
    obj[(i >= 2) & (i < 4)] = 9
    obj[i < -9] = 4
    c.integrate(pts, cls, obj, repeat=np.array([1, 2, 4])[(i + j) % 3])
    cls_img, inst_img = images(3, 6)
    u = lambda k: 33 + 2 * k  # noqa: E731
    cls_img[:, : u(-9)] = -1
    inst_img[:, u(-9) - 1: u(-6) - 1] = -1
    inst_img[:, u(-6) - 1: u(-3) - 1] = 0
    inst_img[:, u(10) - 1:] = 8
    c.assoc(cls_img, inst_img)
    c.assoc(cls_img, inst_img)
    return c


def dense_pending_case(bs):
    """Three fully occupied adjacent blocks (block size 5: two rows of three, to hold as many voxels) of class 3 without object ids -
    a wave scans a block: 512 queued and 512 waiting voxels at block size 8.  They face ONE instance with min_votes out of reach (nobody
    gets an id: all of them wait again), then four instances striped by image column, then the same stripes again (the ids given by
    the second call vote in the third)."""
    c = Case(f"dense_pending-bs{bs}", bs, pose_for(bs), next_id=3)
    n, rows = bs, (1 if bs >= 8 else 2)
    ix, iy, iz = np.meshgrid(np.arange(-n, 2 * n), np.arange(rows * n), np.arange(4 * n, 5 * n), indexing="ij")
    pts = np.stack([(ix.ravel() + 0.5) / 16.0, (iy.ravel() + 0.5) / 16.0, (iz.ravel() + 0.5) / 16.0], 1)  # (cells along z share pixels)
    c.integrate(pts, 3, -1)
    cls_img, one = images(3, 4)
    c.assoc(cls_img, one, min_votes=100000)
    stripes = np.broadcast_to(((np.arange(W) // 3) % 4 + 1).astype(np.int32), (H, W)).copy()
    c.assoc(cls_img, stripes)
    c.assoc(cls_img, stripes)
    return c


def dense_rows_case(bs):
    """One fully occupied bs^3 block and a second, sparse one (five voxels).  A wave scans a block 64 voxels at a time and pushes
    what it finds into its 512-entry window - rows of get_voxels, keys of get_object_segments - which flushes from inside a push once
    more than 448 wait.  Objects 10-12 by y, each of one class (1-3); bs voxels of the dense block (x = 0 of the top y layer) and two
    of the sparse one have no object id: rows of get_voxels, keys of no segment.  One point in every fourth voxel, two in the others.
    - bs 8: 512 rows and 504 keys: seven pushes fill a window to at most 448, the eighth flushes it; the scan's end finds it empty.
    - bs 12: 1728 rows and 1716 keys: every window flushes three times with the rest of the block still to come, so the pushes after
      a flush start at 0 again; with a count above 1 asked for (1296 rows, 1287 keys) the pushes are partial and the flushes fall at
      449..512 entries instead of at 512.
    c.planted = (object id or -1, points) of every voxel."""
    c = Case(f"dense_rows-bs{bs}", bs, IDENTITY)
    ix, iy, iz = np.meshgrid(np.arange(bs), np.arange(bs), np.arange(4 * bs, 5 * bs), indexing="ij")
    sx, sy, sz = np.array([0, 1, 3, bs - 2, bs - 1]), np.array([0, 1, 3, bs - 2, bs - 1]), np.array([0, 1, 3, bs - 2, bs - 1])
    ix, iy, iz = (np.concatenate([a.ravel(), b]) for a, b in zip((ix, iy, iz), (2 * bs + sx, sy, 4 * bs + sz)))
    pts = np.stack([(ix + 0.5) / 16.0, (iy + 0.5) / 16.0, (iz + 0.5) / 16.0], 1)
    obj = np.where((iy == bs - 1) & (ix % bs == 0), -1, iy % 3 + 10)
    obj[-2:] = -1
    rep = np.where((ix + iy + iz) % 4 == 0, 1, 2)
    c.integrate(pts, iy % 3 + 1, obj, repeat=rep)
    c.planted = (obj, rep)
    assert c.n_blocks() == 2
    return c


def scene_from_pairs(name, pairs, min_vote_ratio, min_votes, next_id, bs=8, calls=1):
    """A scene whose only association call casts exactly `pairs`: for (instance, object, n) n voxels with that object id (none for
    PENDING) under pixels of that instance, for (instance, SEEN, _) a pixel of that instance over no voxel; a SEEN marker is implied
    for every instance.  Voxel sites: depth 2, one per pixel."""
    c = Case(name, bs, IDENTITY, next_id=next_id)
    cls_img, inst_img = images(-1, -1)
    pts, objs, s = [], [], 0
    for inst, obj, n in pairs:
        for _ in range(1 if obj == SEEN else n):
            i, j = s % W - 32, s // W - 24
            s += 1
            cls_img[j + 24, i + 32], inst_img[j + 24, i + 32] = 1, inst
            if obj != SEEN:
                pts.append(((i + 0.5) / 16.0, (j + 0.5) / 16.0, 2.0))  # u = 32 + i + 0.5, v = 24 + j + 0.5: a voxel and a pixel of its own
                objs.append(-1 if obj == PENDING else obj)
    assert s <= W * H
    c.integrate(np.array(pts).reshape(-1, 3), 1, np.array(objs, np.int64))
    for _ in range(calls):
        c.assoc(cls_img, inst_img, min_vote_ratio=min_vote_ratio, min_votes=min_votes)
    c.pairs = sorted({(i, o, n) for i, o, n in pairs if o != SEEN} | {(i, SEEN, 1) for i, _, _ in pairs})
    return c


def many_pairs_case():
    """100 instances, each facing voxels of 3 of 20 existing objects with 3, 2 and 1 votes: 300 pairs and 100 markers."""
    pairs = []
    for k in range(100):
        for obj, n in zip((k % 20 + 1, (k + 7) % 20 + 1, (k + 13) % 20 + 1), (3, 2, 1)):
            pairs.append((k + 1, obj, n))
    return scene_from_pairs("many_pairs", pairs, 0.5, 3, 40, calls=2)


THIRD = float(np.float32(1.0 / 3.0))


def rule_scenes():
    """-> [(name, pairs, min_vote_ratio, min_votes, next id)]: exact ratios at the thresholds, totals at min_votes, ties, and a new
    id below / equal to / between / above the existing ids.  At most one instance needs a new id."""
    out = []
    ratio_sets = dict(half=[(4, 2, 1), (4, 3, 1)], third=[(4, 2, 1), (4, 3, 1), (4, 5, 1)], two_thirds=[(4, 3, 1), (4, 2, 2)])
    for rn, pairs in ratio_sets.items():
        for tn, thr in (("0.5", 0.5), ("third", THIRD), ("two_thirds", 2.0 / 3.0)):
            out.append((f"ratio_{rn}_at_{tn}", pairs, thr, 1, 20))
    out.append(("total_equals_min_votes", [(4, 2, 2), (4, 3, 1)], 0.5, 3, 20))
    out.append(("total_below_min_votes", [(4, 2, 2), (4, 3, 1)], 0.5, 4, 20))
    out.append(("tie_later_object_smaller_id", [(4, 9, 2), (4, 3, 2), (6, 1, 1), (6, 0, 1)], 0.5, 1, 20))
    out.append(("tie_three_way_with_instance_0", [(0, 3, 2), (0, 1, 2), (0, 2, 2), (4, 7, 1)], 0.25, 1, 20))
    for nn, nid in (("below", 3), ("equal", 5), ("between", 7), ("above", 12)):
        out.append((f"new_id_{nn}", [(4, 5, 2), (4, 9, 2), (4, PENDING, 2), (6, 9, 1)], 0.25, 1, nid))
    out.append(("new_id_equal_to_the_larger", [(4, 5, 3), (4, 9, 2), (4, PENDING, 2)], 0.25, 1, 9))
    out.append(("seen_only_and_instance_0", [(3, SEEN, 1), (0, SEEN, 1), (4, 2, 1)], 0.5, 1, 20))
    return out


def random_pairs(n, seed):
    """n pairs as several GPUs' lists concatenated would hold them: duplicates, ties, instance 0, PENDING and SEEN markers, object ids
    >= 0 otherwise (the reference never votes for a negative id; (0, PENDING) cannot occur: instance 0 gives object 0 at once)."""
    rng = np.random.default_rng(seed)
    n_inst = max(2, min(300, n // 3 + 1))
    inst = rng.integers(0, n_inst, n)
    obj = rng.integers(0, 12, n)
    kind = rng.random(n)
    obj = np.where(kind < 0.15, SEEN, np.where((kind < 0.30) & (inst != 0), PENDING, obj))
    votes = rng.integers(1, 4, n)
    return [(int(i), int(o), int(v)) for i, o, v in zip(inst, obj, votes)]


def overflow_label_case():
    """Voxels with 7 and with 13 distinct (object, class) observations (the probabilistic payloads keep 6 inline); the leading pair -
    (2, 3) - was observed three times, every other once: it leads by two whole observations (kind 1; the marginal maps of kind 3
    add log 1 = 0 per observation without depths: all entries are exactly 0 and the smallest ids, again 2 and 3, lead by the map's
    order).  They then vote for instance 5."""
    c = Case("overflow_label", 8, IDENTITY, next_id=30)
    pts = np.array([[(i + 0.5) / 16.0, 0.03125, 1.0] for i in (-3, 1, 4)])
    for k in range(3):
        c.integrate(pts, 3, 2)
    for k in range(12):
        m = np.array([True, True, k < 6])  # voxel 2: 1 + 6 = 7 pairs, voxels 0, 1: 13
        c.integrate(pts[m], 4 + k % 5, 10 + k)
    cls_img, inst_img = images(3, 5)
    c.assoc(cls_img, inst_img)
    c.assoc(cls_img, inst_img)
    return c


def segment_ops_case(bs=8):
    """label_case plus a second layer (depth 1.5, outside every image operation's interest) of voxels with planted counts and
    confidences: rows of three voxels fed the observation sequences below ((object, class) per point)."""
    c = label_case(bs)
    seqs = [[(11, 2)], [(11, 2)] * 2, [(11, 2)] * 3, [(11, 2)] * 4, [(11, 2), (12, 2)], [(11, 2)] * 3 + [(12, 2)], [(13, 4)] * 4,
            [(13, 4), (13, 4), (13, 5)], [(7, 1)] * 2, [(14, 6)] * 3, [(14, 6)] * 2 + [(15, 6)] * 2]
    for r, seq in enumerate(seqs):
        pts = np.array([[(k - 1 + 0.5) / 16.0, (r - 5 + 0.5) / 16.0, 1.5] for k in range(3)])
        for obj, cls in seq:
            c.integrate(pts, cls, obj)
    c.seqs = seqs
    return c
