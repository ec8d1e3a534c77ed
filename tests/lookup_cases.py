"""TEST INFRASTRUCTURE ONLY - planted grids for the point lookup (hv_lookup_points): the smallest states at which it can go wrong.

Every state is planted through `integrate` of a few exactly representable points: voxel size 0.25, coordinates that are multiples of
1/16 (so sums, mean positions and squared distances are exact in float32 and float64), and one `carve` through a pinhole camera at
the origin whose only valid depth pixel sees one voxel.  A case runs on any grid with the common interface (the GPU grids, the
oracle's PortGrid / PortSemGrid2) through run_case(); the expected answers come from tests/lookup_reference.py applied to the
grid's own dump.

A voxel is named by its integer coordinate v; a point `at(v, o)` sits o sixteenths of a metre into it (o in 0..3 per axis).
"""
import numpy as np

VOXEL = 0.25
BLOCK_SIZES = (8, 5)  # the default, and one that is no power of two (floor division instead of a shift)
W, H = 64, 48
INTR = (32.0, 32.0, 32.0, 24.0)
DEPTH_MAX, DEPTH_MIN = 8.0, 0.25
POINT_COUNTS = (0, 1, 63, 64, 65, 129)
KEY_LIMIT = 1 << 20


def at(v, o=(1, 1, 1)):
    return [v[k] * VOXEL + o[k] / 16.0 for k in range(3)]


class Case:
    def __init__(self, name, bs):
        self.name, self.bs = name, int(bs)
        self.steps = []    # ("integrate", points f64 [n,3], colours f32 [n,3], class ids, object ids) | ("carve", depth f32 [H,W], threshold)
        self.queries = []  # points [3]
        self.params = [(1, 0.0)]  # (min_count, min_confidence) pairs to look up with
        self.conf_voxel = None    # semantic grids: also look up with min_confidence = this voxel's confidence, and one ulp above it

    def plant(self, v, o=(1, 1, 1), n=1, cls=1, obj=1):
        """n points at at(v, o); cls / obj: one label for all, or one per point."""
        pts = np.array([at(v, o)] * n, np.float64)
        col = np.stack([np.full(n, 0.25), np.full(n, 0.5), (np.arange(n) % 4) * 0.25], 1).astype(np.float32)
        self.steps.append(("integrate", pts, col, np.broadcast_to(np.asarray(cls, np.int32), (n,)).copy(),
                           np.broadcast_to(np.asarray(obj, np.int32), (n,)).copy()))
        return self

    def carve(self, pixel_depth, threshold=0.25):
        depth = np.zeros((H, W), np.float32)  # 0: not a valid depth, such a pixel carves nothing
        depth[24, 32] = pixel_depth
        self.steps.append(("carve", depth, float(threshold)))
        return self

    def ask(self, *points):
        self.queries += [list(p) for p in points]
        return self

    def points(self, dtype):
        return np.ascontiguousarray(np.array(self.queries, np.float64).reshape(-1, 3).astype(dtype))

    def n_blocks(self):
        keys = {tuple(np.floor(np.floor(p / VOXEL) / self.bs).astype(np.int64)) for s in self.steps if s[0] == "integrate" for p in s[1]}
        return len(keys)


def cases(bs):
    e = bs - 1  # the last voxel of block 0 along an axis
    out = []

    # a query in the corner voxel of block 0: its 3^3 neighbourhood spans 8 blocks, of which three exist ((0,0,0), (1,1,1), (1,0,0));
    # the own voxel is empty.  The 5^3 neighbourhood adds a nearer voxel two steps away in block 0.
    c = Case("corner8", bs)
    c.plant((bs, bs, bs), (0, 0, 0), cls=1, obj=11).plant((e - 1, e, e), (0, 2, 2), n=2, cls=2, obj=12).plant((bs, e, e), (3, 2, 2), cls=3, obj=13)
    c.plant((e, e, e - 2), (2, 2, 3), cls=4, obj=14)
    c.ask(at((e, e, e), (2, 2, 2)), at((e, e, e), (3, 3, 3)), at((e, e, e), (0, 0, 0)), at((bs, bs, bs), (2, 1, 0)), at((e + 3, e, e)))
    out.append(c)

    # negative coordinates next to 0: floor, not truncation; -0.0 and 0.0 are voxel 0
    c = Case("negative", bs)
    c.plant((-1, -1, -1), cls=1, obj=1).plant((0, 0, 0), cls=2, obj=2).plant((-1, 0, 0), (3, 1, 1), cls=3, obj=3)
    c.ask([-1 / 16, -1 / 16, -1 / 16], [-1 / 16, 1 / 16, 1 / 16], [0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [1 / 16, -1 / 16, 1 / 16], [-0.25, -0.25, -0.25],
          [-0.5, 1 / 16, 1 / 16])
    # points that have no voxel
    c.ask([np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [1.0e12, 0.0, 0.0], [0.0, -1.0e12, 0.0])
    out.append(c)

    # a query exactly on a voxel face belongs to the voxel above it
    c = Case("face", bs)
    c.plant((2, 0, 0), cls=1, obj=1).plant((1, 0, 0), cls=2, obj=2)
    c.ask([0.5, 1 / 16, 1 / 16], [0.25, 1 / 16, 1 / 16], [0.75, 1 / 16, 1 / 16], [0.5, 0.25, 0.25])
    # (the one query that is no multiple of 1/16: a float64 ulp under the face is voxel 1 in float64 and, rounded to float32, voxel 2)
    c.ask([np.nextafter(0.5, 0.0), 1 / 16, 1 / 16])
    out.append(c)

    # the last voxel before the key range ends at block 2^20 (its lower face is exact in float32 as well), and the first one at -2^20
    top, bot = KEY_LIMIT * bs - 1, -KEY_LIMIT * bs
    c = Case("key_edge", bs)
    c.plant((top, 0, 0), (0, 1, 1), cls=1, obj=1).plant((bot, 0, 0), (0, 1, 1), cls=2, obj=2)
    c.ask(at((top, 0, 0), (0, 1, 1)), at((top - 1, 0, 0), (0, 1, 1)), at((top - 2, 0, 0), (0, 1, 1)), at((top + 1, 0, 0), (0, 1, 1)),
          at((bot, 0, 0), (0, 1, 1)), at((bot + 1, 0, 0), (0, 1, 1)), at((bot + 2, 0, 0), (0, 1, 1)), at((bot - 1, 0, 0), (0, 1, 1)))
    out.append(c)

    # two qualifying neighbours exactly equidistant: the smaller offset index wins
    c = Case("tie", bs)
    c.plant((1, 2, 2), (2, 1, 1), cls=1, obj=1).plant((3, 2, 2), (2, 1, 1), cls=2, obj=2)
    c.plant((2, 1, 2), (2, 0, 1), cls=3, obj=3).plant((2, 3, 2), (2, 2, 1), cls=4, obj=4)  # (farther: 5/16; equidistant among themselves)
    c.ask(at((2, 2, 2), (2, 1, 1)))
    out.append(c)

    # the own voxel qualifies while a neighbour's mean is nearer: the own voxel is the answer
    c = Case("own_wins", bs)
    c.plant((2, 2, 2), (1, 1, 1), cls=1, obj=1).plant((3, 2, 2), (0, 1, 1), cls=2, obj=2)
    c.ask(at((2, 2, 2), (3, 1, 1)))
    out.append(c)

    # the own voxel is present but under min_count, a neighbour holds exactly min_count points
    c = Case("under_min_count", bs)
    c.plant((2, 2, 2), n=1, cls=1, obj=1).plant((2, 3, 2), n=2, cls=2, obj=2).plant((2, 2, 3), (1, 1, 3), n=3, cls=3, obj=3)
    c.ask(at((2, 2, 2)), at((2, 3, 2)))
    c.params = [(1, 0.0), (2, 0.0), (3, 0.0), (4, 0.0), (0, 0.0), (-5, 0.0)]
    out.append(c)

    # a confidence exactly at min_confidence, and one ulp under it (two of three observations agree); the neighbour is sure of its label
    c = Case("conf_edge", bs)
    c.plant((2, 2, 2), n=3, cls=[1, 1, 2], obj=[1, 1, 2]).plant((3, 2, 2), n=2, cls=5, obj=5)
    c.ask(at((2, 2, 2)), at((3, 2, 2)))
    c.conf_voxel = (2, 2, 2)
    c.params = [(1, 0.0), (1, -1.0), (1, 1.0), (1, 2.0), (1, float("nan"))]
    out.append(c)

    # a voxel reset inside a live block: the camera at the origin looks along +z, its one valid pixel sees voxel (0, 0, 8) in front of the
    # measured depth; its neighbours project to other pixels or lie behind the carving depth
    c = Case("reset", bs)
    c.plant((0, 0, 8), cls=1, obj=1).plant((1, 0, 8), cls=2, obj=2).plant((0, 0, 9), cls=3, obj=3)
    c.carve(2.5)
    c.plant((4, 4, 8), cls=4, obj=4)  # (a later integrate into the same grid)
    c.ask(at((0, 0, 8)), at((1, 0, 8)), at((0, 0, 9)), at((0, 1, 8)))
    out.append(c)

    # a probabilistic label map that runs past its six inline pairs into a chained node
    c = Case("chain", bs)
    c.plant((2, 2, 2), n=9, cls=list(range(1, 10)), obj=list(range(11, 20))).plant((2, 2, 2), n=2, cls=4, obj=14)
    c.plant((3, 2, 2), n=17, cls=[k % 17 for k in range(17)], obj=[100 + k for k in range(17)])
    c.ask(at((2, 2, 2)), at((3, 2, 2)), at((1, 2, 2)))
    out.append(c)

    out.append(Case("empty", bs).ask([1 / 16, 1 / 16, 1 / 16], [np.nan, 0.0, 0.0], at((top + 1, 0, 0))))
    return out


def counted_queries(case, n):
    """n query points of the case: its own, repeated, each repetition moved by another multiple of 1/16 inside +-2 voxels."""
    base = np.array(case.queries, np.float64).reshape(-1, 3)
    k = np.arange(n)
    shift = np.stack([(k // len(base)) % 9 - 4, (k // len(base) * 3) % 7 - 3, (k // len(base) * 5) % 5 - 2], 1) / 16.0 * 2.0
    return np.ascontiguousarray(base[k % len(base)] + shift) if n else np.zeros((0, 3), np.float64)


def run_case(grid, case, semantic, carve):
    """Drive `grid` through the case's steps.  carve(grid, depth, threshold) applies the carve step through the grid's own interface."""
    for step in case.steps:
        if step[0] == "integrate":
            if semantic:
                grid.integrate(step[1], step[2], step[3], step[4], None)
            else:
                grid.integrate(step[1], step[2])
        else:
            carve(grid, step[1], step[2])
