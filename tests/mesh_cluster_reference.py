"""The vertex-clustered mesh of include/hipvol.h (hv_tsdf_extract_mesh_clustered) restated in numpy on a full mesh - test
infrastructure, no GPU.

A full vertex lies on the edge from its OWNER voxel g to g + e_axis; its cluster is (unit of g, floor_div(g, cell)).  Units rank by
first appearance in the vertex list, clusters inside a unit by (cx, cy, cz); a simplified vertex is the members' float64 values added
one by one in index order, starting from the first member, over the count; a triangle maps to its clusters' numbers, is dropped when
two are equal, is rotated smallest first, and the distinct triples are sorted."""
import numpy as np

UNIT_VOXELS = 16


def owners_from_positions(vertices, voxel_length):
    """-> (g [V,3] int64, number of vertices that do not fit the rule).  In u = p / voxel_length - 0.5 exactly one coordinate has a
    fractional part in [1e-3, 1 - 1e-3] - the edge's axis: floored; the other two lie within 1e-6 of an integer: rounded."""
    u = np.asarray(vertices, np.float64).reshape(-1, 3) / voxel_length - 0.5
    frac = u - np.floor(u)
    along = (frac >= 1e-3) & (frac <= 1.0 - 1e-3)
    on_grid = np.abs(u - np.rint(u)) <= 1e-6
    fits = (along.sum(axis=1) == 1) & ((along | on_grid).all(axis=1))
    g = np.where(along, np.floor(u), np.rint(u)).astype(np.int64)
    return g, int((~fits).sum())


def _ordered_mean(values, member_of, n):
    """Per cluster: the members' rows added one by one in ascending index, starting from the first member, over the count."""
    values = np.asarray(values, np.float64)
    _, first = np.unique(member_of, return_index=True)
    total = values[first].copy()
    rest = np.ones(len(values), bool)
    rest[first] = False
    np.add.at(total, member_of[rest], values[rest])  # unbuffered: in index order
    return total / np.bincount(member_of, minlength=n).astype(np.float64)[:, None]


def from_map(vertices, colors, triangles, vertex_cluster):
    """The simplified mesh for a GIVEN assignment full vertex -> cluster number (every number 0 .. n - 1 occurs).
    -> (verts [n,3] f64, cols [n,3] f64, tris [m,3] int32)."""
    vc = np.asarray(vertex_cluster, np.int64).reshape(-1)
    if len(vc) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), np.int32)
    n = int(vc.max()) + 1
    assert len(np.unique(vc)) == n, "every cluster number must occur"
    verts, cols = _ordered_mean(vertices, vc, n), _ordered_mean(colors, vc, n)
    t = vc[np.asarray(triangles, np.int64).reshape(-1, 3)]
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    shift = np.argmin(t, axis=1) if len(t) else np.zeros(0, np.int64)
    t = np.stack([t[np.arange(len(t)), (shift + j) % 3] for j in range(3)], axis=1) if len(t) else t
    return verts, cols, np.unique(t, axis=0).astype(np.int32).reshape(-1, 3)


def assignment(g, cell):
    """-> vertex_cluster [V] int32 for owners g [V,3]: clusters numbered by (rank of the unit by first appearance, cx, cy, cz)."""
    g = np.asarray(g, np.int64).reshape(-1, 3)
    if len(g) == 0:
        return np.zeros(0, np.int32)
    assert cell in (2, 4, 8, 16)
    units, first, unit_of = np.unique(g // UNIT_VOXELS, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(units), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(units))
    rows = np.concatenate([rank[unit_of.reshape(-1)][:, None], g // cell], axis=1)  # (// floors towards -inf)
    _, vc = np.unique(rows, axis=0, return_inverse=True)  # rows sorted lexicographically
    return vc.reshape(-1).astype(np.int32)


def cluster(vertices, colors, triangles, g, cell):
    """-> (verts, cols, tris, vertex_cluster) of the contract, for the full mesh and its owners g."""
    vc = assignment(g, cell)
    return from_map(vertices, colors, triangles, vc) + (vc,)
