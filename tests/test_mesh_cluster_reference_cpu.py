"""The numpy restatement of the vertex-clustered mesh (tests/mesh_cluster_reference.py) and the planted cases it is run on
(tests/mesh_cluster_cases.py), checked on oracle.PortTsdf meshes and on a mesh typed out by hand - no GPU."""
import functools

import numpy as np
import pytest

from tests import mesh_cluster_cases as mc
from tests import mesh_cluster_reference as ref
from tests import planted_states as ps

SURFACES = ("smooth", "rough", "two-faced")


@functools.lru_cache(maxsize=None)
def full_mesh(name):
    """(vertices, colours, triangles, owners, ambiguous) of the case on the CPU oracle; shared, never written to."""
    v, t, c = ps.to_oracle(mc.states(name)).extract_triangle_mesh()
    g, bad = ref.owners_from_positions(v, ps.VOX)
    return v, c, t, g, bad


@pytest.mark.parametrize("name", SURFACES + ("no triangles",))
def test_every_vertex_names_its_owner(name):
    v, _, t, g, bad = full_mesh(name)
    assert len(v) > 0 and len(t) > 0 and bad == 0
    # the vertex lies on the edge from its owner's centre towards +axis
    u = v / ps.VOX - 0.5 - g
    assert (u > -1e-6).all() and (u < 1.0).all() and ((u > 1e-3).sum(axis=1) == 1).all()


def test_the_cases_hold_what_they_are_for():
    _, _, t, g, _ = full_mesh("rough")
    reversed_pairs = 0
    for cell in (2, 4, 8):
        kept, distinct, most, rev = mc.duplicates_and_reversed(ref.assignment(g, cell), t)
        assert kept > distinct and most >= 2, cell  # duplicate triples
        reversed_pairs += rev
    assert reversed_pairs > 0
    _, _, t, g, _ = full_mesh("two-faced")
    assert all(mc.duplicates_and_reversed(ref.assignment(g, cell), t)[3] > 0 for cell in (4, 8))
    _, _, _, g, _ = full_mesh("smooth")
    assert ((g // 16) < 0).any(axis=1).sum() > 100  # clusters in units with negative keys
    assert len({tuple(k) for k in (g // 16).tolist()}) == 7  # two of the nine planted units own no vertex
    # (d): three units with one vertex each, the triangle between them; (e): nothing
    v, _, t, g, _ = full_mesh("no triangles")
    assert len(v) == 3 and len(t) == 1 and len({tuple(k) for k in (g // 16).tolist()}) == 3
    assert len(full_mesh("no surface")[0]) == 0


def test_cluster_on_a_mesh_typed_out_by_hand():
    """Voxel length 1, cell 2.  Twelve vertices in two units, the first with a negative key: vertex = owner centre + an offset along
    one axis.  Clusters, numbered by (unit by first appearance, cell):
      unit (-1, 0, 0), listed first: cells (-8,0,0) <- v0, v1 (owners (-16,0,0), (-15,1,1));  (-8,0,1) <- v2;  (-1,7,7) <- v3, v4
      unit (0, 0, 0):                cells (0,0,0) <- v5, v6, v7;  (0,0,1) <- v8 (no triangle refers to it);  (1,0,0) <- v9;
                                           (7,7,7) <- v10, v11
    """
    g = np.array([(-16, 0, 0), (-15, 1, 1), (-16, 1, 2), (-1, 15, 15), (-2, 14, 14),
                  (0, 0, 0), (1, 1, 0), (0, 1, 1), (1, 0, 2), (2, 0, 0), (15, 15, 15), (14, 14, 15)], np.int64)
    axis = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2])
    frac = np.array([0.25, 0.5, 0.75, 0.125, 0.5, 0.25, 0.5, 0.75, 0.5, 0.25, 0.5, 0.125])
    v = g + 0.5
    v[np.arange(12), axis] += frac
    c = np.arange(36, dtype=np.float64).reshape(12, 3) / 64.0
    t = np.array([(0, 2, 3),      # clusters (0, 1, 2)
                  (1, 2, 4),      # (0, 1, 2) again: a duplicate
                  (4, 2, 1),      # (2, 1, 0) -> rotated (0, 2, 1): the reversed twin
                  (0, 1, 2),      # (0, 0, 1): degenerate
                  (5, 9, 10),     # (3, 5, 6)
                  (11, 6, 9),     # (6, 3, 5) -> rotated (3, 5, 6): a duplicate after rotation
                  (9, 3, 7)],     # (5, 2, 3) -> rotated (2, 3, 5): across the two units
                 np.int32)
    got_g, bad = ref.owners_from_positions(v, 1.0)
    assert bad == 0 and (got_g == g).all()
    verts, cols, tris, vc = ref.cluster(v, c, t, g, 2)
    assert vc.tolist() == [0, 0, 1, 2, 2, 3, 3, 3, 4, 5, 6, 6] and vc.dtype == np.int32
    want = np.stack([(v[0] + v[1]) / 2.0, v[2], (v[3] + v[4]) / 2.0, ((v[5] + v[6]) + v[7]) / 3.0, v[8], v[9], (v[10] + v[11]) / 2.0])
    assert (verts == want).all()
    assert (cols == np.stack([(c[0] + c[1]) / 2.0, c[2], (c[3] + c[4]) / 2.0, ((c[5] + c[6]) + c[7]) / 3.0, c[8], c[9], (c[10] + c[11]) / 2.0])).all()
    assert tris.tolist() == [[0, 1, 2], [0, 2, 1], [2, 3, 5], [3, 5, 6]] and tris.dtype == np.int32
    assert 4 not in tris  # the unreferenced cluster stays a vertex
    # at cell 16 every unit is one cluster; only the triangle across the units could survive, and it has two vertices in unit 1
    verts16, _, tris16, vc16 = ref.cluster(v, c, t, g, 16)
    assert vc16.tolist() == [0] * 5 + [1] * 7 and len(tris16) == 0 and verts16.shape == (2, 3)
    # a position off the grid, or on a voxel centre, is reported
    off = v.copy()
    off[3, 1] += 0.01
    off[7] = g[7] + 0.5
    assert ref.owners_from_positions(off, 1.0)[1] == 2


@pytest.mark.parametrize("cell", mc.CELLS)
@pytest.mark.parametrize("name", SURFACES)
def test_properties_of_the_restatement(name, cell):
    v, c, t, g, _ = full_mesh(name)
    verts, cols, tris, vc = ref.cluster(v, c, t, g, cell)
    n = len(verts)
    assert verts.shape == cols.shape == (n, 3) and vc.shape == (len(v),) and set(vc.tolist()) == set(range(n))
    # every simplified vertex lies inside the closed box of its cell: [k c + 0.5, k c + k + 0.5] voxels per axis
    cells = np.zeros((n, 3), np.int64)
    cells[vc] = g // cell
    lo = (cell * cells + 0.5) * ps.VOX
    assert (verts >= lo - 1e-12).all() and (verts <= lo + cell * ps.VOX + 1e-12).all()
    assert (cols >= 0.0).all() and (cols <= 1.0).all()
    # triangles: distinct, sorted, smallest number first, no two numbers equal
    assert (tris[:, 0] < tris[:, 1]).all() and (tris[:, 0] < tris[:, 2]).all() and (tris[:, 1] != tris[:, 2]).all()
    keys = [tuple(r) for r in tris.tolist()]
    assert keys == sorted(set(keys))
    # clusters are numbered unit by unit in the order of the full mesh, ascending by cell inside a unit
    rows = np.zeros((n, 4), np.int64)
    _, first = np.unique(g // 16, axis=0, return_index=True)
    unit_rank = {tuple((g[i] // 16).tolist()): r for r, i in enumerate(sorted(first.tolist()))}
    rows[vc] = np.concatenate([np.array([[unit_rank[tuple(k)]] for k in (g // 16).tolist()]), g // cell], axis=1)
    assert [tuple(r) for r in rows.tolist()] == sorted({tuple(r) for r in rows.tolist()})
    # from_map on the assignment reproduces cluster
    again = ref.from_map(v, c, t, vc)
    assert all((a == b).all() and a.dtype == b.dtype for a, b in zip(again, (verts, cols, tris)))
    # the order of the full triangles does not matter
    perm = np.random.default_rng(7).permutation(len(t))
    shuffled = ref.cluster(v, c, t[perm], g, cell)
    assert all((a == b).all() for a, b in zip(shuffled, (verts, cols, tris, vc)))


def test_empty_meshes():
    e3, ei = np.zeros((0, 3)), np.zeros((0, 3), np.int32)
    verts, cols, tris, vc = ref.cluster(e3, e3, ei, np.zeros((0, 3), np.int64), 4)
    assert verts.shape == cols.shape == tris.shape == (0, 3) and vc.shape == (0,) and tris.dtype == np.int32
    # vertices without triangles
    verts, _, tris, vc = ref.cluster(np.array([[0.75, 0.5, 0.5]]), np.zeros((1, 3)), ei, np.array([[0, 0, 0]]), 2)
    assert verts.tolist() == [[0.75, 0.5, 0.5]] and tris.shape == (0, 3) and vc.tolist() == [0]
