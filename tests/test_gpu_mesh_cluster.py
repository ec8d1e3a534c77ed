"""GPU: ScalableTSDFVolume.extract_simplified_mesh (hv_tsdf_extract_mesh_clustered, hv_extract.hip) on planted voxel states
(tests/mesh_cluster_cases.py) and on a fused map, held to the numpy restatement (tests/mesh_cluster_reference.py) run on the volume's
OWN extract_triangle_mesh().

Bar: vertices, colours, triangles and the vertex map EQUAL to the restatement bit for bit - the contract fixes the order of every
sum, and the members are the full mesh's own float64 values.  Voxel 0.02, sdf_trunc 0.08."""
import ctypes
import functools

import numpy as np
import pytest

from tests import mesh_cluster_cases as mc
from tests import mesh_cluster_reference as ref
from tests import planted_states as ps
from tests.conftest import canonical_mesh
from tests.test_gpu_tsdf_deintegrate import assert_bitwise
from tests.test_gpu_tsdf_edges import intrinsic, tiny_frames, volume

pytestmark = pytest.mark.gpu

HV_ERR_INVALID, HV_ERR_MODE = -1, -4
SURFACES = ("smooth", "rough", "two-faced", "no triangles", "lone sphere")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def parts(m, with_map=True):
    return (m.vertices, m.vertex_colors, m.triangles) + ((m.vertex_cluster,) if with_map else ())


def assert_same_mesh(got, want, what=""):
    for a, b, name in zip(got, want, ("vertices", "colours", "triangles", "vertex_cluster")):
        assert same(np.asarray(a), np.asarray(b)), f"{what} {name}: {np.asarray(a).shape} {np.asarray(a).dtype} / {np.asarray(b).shape} {np.asarray(b).dtype}"


def restate(vol, cell):
    """The restatement on the volume's own full mesh, owners read from the positions (planted cases: none ambiguous)."""
    full = vol.extract_triangle_mesh()
    g, bad = ref.owners_from_positions(full.vertices, ps.VOX)
    assert bad == 0
    return ref.cluster(full.vertices, full.vertex_colors, full.triangles, g, cell)


@functools.lru_cache(maxsize=None)
def planted(name):
    """The case planted into a volume of its own.  Shared by the tests that only read."""
    states = mc.states(name)
    vol = ps.plant(volume(ps.VOX, ps.TRUNC), states)
    assert_bitwise(vol.dump(), ps.as_dump(states))
    return vol


@functools.lru_cache(maxsize=None)
def expected(name, cell):
    return restate(planted(name), cell)


@pytest.mark.parametrize("cell", mc.CELLS)
@pytest.mark.parametrize("name", SURFACES)
def test_bit_for_bit_parity(name, cell):
    vol = planted(name)
    want = expected(name, cell)
    m = vol.extract_simplified_mesh(cell=cell, vertex_map=True)
    print(name, cell, "full", len(m.vertex_cluster), "->", len(m.vertices), "vertices", len(m.triangles), "triangles")
    assert_same_mesh(parts(m), want, f"{name} cell {cell}")
    assert len(m.vertices) > 0 and (name == "no triangles" or len(m.vertices) < len(m.vertex_cluster))
    # without the map the mesh is the same and carries no map; float32 is the float64 result rounded once
    plain = vol.extract_simplified_mesh(cell=cell)
    assert not hasattr(plain, "vertex_cluster")
    assert_same_mesh(parts(plain, False), want[:3])
    m32 = vol.extract_simplified_mesh(cell=cell, dtype=np.float32, vertex_map=True)
    assert_same_mesh(parts(m32), (want[0].astype(np.float32), want[1].astype(np.float32), want[2], want[3]), "float32")
    # called again: bitwise equal
    assert_same_mesh(parts(vol.extract_simplified_mesh(cell=cell, vertex_map=True)), parts(m), "repeat")


def test_the_planted_cases_reach_the_hard_parts():
    """What the parity test is worth: the volume's own meshes hold duplicate and reversed triples, clusters in units with negative
    keys, units with a vertex and no triangle."""
    full = planted("rough").extract_triangle_mesh()
    for cell in (2, 4, 8):
        kept, distinct, most, _ = mc.duplicates_and_reversed(expected("rough", cell)[3], full.triangles)
        assert kept > distinct and most >= 2
    assert mc.duplicates_and_reversed(expected("rough", 4)[3], full.triangles)[3] > 0
    assert mc.duplicates_and_reversed(expected("two-faced", 4)[3], planted("two-faced").extract_triangle_mesh().triangles)[3] > 0
    g, _ = ref.owners_from_positions(planted("smooth").extract_triangle_mesh().vertices, ps.VOX)
    assert ((g // 16) < 0).any()
    corner = planted("no triangles").extract_triangle_mesh()
    assert len(corner.vertices) == 3 and len(corner.triangles) == 1


def test_no_surface_and_the_empty_map():
    for vol in (planted("no surface"), volume(ps.VOX, ps.TRUNC)):
        for cell in mc.CELLS:
            for dt in (np.float64, np.float32):
                m = vol.extract_simplified_mesh(cell=cell, dtype=dt, vertex_map=True)
                assert m.vertices.shape == m.vertex_colors.shape == m.triangles.shape == (0, 3) and m.vertex_cluster.shape == (0,)
                assert m.vertices.dtype == dt and m.triangles.dtype == np.int32 and m.vertex_cluster.dtype == np.int32


@pytest.mark.parametrize("warm", ["cold", "float64", "float32"])
def test_warm_and_cold_full_mesh_cache(warm):
    """The simplified mesh does not care whether, or in which type, the full mesh is cached; and it leaves that cache, and the point
    cloud's, alone."""
    from pyslam_amd import _lib as L

    vol = ps.plant(volume(ps.VOX, ps.TRUNC), mc.states("rough"))
    before = vol.extract_triangle_mesh(dtype=np.dtype(warm)) if warm != "cold" else None
    m = vol.extract_simplified_mesh(cell=4, vertex_map=True)
    if before is not None:  # the fetch of the cached full mesh, in its type, right after the simplified one
        fn = vol._lib.hv_tsdf_extract_mesh if warm == "float64" else vol._lib.hv_tsdf_extract_mesh_f32
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        v, c, t = np.zeros_like(before.vertices), np.zeros_like(before.vertex_colors), np.zeros_like(before.triangles)
        L.check(fn(vol._h, L.ptr(v), L.ptr(c), len(v), L.ptr(t), len(t), ctypes.byref(nv), ctypes.byref(nt)))
        assert_same_mesh((v, c, t), parts(before, False), "cached full mesh")
    after = vol.extract_triangle_mesh()
    if before is not None:
        dt = before.vertices.dtype
        assert_same_mesh((after.vertices.astype(dt), after.vertex_colors.astype(dt), after.triangles), parts(before, False), "full mesh after")
    g, bad = ref.owners_from_positions(after.vertices, ps.VOX)
    assert bad == 0
    assert_same_mesh(parts(m), ref.cluster(after.vertices, after.vertex_colors, after.triangles, g, 4), warm)
    pc = vol.extract_point_cloud()
    vol.extract_simplified_mesh(cell=2)
    pc1 = vol.extract_point_cloud()
    assert len(pc.points) > 0 and same(pc1.points, pc.points) and same(pc1.colors, pc.colors)


def test_reads_only():
    vol = ps.plant(volume(ps.VOX, ps.TRUNC), mc.states("smooth"))
    dump, dirty, touched, n = vol.dump(), vol.dirty_keys(), vol.touched_keys(), vol.num_blocks()
    for cell in mc.CELLS:
        vol.extract_simplified_mesh(cell=cell, vertex_map=True)
    assert_bitwise(vol.dump(), dump)
    assert np.array_equal(vol.dirty_keys(), dirty) and np.array_equal(vol.touched_keys(), touched) and vol.num_blocks() == n


def _plant_in_order(states, order):
    keys, tsdf, weight, colour = states
    vol = volume(ps.VOX, ps.TRUNC)
    for i in order:  # one unit per call: the pool takes them in this order
        ps.plant(vol, (keys[i:i + 1], tsdf[i:i + 1], weight[i:i + 1], colour[i:i + 1]))
    return vol


def test_plant_order():
    """The pool order reaches the result only through the full mesh's unit order: each volume matches the restatement on its own
    full mesh, and the two results are the same mesh."""
    states = mc.states("rough")
    n = len(states[0])
    meshes = []
    for order in (range(n), np.random.default_rng(11).permutation(n)):
        vol = _plant_in_order(states, [int(i) for i in order])
        m = vol.extract_simplified_mesh(cell=4, vertex_map=True)
        assert_same_mesh(parts(m), restate(vol, 4), "own full mesh")
        meshes.append(m)
    assert not same(meshes[0].vertices, meshes[1].vertices)  # the orders do differ
    a, b = (canonical_mesh(m.vertices, m.triangles, m.vertex_colors) for m in meshes)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_staleness():
    vol = ps.plant(volume(ps.VOX, ps.TRUNC), mc.states("smooth"))
    first = vol.extract_simplified_mesh(cell=4, vertex_map=True)
    assert_same_mesh(parts(first), restate(vol, 4))
    ps.plant(vol, mc.states("rough"))  # the same units, other values
    second = vol.extract_simplified_mesh(cell=4, vertex_map=True)
    assert_same_mesh(parts(second), restate(vol, 4), "after the change")
    assert len(second.vertices) != len(first.vertices)


def test_device_outputs():
    torch = pytest.importorskip("torch")
    vol = planted("rough")
    for dt in (np.float64, np.float32):
        host = vol.extract_simplified_mesh(cell=2, dtype=dt, vertex_map=True)
        dev = vol.extract_simplified_mesh(cell=2, dtype=dt, vertex_map=True, device=True)
        for a, b in zip(parts(dev), parts(host)):
            assert isinstance(a, torch.Tensor) and a.is_cuda and a.device.index == vol._device().index
            assert same(a.cpu().numpy(), b)
    assert not hasattr(vol.extract_simplified_mesh(cell=2, device=True), "vertex_cluster")


@pytest.mark.parametrize("vertex_map", [False, True])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_device_outputs_of_vertices_without_triangles(dt, vertex_map):
    """A zero-row torch tensor has no address: the library must not take the fill of such a result for a size query."""
    torch = pytest.importorskip("torch")
    vol = planted("lone sphere")
    host = vol.extract_simplified_mesh(cell=16, dtype=dt, vertex_map=True)
    assert host.vertices.shape == (1, 3) and host.triangles.shape == (0, 3) and len(host.vertex_cluster) > 300
    assert_same_mesh(parts(host), expected("lone sphere", 16) if dt == np.float64 else
                     tuple(a.astype(np.float32) if a.dtype == np.float64 else a for a in expected("lone sphere", 16)))
    dev = vol.extract_simplified_mesh(cell=16, dtype=dt, vertex_map=vertex_map, device=True)
    assert hasattr(dev, "vertex_cluster") == vertex_map
    for a, b in zip(parts(dev, vertex_map), parts(host, vertex_map)):
        assert isinstance(a, torch.Tensor) and a.is_cuda and same(a.cpu().numpy(), b)


@functools.lru_cache(maxsize=None)
def fused():
    s, frames = tiny_frames(0, 8)
    vol = volume(ps.VOX, ps.TRUNC)
    from pyslam_amd.volumetric import RGBDImage

    for d, c, T in frames:
        vol.integrate(RGBDImage(c, d, 1.0, 4.0), intrinsic(s), T)
    return vol


@pytest.mark.parametrize("cell", mc.CELLS)
def test_fused_map(cell):
    """Real content (an exact-zero tsdf may occur, so owners are not read from positions): the volume's own map is a valid
    assignment, and the mesh is what the restatement makes of it."""
    vol = fused()
    full = vol.extract_triangle_mesh()
    m = vol.extract_simplified_mesh(cell=cell, vertex_map=True)
    vc = m.vertex_cluster
    assert len(full.vertices) > 5000 and vc.shape == (len(full.vertices),) and vc.dtype == np.int32
    n = len(m.vertices)
    assert np.array_equal(np.unique(vc), np.arange(n)) and 0 < n < len(full.vertices)
    # the members of every cluster lie inside ONE closed cell box, widened by 1e-9 m
    size = cell * ps.VOX
    u = full.vertices - 0.5 * ps.VOX
    lo, hi = np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
    np.minimum.at(lo, vc, u)
    np.maximum.at(hi, vc, u)
    box = np.floor((lo + 1e-9) / size)  # the cell of the lowest member (a member on the low face counts as inside)
    assert (lo >= box * size - 1e-9).all() and (hi <= (box + 1) * size + 1e-9).all()
    assert_same_mesh(parts(m, False), ref.from_map(full.vertices, full.vertex_colors, full.triangles, vc), f"cell {cell}")
    m32 = vol.extract_simplified_mesh(cell=cell, dtype=np.float32)
    assert same(m32.vertices, m.vertices.astype(np.float32)) and same(m32.vertex_colors, m.vertex_colors.astype(np.float32))
    assert same(m32.triangles, m.triangles)


def _abi(vol, cell, f32=False, caps=None, with_map=True):
    """Count then fill through the binding's _lib.  caps = (vertices, triangles, full vertices) of the fill call; buffers start as
    0xAB bytes.  -> (rc, (nv, nt, nf), arrays)."""
    from pyslam_amd import _lib as L

    fn = vol._lib.hv_tsdf_extract_mesh_clustered_f32 if f32 else vol._lib.hv_tsdf_extract_mesh_clustered
    nv, nt, nf = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = fn(vol._h, cell, None, None, 0, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt), ctypes.byref(nf))
    if rc != 0:
        return rc, (nv.value, nt.value, nf.value), None
    dt = np.float32 if f32 else np.float64
    fill = lambda shape, t: np.full(int(np.prod(shape)) * np.dtype(t).itemsize, 0xAB, np.uint8).view(t).reshape(shape)
    v, c, t, m = fill((nv.value, 3), dt), fill((nv.value, 3), dt), fill((nt.value, 3), np.int32), fill((nf.value,), np.int32)
    cv, ct, cf = caps if caps is not None else (nv.value, nt.value, nf.value)
    rc = fn(vol._h, cell, L.ptr(v), L.ptr(c), cv, L.ptr(t), ct, L.ptr(m) if with_map else None, cf, ctypes.byref(nv), ctypes.byref(nt),
            ctypes.byref(nf))
    return rc, (nv.value, nt.value, nf.value), (v, c, t, m)


def test_c_level_errors_and_caps():
    from pyslam_amd.volumetric import VoxelBlockGrid

    vol = planted("smooth")
    want = expected("smooth", 4)
    for cell in (0, 1, 3, 5, 32, -4):
        rc, counts, _ = _abi(vol, cell)
        assert rc == HV_ERR_INVALID and counts == (-1, -1, -1), cell
    fn = vol._lib.hv_tsdf_extract_mesh_clustered
    n = ctypes.c_int64()
    assert fn(vol._h, 4, None, None, 0, None, 0, None, 0, None, ctypes.byref(n), ctypes.byref(n)) == HV_ERR_INVALID
    assert fn(vol._h, 4, None, None, 0, None, 0, None, 0, ctypes.byref(n), ctypes.byref(n), None) == HV_ERR_INVALID
    grid = VoxelBlockGrid(0.05, 8)
    assert _abi(grid, 4)[0] == HV_ERR_MODE
    # the full result, then caps below every count: the counts stay, the rows beyond the caps are not written
    rc, counts, arrays = _abi(vol, 4)
    assert rc == 0 and counts == (len(want[0]), len(want[2]), len(want[3]))
    assert_same_mesh(arrays, want)
    rc, counts, (v, c, t, m) = _abi(vol, 4, caps=(10, 7, 100))
    assert rc == 0 and counts == (len(want[0]), len(want[2]), len(want[3]))
    assert same(v[:10], want[0][:10]) and same(c[:10], want[1][:10]) and same(t[:7], want[2][:7]) and same(m[:100], want[3][:100])
    assert (bits(v[10:]) == 0xAB).all() and (bits(c[10:]) == 0xAB).all() and (bits(t[7:]) == 0xAB).all() and (bits(m[100:]) == 0xAB).all()
    rc, _, (v, c, t, m) = _abi(vol, 4, f32=True, with_map=False)
    assert rc == 0 and same(v, want[0].astype(np.float32)) and same(t, want[2]) and (bits(m) == 0xAB).all()
