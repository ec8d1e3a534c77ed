"""GPU: one long-lived ScalableTSDFVolume through the scripts of tests/lifetime_cases.py - the state an hv_volume carries from one call
into the next (per-unit extraction caches and their stamps, cached extraction results, the batch pipeline, dirty units), which the
one-call-per-volume tests of the single operations never see.

After every step k of a script:
  1. the step alone: vol.dump() against that operation's restatement applied to the dump taken before the step - the GPU's own, so
     nothing accumulates - with that operation's checker from its own test module (assert_bitwise for de-integration, prune,
     component removal and repack; assert_matches_restatement for merges; assert_same_volume, the fuse bar of tests/test_gpu_tsdf.py,
     for fusion), and the returned stats equal to the restatement's;
  2. the readers the step's tick names, on the long-lived volume and on a TWIN - a fresh volume that unpacks vol.pack(): another
     pool order, a first-ever extraction, no stamps, no pipeline - bitwise equal; after the last step also ray_cast, sample_points,
     check_frame, distance_field, surface_components and pack(), and the mesh against the oracle loaded with vol.dump();
  3. every unit that differs from the dump taken at the last mark_merged is in dirty_keys(), which holds only units of the map.
No tolerance of this file's own.

Meshes and clouds of two volumes are compared as tables of rows sorted on their exact values (mesh_rows), not with
conftest.canonical_mesh: that orders vertices by positions rounded to 1e-9, and the order of coincident vertices then follows the pool
order, which is exactly what differs between the long-lived volume and its twin.

What the pipeline scripts hold is the pipeline's LOGICAL state (parity, touch counters, versions, which half of the touched lists a
batch uses), not a real overlap of a touch pass with the previous sweep: every step is bracketed by dump(), which drains the main
stream, and a tick that builds the twin calls pack(), which disarms the pipeline, so the batch behind such a tick starts a fresh chain.

The restatements run in Python and dominate the wall time.  The bar is the slowest case of tests/test_gpu_tsdf_merge.py: 1.7 s on the
MI355X for the first of them, which renders the shared frame stream (lru-cached for the process: a one-off cost charged to whichever
test asks first, 1-9 s), 0.5-1.0 s for the others.  Measured in the same run, wall seconds of a whole test on the MI355X / of the
script's restatements alone on the CPU (tests/test_lifetime_reference_cpu.py): chain_a 0.7 / 3.2, chain_b 0.5 / 1.0, chain_c 0.4 / 0.5,
chain_d 0.6 / 0.7, chain_e 0.6 / 1.1, chain_f 0.3 / 0.2, gather_a 0.2 / 0.1, gather_b 0.4 / 0.6, pool_grows 0.6 / 1.2, slots_move
0.5 / 1.0, each pipeline script 0.1-0.2 / 0.2-0.3 per sweep form, the two-volume test 0.2, the size-query test 0.3: every script is
below the bar and none is split for its time.

With one invalidation at a time taken out of the library on a scratch copy: without the extract_epoch bump of hv_rekey_in_place
slots_move fails at its first extraction after the prune (the floater's vertices are missing: its new pool slot still holds the masks
of the all-zero unit that was there); without the stamp write of the component-removal kernel every script with a removal fails
(dirty_keys() misses the changed units, the warm mesh keeps the removed pieces); without `mesh_cache_version = 0` in points_compute
test_size_query_then_anything_then_fetch fails at the points size query between a mesh size query and its fetch.  Without the
`pipe_armed = false` of hv_components.hip nothing fails, and nothing can: the labelling drains both streams, a removal that changes a
voxel bumps content_version, which ends the chain by itself, and after one that changes nothing the volume is what the last batch
left.
"""
import ctypes
import functools
import time

import numpy as np
import pytest

from tests import lifetime_cases as lc
from tests import pack_reference as PR
from tests import planted_states as ps
from tests.conftest import _lex_less
from tests.test_gpu_tsdf import assert_same_volume
from tests.test_gpu_tsdf_deintegrate import assert_bitwise
from tests.test_gpu_tsdf_edges import assert_meshes_match, cuda, intrinsic, stack
from tests.test_gpu_tsdf_merge import assert_consistent, assert_matches_restatement

pytestmark = pytest.mark.gpu

VOX, TRUNC = lc.VOX, lc.TRUNC


def fresh(max_blocks=lc.BIG_BLOCKS):
    from pyslam_amd.volumetric import ScalableTSDFVolume

    return ScalableTSDFVolume(VOX, TRUNC, max_blocks=max_blocks)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def key_set(keys):
    return {tuple(int(x) for x in k) for k in np.asarray(keys).reshape(-1, 3)}


def start_volume(script):
    """The script's start states planted part by part (the order of the planting calls is the pool order), nothing dirty."""
    vol = fresh(script.max_blocks)
    for part in script.start:
        ps.plant(vol, part())
    assert_bitwise(vol.dump(), lc.start_dump(script))
    vol.mark_merged()
    return vol


@functools.lru_cache(maxsize=None)
def merge_sources():
    """name -> (volume, its dump) of lifetime_cases' merge sources.  Shared: only read."""
    out = {}
    for name in lc.SOURCES:
        vol = ps.plant(fresh(), lc.source(name))
        assert_bitwise(vol.dump(), ps.as_dump(lc.source(name)))
        out[name] = (vol, vol.dump())
    return out


def twin_of(vol):
    twin = fresh()
    twin.unpack(vol.pack())
    return twin


# ---- one step on the volume --------------------------------------------------------------------------------------------------------
def run_step(vol, step, before=None):
    """-> the stats the call returned, as a tuple (None where the call returns none)."""
    from pyslam_amd.volumetric import RGBDImage

    op, arg = step.op, step.arg
    if op in ("fuse", "fuse_batch", "deintegrate_batch", "reintegrate_batch", "ray_cast"):
        s, frames = lc.frames_for(arg)
        K = intrinsic(s)
        d, c, T = stack(frames)
        if op == "fuse":
            for depth, colour, pose in frames:
                vol.integrate(RGBDImage(colour, depth, 1.0, 4.0), K, pose)
            return None
        if op == "fuse_batch":
            vol.integrate_batch(*cuda(d, c), K, T, depth_scale=1.0, depth_trunc=4.0)
            return None
        if op == "deintegrate_batch":
            return vol.deintegrate_batch(*cuda(d, c), K, T).as_tuple()
        if op == "reintegrate_batch":
            return vol.reintegrate_batch(*cuda(d, c), K, T, np.ascontiguousarray(T @ lc.MOVE)).as_tuple()
        vol.ray_cast(K, T[0], 0.1, 4.0)
        return None
    if op == "prune":
        empty, lo, hi = arg
        bounds = None if lo is None else ((np.asarray(lo, np.float64) + 0.5) * ps.UNIT, (np.asarray(hi, np.float64) + 0.5) * ps.UNIT)
        return vol.prune(empty=empty, bounds=bounds).as_tuple()
    if op == "merge":
        return vol.integrate_volume(merge_sources()[arg[0]][0], lc.TRANSFORMS[arg[1]]).as_tuple()
    if op == "remove_small":
        return tuple(vol.remove_small_components(arg[0], margin=arg[1]))
    if op == "repack":
        buf = vol.pack()
        assert buf.tobytes() == PR.pack_reference(*PR.state_of_volume(vol), voxel_length=VOX, sdf_trunc=TRUNC)
        vol.reset()
        assert vol.num_blocks() == 0
        st = vol.unpack(buf)
        return (st.units, st.voxels, st.bytes)
    if op == "mark_merged":
        vol.mark_merged()
    elif op == "read_mesh":
        assert len(vol.extract_triangle_mesh().triangles) > 0
    else:
        assert op == "sample_points", op
        vol.sample_points(lc.sample_positions(before if before is not None else vol.dump(), arg))
    return None


def check_step(vol, step, before, stats, label):
    """Check 1: the volume after the step against the step's restatement applied to `before`.  -> the dump after the step."""
    after = vol.dump()
    sources = {name: dump for name, (_, dump) in merge_sources().items()}
    if step.op == "merge":
        # (assert_matches_restatement runs merge_reference itself, with its fragile-voxel rule)
        _, ref_stats = assert_matches_restatement(after, before, sources[step.arg[0]], lc.TRANSFORMS[step.arg[1]], step.arg[1])
        assert stats == ref_stats, (label, stats, ref_stats)
    else:
        ref, ref_stats, extra = lc.reference_step(before, step, sources)
        if "oracle" in extra:
            assert_same_volume(vol, extra["oracle"], swept=step.op != "fuse")
        else:
            assert_bitwise(after, ref)
        if ref_stats is not None:
            assert stats == ref_stats, (label, stats, ref_stats)
    if step.nothing or step.op in ("mark_merged", "repack"):
        assert_bitwise(after, before)
    return after


# ---- readers -----------------------------------------------------------------------------------------------------------------------
def sorted_rows(*columns):
    """The rows of the columns side by side, sorted on every column: equal for two results that hold the same rows in any order."""
    n = len(columns[0])
    rows = np.concatenate([np.asarray(c, np.float64).reshape(n, int(np.prod(np.shape(c)[1:]))) for c in columns], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def mesh_rows(vertices, triangles, colours):
    """A mesh as two order-free tables: (vertex | colour) rows, and the triangles as rows of their three vertex POSITIONS, each
    rotated to its smallest rotation.  conftest.canonical_mesh orders vertices by positions rounded to 1e-9, which leaves the order of
    coincident vertices (a tsdf of exactly 0 on a voxel corner puts the vertices of several edges there, an ulp apart) to the pool
    order; the twin has another pool order, so the tables are sorted on the exact values."""
    v, t = np.asarray(vertices, np.float64), np.asarray(triangles)
    tri = np.zeros((0, 9))
    if len(t):
        p = v[t]
        rots = [np.concatenate([p[:, (r + k) % 3] for k in range(3)], axis=1) for r in range(3)]
        tri = rots[0]
        for r in rots[1:]:
            tri = np.where(_lex_less(r, tri)[:, None], r, tri)
        tri = tri[np.lexsort(tri.T[::-1])]
    return sorted_rows(v, colours), tri


def assert_same_rows(a, b, label):
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), label


def same(a, b, mesh=True, points=True, dtype=None):
    """tests/test_gpu_tsdf.py's `same` (test_incremental_extraction_equals_a_full_pass_at_every_tick) for two volumes whose pool
    orders differ: the same rows, bit for bit, in any order."""
    if mesh:
        ma, mb = a.extract_triangle_mesh(dtype=dtype), b.extract_triangle_mesh(dtype=dtype)
        assert ma.vertices.shape == mb.vertices.shape and ma.triangles.shape == mb.triangles.shape and len(ma.triangles) > 0
        assert_same_rows(mesh_rows(ma.vertices, ma.triangles, ma.vertex_colors), mesh_rows(mb.vertices, mb.triangles, mb.vertex_colors), "mesh")
    if points:
        pa, pb = a.extract_point_cloud(), b.extract_point_cloud()
        assert pa.points.shape == pb.points.shape and len(pa.points) > 0
        assert_same_rows([sorted_rows(pa.points, pa.colors)], [sorted_rows(pb.points, pb.colors)], "points")


def same_normals(a, b):
    pa, pb = a.extract_point_cloud(normals=True), b.extract_point_cloud(normals=True)
    assert pa.points.shape == pb.points.shape and len(pa.points) > 0 and pa.normals.shape == pa.points.shape
    assert_same_rows([sorted_rows(pa.points, pa.colors, pa.normals)], [sorted_rows(pb.points, pb.colors, pb.normals)], "points with normals")


def same_mesh32(a, b):
    """The float32 mesh is the float64 mesh rounded once (test_float32_extraction_is_the_float64_result_rounded_once), on the
    long-lived volume - float32 first, so that the cached result changes type - and equal to the twin's."""
    m32 = a.extract_triangle_mesh(dtype=np.float32)
    m64 = a.extract_triangle_mesh()
    assert m32.vertices.dtype == np.float32 and len(m64.triangles) > 0
    np.testing.assert_array_equal(m32.vertices, m64.vertices.astype(np.float32))
    np.testing.assert_array_equal(m32.vertex_colors, m64.vertex_colors.astype(np.float32))
    np.testing.assert_array_equal(m32.triangles, m64.triangles)
    same(a, b, points=False, dtype=np.float32)


def check_tick(vol, tick):
    """Check 2: the readers of the tick, warm against cold."""
    if not tick:
        return None
    twin = twin_of(vol)
    for reader in tick:
        if reader == "mesh":
            same(vol, twin, mesh=True, points=False)
        elif reader == "points":
            same(vol, twin, mesh=False, points=True)
        elif reader == "normals":
            same_normals(vol, twin)
        else:
            assert reader == "mesh32", reader
            same_mesh32(vol, twin)
    return twin


def read_everything(vol, dump):
    """ray_cast, sample_points, check_frame, distance_field, surface_components and pack() -> {name: array}."""
    s, frames = lc.frames_for(lc.tiny(1, 1))
    K = intrinsic(s)
    depth, _, T = frames[0]
    out = {}
    for name, a in vol.ray_cast(K, T, 0.1, 4.0).items():
        out["ray_cast " + name] = a
    res = vol.sample_points(lc.sample_positions(dump, 500), color=True)
    for name in ("sdf", "gradient", "color", "weight", "status"):
        out["sample " + name] = getattr(res, name)
    chk = vol.check_frame(depth, K, T, depth_max=4.0)
    out["check sdf"], out["check cls"], out["check stats"] = chk.sdf, chk.cls, np.array(chk.stats.as_tuple())
    keys = np.asarray(dump[0], np.float64)
    centre = (keys.mean(axis=0) + 0.5) * ps.UNIT
    field = vol.distance_field((centre - 0.4, centre + 0.4), 0.2, outputs=("distance", "dist2", "cls"))
    out["distance"], out["dist2"], out["distance cls"], out["distance stats"] = field.distance, field.dist2, field.cls, np.array(field.stats.as_tuple())
    comp = vol.surface_components(sites=True)
    for name in ("seed", "sites", "lo", "hi", "site_index", "site_label"):
        out["components " + name] = getattr(comp, name)
    out["components stats"] = np.array(comp.stats.as_tuple())
    out["pack"] = vol.pack()
    return out


def check_last(vol, twin, dump):
    a, b = read_everything(vol, dump), read_everything(twin, dump)
    assert a["ray_cast mask"].any() and (a["sample status"] > 1).any() and a["components stats"][2] >= 1 and a["distance stats"][3] > 0
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(bits(x), bits(y)), name
    assert assert_meshes_match(vol, ps.to_oracle(dump)) > 0


def check_dirty(vol, after, marked, step, label):
    """Check 3.  -> the dump taken at the last mark_merged."""
    assert_consistent(vol)
    dirty, held = key_set(vol.dirty_keys()), key_set(vol.unit_keys())
    if step.op == "mark_merged":
        assert not dirty, (label, len(dirty))
        return after
    index = {tuple(k): i for i, k in enumerate(marked[0].tolist())}
    changed = set()
    for i, key in enumerate(after[0].tolist()):
        j = index.get(tuple(key))
        if j is None or not all(np.array_equal(bits(a[i]), bits(m[j])) for a, m in zip(after[1:], marked[1:])):
            changed.add(tuple(key))
    assert changed <= dirty <= held, (label, sorted(changed - dirty), sorted(dirty - held))
    return marked


def moved_units(pool_before, pool_after, after):
    """key -> the unit's rows (bits) of the units that a prune moved to another pool slot."""
    was = {tuple(k): i for i, k in enumerate(np.asarray(pool_before).tolist())}
    index = {tuple(k): i for i, k in enumerate(after[0].tolist())}
    return {tuple(k): tuple(bits(a[index[tuple(k)]]).copy() for a in after[1:]) for i, k in enumerate(np.asarray(pool_after).tolist())
            if was[tuple(k)] != i}


def read_tick(vol, tick):
    """The tick's readers on the volume alone."""
    for reader in tick:
        if reader in lc.MESH_TICKS:
            vol.extract_triangle_mesh(dtype=np.float32 if reader == "mesh32" else None)
        else:
            vol.extract_point_cloud(normals=reader == "normals")


def run_script(name, checks=True):
    """The whole script.  checks=False: the calls and the ticks' readers alone.  -> the volume"""
    script = lc.SCRIPTS[name]
    vol = start_volume(script)
    marked = before = vol.dump()
    twin = moved = None
    for k, step in enumerate(script.steps):
        label = (name, k, step.op)
        if not checks:
            run_step(vol, step)
            read_tick(vol, step.tick)
            continue
        pool = vol.unit_keys() if step.op == "prune" else None
        stats = run_step(vol, step, before)
        after = check_step(vol, step, before, stats, label)
        if pool is not None and moved is None:
            moved = moved_units(pool, vol.unit_keys(), after)
            assert moved or name != "slots_move", label  # slots move
        if step.tick and moved:
            # units whose pool slot the script's first prune changed, still held and written by nothing since.  In slots_move every
            # cache was filled right before that prune: at this extraction only the re-key's new extraction epoch stands between the
            # masks cached for those slots and the mesh
            index = {tuple(k): i for i, k in enumerate(after[0].tolist())}
            still = [k for k, rows in moved.items() if k in index and all(np.array_equal(bits(a[index[k]]), r) for a, r in zip(after[1:], rows))]
            print(f"{name} step {k}: {len(moved)} units moved by the prune, {len(still)} of them unwritten at this extraction")
            assert still or name != "slots_move", label
            moved = ()
        twin = check_tick(vol, step.tick)
        marked = check_dirty(vol, after, marked, step, label)
        before = after
    if checks:
        check_last(vol, twin if twin is not None else twin_of(vol), before)
    return vol


# ---- the scripts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sorted(lc.SCRIPTS) if n not in lc.PIPELINE])
def test_script(name):
    t0 = time.time()
    run_script(name)
    print(f"{name}: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("name", lc.PIPELINE)
def test_pipeline_script(name, sweep_form):
    """Between two integrate_batch calls of a running chain: each of the operations the module docstring of lifetime_cases lists,
    in both forms of the sweep (the bitwise form holds every batch to the oracle bit for bit)."""
    t0 = time.time()
    run_script(name)
    print(f"{name} ({sweep_form}): {time.time() - t0:.1f} s")


def test_two_long_lived_volumes_do_not_share_state():
    """slots_move on one volume and the three pipeline scripts, one after the other on volumes of their own, step by step in turn in
    one process (the constant tables of hv_extract.hip are uploaded once per process; the scratch is the volume's own; the pipeline
    scripts rebuild the sweep's multiplier table and run ray_cast and sample_points): all end bitwise where they end alone."""
    alone = {name: run_script(name, checks=False) for name in ("slots_move",) + lc.PIPELINE}
    a = lc.SCRIPTS["slots_move"]
    va = start_volume(a)
    b_steps = [(name, step) for name in lc.PIPELINE for step in lc.SCRIPTS[name].steps]
    vb = {}
    for k in range(max(len(a.steps), len(b_steps))):
        name, step = b_steps[k] if k < len(b_steps) else (None, None)
        if name is not None and name not in vb:
            vb[name] = start_volume(lc.SCRIPTS[name])
        if k < len(a.steps):
            run_step(va, a.steps[k])
        if name is not None:
            run_step(vb[name], step)
            read_tick(vb[name], step.tick)  # (the readers in the other order)
        if k < len(a.steps):
            read_tick(va, a.steps[k].tick)
    for vol, name in [(va, "slots_move")] + [(vb[name], name) for name in lc.PIPELINE]:
        assert_bitwise(vol.dump(), alone[name].dump())
        same(vol, alone[name])  # (order-free: which pool slot a unit claims is decided by the order of the claims)
        same_normals(vol, alone[name])


# ---- sizes first, data second ------------------------------------------------------------------------------------------------------
def mesh_arrays(vol):
    m = vol.extract_triangle_mesh()
    return np.asarray(m.vertices), np.asarray(m.triangles), np.asarray(m.vertex_colors)


def mesh_query(vol, f32=False):
    from pyslam_amd import _lib as L

    fn = vol._lib.hv_tsdf_extract_mesh_f32 if f32 else vol._lib.hv_tsdf_extract_mesh
    nv, nt = ctypes.c_int64(-1), ctypes.c_int64(-1)
    L.check(fn(vol._h, None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt)))
    return int(nv.value), int(nt.value)


def mesh_fetch(vol, cap_v, cap_t):
    """The fetch with the capacities of an earlier query, into buffers of NaN / -1.  -> (vertices, colours, triangles, (nv, nt))"""
    from pyslam_amd import _lib as L

    verts, cols, tris = np.full((cap_v, 3), np.nan), np.full((cap_v, 3), np.nan), np.full((cap_t, 3), -1, np.int32)
    nv, nt = ctypes.c_int64(-1), ctypes.c_int64(-1)
    L.check(vol._lib.hv_tsdf_extract_mesh(vol._h, L.ptr(verts), L.ptr(cols), cap_v, L.ptr(tris), cap_t, ctypes.byref(nv), ctypes.byref(nt)))
    return verts, cols, tris, (int(nv.value), int(nt.value))


def points_query(vol, f32=False):
    from pyslam_amd import _lib as L

    fn = vol._lib.hv_tsdf_extract_points_f32 if f32 else vol._lib.hv_tsdf_extract_points
    n = ctypes.c_int64(-1)
    L.check(fn(vol._h, None, None, 0, ctypes.byref(n)))
    return int(n.value)


def points_fetch(vol, cap):
    from pyslam_amd import _lib as L

    pts, cols = np.full((cap, 3), np.nan), np.full((cap, 3), np.nan)
    n = ctypes.c_int64(-1)
    L.check(vol._lib.hv_tsdf_extract_points(vol._h, L.ptr(pts), L.ptr(cols), cap, ctypes.byref(n)))
    return pts, cols, int(n.value)


def fused_tiny_map():
    vol = fresh()
    run_step(vol, lc.Step("fuse_batch", lc.tiny(0, 4)))
    return vol


def _sample(vol):
    vol.sample_points(lc.sample_positions(vol.dump(), 500), color=True)


def _check_frame(vol):
    s, frames = lc.frames_for(lc.tiny(1, 1))
    vol.check_frame(frames[0][0], intrinsic(s), frames[0][2], depth_max=4.0)


def _distance(vol):
    centre = (np.asarray(vol.unit_keys(), np.float64).mean(axis=0) + 0.5) * ps.UNIT
    vol.distance_field((centre - 0.3, centre + 0.3), 0.2)


READS = {
    "the other size query": None,  # points for the mesh protocol, mesh for the points protocol
    "point normals": lambda v: v.extract_point_cloud(normals=True),
    "ray_cast": lambda v: run_step(v, lc.Step("ray_cast", lc.tiny(1, 1))),
    "sample_points": _sample,
    "check_frame": _check_frame,
    "distance_field": _distance,
    "surface_components": lambda v: v.surface_components(sites=True),
    "pack": lambda v: v.pack(),
    "dirty_keys": lambda v: v.dirty_keys(),
    "the float32 size query": None,
    "a prune that releases nothing": lambda v: run_step(v, lc.Step("prune", lc.EVERYTHING)),
    "a removal that removes nothing": lambda v: run_step(v, lc.Step("remove_small", (1, 1))),
}
WRITES = {
    "fuse_batch": lc.Step("fuse_batch", lc.tiny(20, 1)),
    "fuse": lc.Step("fuse", lc.tiny(24, 1)),
    "deintegrate_batch": lc.Step("deintegrate_batch", lc.tiny(1, 2)),
    "merge": lc.Step("merge", ("blob", "into view")),
    "remove_small": lc.Step("remove_small", (1 << 40, 1)),  # every component goes
    "prune": lc.Step("prune", (True, (2, -1, 1), (5, 4, 3))),
    "repack": lc.Step("repack", None),
}


def test_size_query_then_anything_then_fetch():
    """At the C ABI: the size query does the device work into buffers that other calls share (out_a: mesh, points, dirty_keys; out_b:
    triangles, point normals); whatever is called before the fetch, the fetch returns the CURRENT map's result - recomputed where
    the call in between overwrote or invalidated the cached one - in at most the capacities it was given."""
    vol = fused_tiny_map()
    twin = twin_of(vol)
    want_mesh = mesh_rows(*mesh_arrays(twin))
    tp = twin.extract_point_cloud()
    want_points = sorted_rows(tp.points, tp.colors)
    dump = vol.dump()
    for name, call in READS.items():
        # mesh: query, the call, fetch
        nv, nt = mesh_query(vol)
        assert (nv, nt) == (len(want_mesh[0]), len(want_mesh[1])) and nt > 0
        if name == "the other size query":
            points_query(vol)
        elif name == "the float32 size query":
            mesh_query(vol, f32=True)
        else:
            call(vol)
        verts, cols, tris, counts = mesh_fetch(vol, nv, nt)
        assert counts == (nv, nt), (name, counts)
        assert_same_rows(mesh_rows(verts, tris, cols), want_mesh, ("mesh after", name))
        # points: query, the call, fetch
        n = points_query(vol)
        assert n == len(want_points) > 0
        if name == "the other size query":
            mesh_query(vol)
        elif name == "the float32 size query":
            points_query(vol, f32=True)
        else:
            call(vol)
        pts, pcols, got = points_fetch(vol, n)
        assert got == n, (name, got)
        assert_same_rows([sorted_rows(pts, pcols)], [want_points], ("points after", name))
    assert_bitwise(vol.dump(), dump)
    # a writer between the query and the fetch: the fetch returns the NEW map's counts and, row for row, the start of its result
    for name, step in WRITES.items():
        for what in ("mesh", "points"):
            vol = fused_tiny_map()
            before = vol.dump()
            caps = mesh_query(vol) if what == "mesh" else (points_query(vol),)
            run_step(vol, step)
            after = vol.dump()
            assert not lc.same_bits(before, after) or name == "repack", name
            if what == "mesh":
                verts, cols, tris, counts = mesh_fetch(vol, *caps)
                full = mesh_arrays(vol)
                assert counts == (len(full[0]), len(full[1])), (name, counts)
                nv, nt = min(caps[0], counts[0]), min(caps[1], counts[1])
                assert np.array_equal(bits(verts[:nv]), bits(full[0][:nv])) and np.array_equal(bits(cols[:nv]), bits(full[2][:nv])), name
                assert np.array_equal(tris[:nt], full[1][:nt]), name
                assert np.isnan(verts[nv:]).all() and (tris[nt:] == -1).all(), name  # nothing beyond what the new result holds
                assert_same_rows(mesh_rows(*full), mesh_rows(*mesh_arrays(twin_of(vol))), ("mesh after", name))
            else:
                pts, pcols, got = points_fetch(vol, *caps)
                full = vol.extract_point_cloud()
                assert got == len(full.points), (name, got)
                n = min(caps[0], got)
                assert np.array_equal(bits(pts[:n]), bits(np.asarray(full.points)[:n])) and np.array_equal(bits(pcols[:n]), bits(np.asarray(full.colors)[:n])), name
                assert np.isnan(pts[n:]).all(), name
                tw = twin_of(vol).extract_point_cloud()
                assert_same_rows([sorted_rows(full.points, full.colors)], [sorted_rows(tw.points, tw.colors)], ("points after", name))
            assert_bitwise(vol.dump(), after)
