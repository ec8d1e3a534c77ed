"""GPU: ScalableTSDFVolume.surface_components / remove_small_components (hv_tsdf_surface_components, hv_tsdf_remove_components,
hv_components.hip) on planted voxel states (tests/planted_states.py, tests/components_cases.py), held to the numpy restatement
(tests/components_reference.py) run on the planted volume's OWN dump().

Bar: the table, the site list, the stats and the dump after a removal EQUAL to the restatement.  The contract is integer throughout:
there is no fragile point and no allowance.  Voxel 0.02, sdf_trunc 0.08.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

from tests import components_cases as cc
from tests import components_reference as cr
from tests import planted_states as ps
from tests.test_gpu_tsdf_deintegrate import assert_bitwise
from tests.test_gpu_tsdf_edges import intrinsic, tiny_frames, volume

pytestmark = pytest.mark.gpu

VOX, TRUNC = cc.VOX, cc.TRUNC
TABLE = ("seed", "sites", "lo", "hi")
LIST = ("site_index", "site_label")
OUTPUTS = TABLE + LIST
DTYPES = {"seed": np.int32, "sites": np.int64, "lo": np.int32, "hi": np.int32, "site_index": np.int32, "site_label": np.int32}
HV_ERR_INVALID, HV_ERR_MODE = -1, -4
CASES = [(name, thr) for name, (_, thresholds, _) in cc.STATES.items() for thr in thresholds]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@functools.lru_cache(maxsize=None)
def planted(name):
    """-> (volume, its dump) of the named state of components_cases.STATES.  Shared by the tests that only read."""
    states = cc.STATES[name][0]()
    vol = ps.plant(volume(VOX, TRUNC), states)
    assert_bitwise(vol.dump(), ps.as_dump(states))
    return vol, vol.dump()


@functools.lru_cache(maxsize=None)
def reference(name, threshold):
    return cr.components(planted(name)[1], threshold)


def shapes(C, N):
    return {"seed": (C, 3), "sites": (C,), "lo": (C, 3), "hi": (C, 3), "site_index": (N, 3), "site_label": (N,)}


def call_abi(vol, threshold=0.0, want=OUTPUTS, stats=True, device=False, caps=None, loc=None, check=True):
    """hv_tsdf_surface_components, count then fill, with exactly the outputs `want` (the others NULL).  Buffers start as 0xAB bytes.
    caps = (component_cap, site_cap) overrides the capacities of the fill call.  -> ({name: array}, (C, N), stats tuple or None, rc)."""
    from pyslam_amd import _lib as L

    nc, ns = ctypes.c_int64(-1), ctypes.c_int64(-1)
    fn = vol._lib.hv_tsdf_surface_components
    rc = fn(vol._h, float(threshold), None, None, None, None, 0, None, None, 0, ctypes.byref(nc), ctypes.byref(ns), None, L.HV_HOST)
    if rc != 0:
        if check:
            L.check(rc)
        return {}, (nc.value, ns.value), None, rc
    C, N = int(nc.value), int(ns.value)
    shp = shapes(C, N)
    out = {name: np.full(int(np.prod(shp[name])) * np.dtype(DTYPES[name]).itemsize, 0xAB, np.uint8).view(DTYPES[name]).reshape(shp[name])
           for name in want}
    held = out
    if device:
        import torch

        held = {name: torch.from_numpy(a).cuda() for name, a in out.items()}
        torch.cuda.synchronize()
    st = L.HvComponentsStats(-1, -1, -1, -1)
    ccap, scap = caps if caps is not None else (C, N)
    rc = fn(vol._h, float(threshold), *(L.ptr(held.get(name)) for name in TABLE), ccap, *(L.ptr(held.get(name)) for name in LIST), scap,
            ctypes.byref(nc), ctypes.byref(ns), ctypes.byref(st) if stats else None,
            loc if loc is not None else (L.HV_DEVICE if device else L.HV_HOST))
    if check:
        L.check(rc)
    if device:
        vol.synchronize()
        out = {name: t.cpu().numpy() for name, t in held.items()}
    return out, (int(nc.value), int(ns.value)), ((st.units, st.sites, st.components, st.largest) if stats else None), rc


def assert_equal(got, ref, label, names=OUTPUTS):
    for name in names:
        g, r = np.asarray(got[name]), np.asarray(ref[name])
        assert g.shape == r.shape and g.dtype == r.dtype, (label, name, g.shape, g.dtype, r.shape, r.dtype)
        assert np.array_equal(g, r), (label, name, int((g != r).sum()))


def result_dict(res):
    return {name: (getattr(res, name).cpu().numpy() if hasattr(getattr(res, name), "is_cuda") else getattr(res, name)) for name in OUTPUTS
            if getattr(res, name) is not None}


# ---- labelling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,threshold", CASES)
def test_table_list_and_stats_equal_the_restatement(name, threshold):
    """Through the ABI with host and with device buffers, and through the Python method, sites on and off, numpy and torch."""
    vol, _ = planted(name)
    ref = reference(name, threshold)
    expected = cc.STATES[name][2]
    if expected is not None:
        assert ref["stats"][2] == expected[cc.STATES[name][1].index(threshold)]
    print(f"{name} @ {threshold}: units, sites, components, largest = {ref['stats']}")
    for device in (False, True):
        got, counts, stats, _ = call_abi(vol, threshold, device=device)
        assert counts == (ref["stats"][2], ref["stats"][1]) and stats == ref["stats"], (name, device, counts, stats, ref["stats"])
        assert_equal(got, ref, (name, threshold, device))
    for sites, device in itertools.product((False, True), repeat=2):
        res = vol.surface_components(weight_threshold=threshold, sites=sites, device=device)
        assert res.stats.as_tuple() == ref["stats"] and len(res) == ref["stats"][2]
        if device:
            import torch

            assert all(isinstance(getattr(res, n), torch.Tensor) and getattr(res, n).is_cuda for n in (TABLE + LIST if sites else TABLE))
        if not sites:
            assert res.site_index is None and res.site_label is None
        assert_equal(result_dict(res), ref, (name, threshold, sites, device), TABLE + (LIST if sites else ()))


def test_every_subset_of_null_outputs():
    """Any output may be NULL, the stats too: what is asked for equals the full call, and the counts are always written."""
    vol, _ = planted("two blobs")
    ref = reference("two blobs", 0.0)
    for k in range(len(OUTPUTS) + 1):
        for want in itertools.combinations(OUTPUTS, k):
            for stats in (True, False):
                got, counts, st, _ = call_abi(vol, want=want, stats=stats)
                assert set(got) == set(want) and counts == (ref["stats"][2], ref["stats"][1])
                assert_equal(got, ref, (want, stats), want)
                assert st == (ref["stats"] if stats else None)
    # a part of the outputs as device pointers
    for want in (("site_label",), ("seed", "site_index"), ("sites", "hi")):
        assert_equal(call_abi(vol, want=want, device=True)[0], ref, want, want)


def test_another_pool_order_gives_the_same_bits():
    """The same state planted with its units shuffled, and after a prune that moved units into holes: every output is bitwise equal."""
    for name, threshold in (("serpentine", 0.0), ("cluster", 3.0), ("dust", 0.0)):
        states = cc.STATES[name][0]()
        ref = reference(name, threshold)
        order = np.random.default_rng(4).permutation(len(states[0]))
        shuffled = ps.plant(volume(VOX, TRUNC), tuple(np.asarray(a)[order] for a in states))
        # empty units claimed FIRST take the low pool slots: releasing them moves the tail's survivors into the holes
        holes = np.array([(40 + i, -40, 7) for i in range(9)], np.int64)
        moved = ps.plant(ps.plant(volume(VOX, TRUNC), ps.empty_units(holes)), tuple(np.asarray(a)[order[::-1]] for a in states))
        assert moved.prune(empty=True).units_empty == len(holes)
        for vol in (shuffled, moved):
            assert_bitwise(vol.dump(), planted(name)[1])
            got, _, stats, _ = call_abi(vol, threshold)
            assert_equal(got, ref, name)
            assert stats == ref["stats"]


def test_the_query_only_reads():
    vol = ps.plant(volume(VOX, TRUNC), cc.two_blobs_states())
    mesh = vol.extract_triangle_mesh()
    before = (vol.dump(), vol.dirty_keys(), vol.touched_keys(), vol.num_blocks())
    call_abi(vol)
    vol.surface_components(sites=True)
    vol.surface_components(weight_threshold=2.0, device=True)
    assert_bitwise(vol.dump(), before[0])
    assert np.array_equal(vol.dirty_keys(), before[1]) and np.array_equal(vol.touched_keys(), before[2]) and vol.num_blocks() == before[3]
    again = vol.extract_triangle_mesh()
    for name in ("vertices", "triangles", "vertex_colors"):
        a, b = np.asarray(getattr(again, name)), np.asarray(getattr(mesh, name))
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), name


def test_empty_map_and_a_map_without_a_site():
    empty = volume(VOX, TRUNC)
    for vol, units in ((empty, 0), (planted("no site")[0], len(planted("no site")[1][0]))):
        got, counts, stats, _ = call_abi(vol)
        assert counts == (0, 0) and stats == (units, 0, 0, 0) and all(got[n].shape == shapes(0, 0)[n] for n in OUTPUTS)
        res = vol.surface_components(sites=True)
        assert len(res) == 0 and res.seed.shape == (0, 3) and res.site_label.shape == (0,)
    before = empty.dirty_keys()
    assert tuple(empty.remove_small_components(5)) == (0, 0, 0, 0, 0, 0, 0) and empty.num_blocks() == 0
    assert np.array_equal(empty.dirty_keys(), before)
    vol = ps.plant(volume(VOX, TRUNC), cc.STATES["no site"][0]())
    dump = vol.dump()
    assert tuple(vol.remove_small_components(1000, margin=16)) == (0, 0, 0, 0, 0, 0, 0)
    assert_bitwise(vol.dump(), dump)


# ---- removal ---------------------------------------------------------------------------------------------------------------------
REMOVALS = [("two blobs", 0.0), ("corner apart", 0.0), ("dust", 0.0), ("mixed weights", 2.0), ("cluster", 3.0)]
EXACT_ROUND_TRIP = ("two blobs", "dust")  # weights 4 and 2: planting the expected dump reproduces it bit for bit


def mesh_arrays(vol):
    mesh = vol.extract_triangle_mesh()
    return tuple(np.asarray(getattr(mesh, name)) for name in ("vertices", "triangles", "vertex_colors"))


def canonical(vol):
    """The mesh in the order-free form of tests/conftest.py: two volumes need not hold their units in the same pool order."""
    from tests.conftest import canonical_mesh

    return canonical_mesh(*mesh_arrays(vol))


@pytest.mark.parametrize("name,threshold", REMOVALS)
def test_removal_equals_the_restatement(name, threshold):
    """min_sites in {1, 8, half the largest, largest + 1} x margin in {0, 1, 4, 16}: dump and stats equal the restatement's; the
    units it changed, and only those, carry a new stamp; a second identical call resets nothing and stamps nothing; the mesh equals
    that of a fresh volume planted with the expected dump (the caches were invalidated)."""
    states = cc.STATES[name][0]()
    dump = planted(name)[1]
    largest = reference(name, threshold)["stats"][3]
    for min_sites, margin in itertools.product(cc.min_sites_axis(largest), cc.MARGINS):
        expected, ref_stats = cr.remove_components(dump, min_sites, margin, threshold, ref=reference(name, threshold))
        vol = ps.plant(volume(VOX, TRUNC), states)
        check_mesh = name in EXACT_ROUND_TRIP and margin in (0, 4)
        if check_mesh:
            mesh_arrays(vol)  # fill the extraction caches with the map as it is BEFORE the removal
        vol.mark_merged()
        assert len(vol.dirty_keys()) == 0
        stats = vol.remove_small_components(min_sites, weight_threshold=threshold, margin=margin)
        print(f"{name} @ {threshold}: min_sites {min_sites}, margin {margin}: {stats}")
        assert tuple(stats) == ref_stats, (name, min_sites, margin, tuple(stats), ref_stats)
        after = vol.dump()
        assert_bitwise(after, expected)
        changed = np.array([k for k, a, b in zip(dump[0], dump[2], expected[2]) if not np.array_equal(a, b)], np.int32).reshape(-1, 3)
        assert len(changed) == stats.units_changed and np.array_equal(vol.dirty_keys(), changed), (name, min_sites, margin)
        assert vol.num_blocks() == len(dump[0])  # no unit is released
        if check_mesh:
            fresh = ps.plant(volume(VOX, TRUNC), expected)
            assert_bitwise(fresh.dump(), expected)
            for a, b in zip(canonical(vol), canonical(fresh)):
                assert a.shape == b.shape and np.array_equal(a, b), (name, min_sites, margin)
        vol.mark_merged()
        second = vol.remove_small_components(min_sites, weight_threshold=threshold, margin=margin)
        assert second.voxels_reset == 0 and second.components_removed == 0 and second.units_changed == 0
        assert second.components == stats.components - stats.components_removed and second.sites == stats.sites - stats.sites_removed
        assert len(vol.dirty_keys()) == 0
        assert_bitwise(vol.dump(), expected)


def test_default_margin_is_the_band_and_prune_releases_what_the_reference_says():
    """margin=None is min(16, ceil(sdf_trunc / voxel_length)) = 4.  Dust with a large min_sites: every speck goes and, within four
    voxels of one everywhere, every voxel with it; prune(empty=True) then releases exactly the units the reference finds empty."""
    for name, min_sites in (("dust", 1000), ("two blobs", int(reference("two blobs", 0.0)["sites"][1]) + 1)):
        vol = ps.plant(volume(VOX, TRUNC), cc.STATES[name][0]())
        expected, ref_stats = cr.remove_components(planted(name)[1], min_sites, 4, ref=reference(name, 0.0))
        stats = vol.remove_small_components(min_sites)
        assert tuple(stats) == ref_stats
        empty = cr.empty_units(expected)
        assert stats.units_emptied == len(empty) == (64 if name == "dust" else 1)
        pruned = vol.prune(empty=True)
        assert pruned.units_empty == len(empty) and pruned.units_after == len(expected[0]) - len(empty)
        keep = np.array([not (k == empty).all(axis=1).any() for k in expected[0]], bool)
        assert_bitwise(vol.dump(), tuple(a[keep] for a in expected))


def test_a_floater_in_a_fused_map_goes_and_the_rest_keeps_its_triangles():
    s, frames = tiny_frames(0, 8)
    vol = volume(VOX, TRUNC)
    for d, c, T in frames:
        vol.integrate_batch(d[None], c[None], intrinsic(s), T[None], 1.0, 4.0)
    floater = cc._band(lambda p: np.linalg.norm(p - np.array(cc.SMALL_CENTRE) * VOX, axis=-1) - cc.SMALL_RADIUS * VOX, [(2, 0, 0)])
    shift = vol.unit_keys().max(axis=0).astype(np.int64) + 3 - np.array([2, 0, 0])  # three units beyond the map on every axis
    floater = (floater[0] + shift.astype(np.int32),) + tuple(floater[1:])
    size = int(cr.components(ps.as_dump(floater))["sites"][0])
    # the fused map's own specks of that size go first: what is left is the map the floater is then planted into
    vol.remove_small_components(size + 1)
    clean = vol.surface_components()
    assert len(clean) >= 1 and int(clean.sites.min()) > size
    triangles = len(mesh_arrays(vol)[1])
    assert triangles > 1000
    ps.plant(vol, floater)
    with_floater = vol.surface_components()
    assert len(with_floater) == len(clean) + 1 and size in with_floater.sites.tolist()
    assert len(mesh_arrays(vol)[1]) > triangles
    stats = vol.remove_small_components(size + 1)
    print(f"fused map: {len(clean)} components, floater of {size} sites: {stats}")
    assert stats.components_removed == 1 and stats.sites_removed == size and stats.units_changed == 1 and stats.units_emptied == 1
    assert len(mesh_arrays(vol)[1]) == triangles
    after = vol.surface_components()
    assert len(after) == len(clean) and np.array_equal(after.seed, clean.seed) and np.array_equal(after.sites, clean.sites)


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_by_return_code_leave_the_volume_alone():
    from pyslam_amd import _lib as L
    from pyslam_amd.volumetric import VoxelBlockGrid

    vol = ps.plant(volume(VOX, TRUNC), cc.two_blobs_states())
    vol.mark_merged()
    dump = vol.dump()
    C, N = reference("two blobs", 0.0)["stats"][2], reference("two blobs", 0.0)["stats"][1]

    def label_refused(v, code, threshold=0.0, want=OUTPUTS, caps=None, loc=None):
        """The fill call returns `code` and writes no buffer."""
        nc, ns = ctypes.c_int64(-7), ctypes.c_int64(-7)
        out = {name: np.full(int(np.prod(shapes(C, N)[name])) * np.dtype(DTYPES[name]).itemsize, 0xAB, np.uint8).view(DTYPES[name]) for name in want}
        st = L.HvComponentsStats(-1, -1, -1, -1)
        ccap, scap = caps if caps is not None else (C, N)
        rc = v._lib.hv_tsdf_surface_components(v._h, float(threshold), *(L.ptr(out.get(n)) for n in TABLE), ccap, *(L.ptr(out.get(n)) for n in LIST),
                                               scap, ctypes.byref(nc), ctypes.byref(ns), ctypes.byref(st), L.HV_HOST if loc is None else loc)
        assert rc == code, (rc, code)
        assert all((bits(a) == 0xAB).all() for a in out.values()) and st.largest == -1
        assert L.load().hv_last_error()
        return nc.value, ns.value

    def remove_refused(v, code, threshold=0.0, min_sites=5, margin=1):
        st = L.HvRemoveComponentsStats(-1, -1, -1, -1, -1, -1, -1)
        rc = v._lib.hv_tsdf_remove_components(v._h, float(threshold), int(min_sites), int(margin), ctypes.byref(st))
        assert rc == code and st.voxels_reset == -1 and L.load().hv_last_error(), (rc, code)

    grid = VoxelBlockGrid(0.02, 8, max_blocks=1 << 10, max_points=1 << 12)
    owner = volume(VOX, TRUNC)
    owner.set_owner(0, 2)
    tiled = volume(VOX, TRUNC)
    tiled.set_tile(0, 0, 80, 120)
    for v in (grid, owner, tiled):
        label_refused(v, HV_ERR_MODE)
        remove_refused(v, HV_ERR_MODE)
    with pytest.raises(L.HipVolError, match="owner-sharded"):
        owner.surface_components()
    with pytest.raises(L.HipVolError, match="tile-sharded"):
        tiled.remove_small_components(5)
    for threshold in (-1.0, float("nan"), float("inf")):
        label_refused(vol, HV_ERR_INVALID, threshold=threshold)
        remove_refused(vol, HV_ERR_INVALID, threshold=threshold)
        with pytest.raises(L.HipVolError, match="weight_threshold"):
            vol.surface_components(weight_threshold=threshold)
    label_refused(vol, HV_ERR_INVALID, loc=2)
    # capacities: too small for what is asked for (the counts are still written); not looked at for what is not
    assert label_refused(vol, HV_ERR_INVALID, caps=(C - 1, N)) == (C, N)
    assert label_refused(vol, HV_ERR_INVALID, caps=(C, N - 1)) == (C, N)
    assert label_refused(vol, HV_ERR_INVALID, want=("site_label",), caps=(C, N - 1)) == (C, N)
    label_refused(vol, HV_ERR_INVALID, want=("seed",), caps=(-1, 0))
    assert_equal(call_abi(vol, want=TABLE, caps=(C, 0))[0], reference("two blobs", 0.0), "table alone", TABLE)
    assert_equal(call_abi(vol, want=LIST, caps=(0, N))[0], reference("two blobs", 0.0), "list alone", LIST)
    for min_sites in (0, -1, -(1 << 40)):
        remove_refused(vol, HV_ERR_INVALID, min_sites=min_sites)
        with pytest.raises(L.HipVolError, match="min_sites"):
            vol.remove_small_components(min_sites)
    for margin in (-1, 17, 1 << 20):
        remove_refused(vol, HV_ERR_INVALID, margin=margin)
        with pytest.raises(L.HipVolError, match="margin"):
            vol.remove_small_components(5, margin=margin)
    assert_bitwise(vol.dump(), dump)
    assert len(vol.dirty_keys()) == 0 and vol.num_blocks() == len(dump[0])
    # the limits themselves are accepted: nothing is smaller than one site
    assert vol.remove_small_components(1, margin=16).voxels_reset == 0 and vol.remove_small_components(1 << 62, margin=0).components_removed == C
