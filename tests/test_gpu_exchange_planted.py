"""GPU: the multi-GPU exchange on planted inputs (tests/exchange_cases.py) against its numpy restatement
(tests/exchange_reference.py, which tests/test_exchange_reference_cpu.py ties to the host plan and to float64) - no process group:
volumes and one grid in this process play the ranks, a sum plays the all-reduce, a concatenation the all-gather.

a. hv_merge_halo_plan_device on planted key lists: keys, actions and row order, per rank; replaced, empty and refused plans.
b. hv_merge_halo_lists_device on volumes of 0 .. 600 units, dirty patterns, buffers shorter than the lists.
c. export / import / halo pack / unpack (host and device payloads, planned ranges), bit for bit on planted unit states.
d. two whole merge windows through the host path and the device path, and the invariant of include/hipvol.h.
e. extraction, ray cast and samples from warm caches after the writers that stamp no unit.
f. hv_assoc_pairs_export / _import on planted pair lists, and the two capacity conditions the code counts.

Bitwise is the bar for the tsdf plane: pyslam_amd/build.py compiles without contraction and fast math and with IEEE float32
division, so N / W on the device is the float32 quotient numpy computes.  Nothing here writes past a buffer or drives the vote
table to capacity: 6000 pairs go into a table of 65 536 slots.

The warm-cache twin is tests/test_gpu_lifetime.py's twin_of (pack -> unpack into a fresh volume: the pool's bits, no cache).

Measured on the MI355X when the file was written: every case equal to the restatement, the file in about 4 s.  On scratch copies
of the library (none committed), each run under this file: the keeper of k_halo_decide taken from the LAST holder fails 18 tests
(the device plan on 9 key lists, every planned pack and unpack, the merge windows); k_tsdf_halo_unpack without its `wf > 0.f`
guard fails 7 (halo_unpack on every unit case, the planned ranges, the windows); hv_merge_halo_unpack_planned without `+ first`
on its action pointer fails 3 (the planned ranges, the windows for 3 and 8 ranks); k_assoc_pairs_import reading every rank at
rank 0's offset fails 28 (every pair case of more than one rank, the list above 4096 pairs).  test_refused_lists_leave_no_plan
came with a fix: hv_merge_halo_plan_device used to reset the stored plan only after its argument checks, so a refused call kept
the plan of earlier lists (read off the code; the test was not run against the old library).
"""
import ctypes
import functools
import types

import numpy as np
import pytest

from tests import exchange_cases as EC
from tests import exchange_reference as ER
from tests import lifetime_cases as lc
from tests import pack_reference as PR
from tests import planted_states as ps
from tests.assoc_rules_reference import decide, pack_pairs
from tests.test_gpu_lifetime import same, same_mesh32, same_normals, twin_of

pytestmark = pytest.mark.gpu

SENTINEL = -0x0123456789ABCDEF  # an int64 no packed key and no message word equals
NV = ps.NV


def volume(max_blocks=1 << 10):
    from pyslam_amd.volumetric import ScalableTSDFVolume

    return ScalableTSDFVolume(ps.VOX, ps.TRUNC, max_blocks=max_blocks)


def holding(state, max_blocks=1 << 10):
    """A fresh volume that holds the state, bit for bit (every unit dirty)."""
    vol = volume(max_blocks)
    if len(state[0]):
        vol.unpack(EC.state_buffer(state))
    return vol


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_state(vol, want, label):
    assert ER.same_state(PR.state_of_volume(vol), want) is None, (label, ER.same_state(PR.state_of_volume(vol), want))


def rows(keys, action):
    return [tuple(k) + (int(a),) for k, a in zip(np.asarray(keys).tolist(), np.asarray(action).tolist())]


# ---- a. the device plan ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gathered(name):
    """The case's padded lists on the device (shared: only read)."""
    import torch

    case = next(c for c in EC.key_list_cases() if c.name == name)
    da, dc, ha, hc = EC.padded(case)
    out = case, cuda(da), dc, cuda(ha), hc
    torch.cuda.synchronize()
    return out


def plan(vol, name, rank, all_dirty_kept=False):
    case, da, dc, ha, hc = gathered(name)
    n = vol.halo_plan_device(da, dc, ha, hc, case.world, rank, all_dirty_kept)
    keys, action = vol.halo_plan_fetch()
    assert n == len(keys) == len(action)
    return keys, action


@pytest.fixture(scope="module")
def planner():
    return volume(64)


@pytest.mark.parametrize("name", [c.name for c in EC.key_list_cases()])
def test_device_plan_equals_the_restatement_in_packed_order(planner, name):
    case = gathered(name)[0]
    for rank in case.ranks():
        keys, action = plan(planner, name, rank)
        want = ER.plan_held(case.dirty, case.held, case.world, rank, order="packed")
        assert rows(keys, action) == rows(*want), (name, rank)
        assert keys.dtype == np.int32 and action.dtype == np.uint8


@pytest.mark.parametrize("name", ["w1 dirty and held", "w1 one entry", "w3 rules"])
def test_all_dirty_kept_shares_every_dirty_key_as_its_keeper(planner, name):
    case = gathered(name)[0]
    for rank in case.ranks():
        keys, action = plan(planner, name, rank, all_dirty_kept=True)
        want = ER.plan_held(case.dirty, case.held, case.world, rank, all_dirty_kept=True, order="packed")
        assert rows(keys, action) == rows(*want), (name, rank)
        assert len(keys) == len({tuple(k) for d in case.dirty for k in d.tolist()})


def test_a_second_plan_replaces_the_first_and_an_empty_one_leaves_nothing(planner):
    import torch

    assert len(plan(planner, "w3 rules", 0)[0]) == 4
    assert plan(planner, "w8 straddle total 257", 3)[0].tolist() == [[0, 0, 0]]
    assert len(plan(planner, "w3 all empty", 1)[0]) == 0
    payload = torch.zeros((1, NV, 5), dtype=torch.float32, device="cuda")
    planner.halo_pack_planned(0, 0, payload)
    planner.halo_unpack_planned(0, 0, payload)
    planner.synchronize()
    assert planner.num_blocks() == 0


def test_refused_lists_leave_no_plan(planner):
    import torch

    from pyslam_amd._lib import HipVolError

    case, da, dc, ha, hc = gathered("w3 rules")
    wide = torch.zeros((65, da.shape[1]), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert len(plan(planner, "w3 rules", 0)[0]) == 4
    with pytest.raises(HipVolError, match="bad rank / world size"):
        planner.halo_plan_device(wide, np.zeros(65, np.int64), wide, np.zeros(65, np.int64), 65, 0)
    assert [len(x) for x in planner.halo_plan_fetch()] == [0, 0]
    assert len(plan(planner, "w3 rules", 0)[0]) == 4
    long = dc.copy()
    long[1] = da.shape[1] + 1
    with pytest.raises(HipVolError, match="longer than its stride"):
        planner.halo_plan_device(da, long, ha, hc, 3, 0)
    assert [len(x) for x in planner.halo_plan_fetch()] == [0, 0]
    with pytest.raises(HipVolError, match="range outside the plan"):
        planner.halo_pack_planned(0, 1, torch.zeros((1, NV, 5), dtype=torch.float32, device="cuda"))
    for rank in (-1, 3):
        with pytest.raises(HipVolError, match="bad rank / world size"):
            planner.halo_plan_device(da, dc, ha, hc, 3, rank)
    assert len(plan(planner, "w64 straddle", 63)[0]) == 1  # world 64 is taken


# ---- b. the device lists ---------------------------------------------------------------------------------------------------------
def plant_empty(vol, keys, chunk=256, payload=None):
    """Units through import_numerators, `chunk` at a time from one payload (all zero by default).  Import stamps nothing."""
    keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 3)
    payload = np.zeros((min(chunk, max(len(keys), 1)), NV, 5), np.float32) if payload is None else payload
    for lo in range(0, len(keys), chunk):
        part = np.ascontiguousarray(keys[lo:lo + chunk])
        vol.import_numerators(part, payload[:len(part)])


def stamp(vol, keys):
    """Make the units `keys` dirty where they lie in the pool: a source volume with one observed voxel in each is fused in."""
    keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 3)
    payload = np.zeros((min(256, len(keys)), NV, 5), np.float32)
    payload[:, 77] = (0.5, 1.0, 10.0, 20.0, 30.0)
    src = volume(max(64, 2 * len(keys)))
    plant_empty(src, keys, payload=payload)
    vol.integrate_volume(src)


def unit_line(n):
    """n keys whose (x, y, z) order, packed order and planting order all differ."""
    j = np.arange(n, dtype=np.int64)
    return np.stack([(j * 7) % 1009 - 500, j % 5 - 2, 3 - j % 4 - j // 1009], axis=1)


def device_lists(vol, cap_dirty=None, cap_held=None):
    """-> (n_dirty, n_held, the whole dirty buffer, the whole held buffer): the call sees views of cap_* words (default: num_blocks)
    of buffers 8 words longer, filled with SENTINEL."""
    import torch

    nb = vol.num_blocks()
    cd, ch = (nb if cap_dirty is None else cap_dirty), (nb if cap_held is None else cap_held)
    d = torch.full((max(nb, cd) + 8,), SENTINEL, dtype=torch.int64, device="cuda")
    h = torch.full((max(nb, ch) + 8,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nd, nh = vol.halo_lists_device(d[:cd], h[:ch])
    return nd, nh, d.cpu().numpy(), h.cpu().numpy()


def packed_set(keys):
    return set(ER.pack_key(np.asarray(keys).reshape(-1, 3)).view(np.int64).tolist())


def check_lists(vol, dirty_keys, all_keys, label):
    want_d, want_h = packed_set(dirty_keys), packed_set(all_keys)
    assert packed_set(vol.dirty_keys()) == want_d and packed_set(vol.unit_keys()) == want_h, label
    nd, nh, d, h = device_lists(vol)
    assert (nd, nh) == (len(want_d), len(want_h)), label
    assert set(d[:nd].tolist()) == want_d and set(h[:nh].tolist()) == want_h, label
    assert (d[nd:] == SENTINEL).all() and (h[nh:] == SENTINEL).all(), label
    # buffers shorter than the lists: full counts, the first cap entries a subset without repeats, nothing behind the view
    # (at least one word each: a view of no words has no address, and a null buffer asks for the sizes only)
    for cd, ch in ((1, max(nh, 1)), (max(nd - 1, 1), 1), (max(nd // 2, 1), max(nh // 2, 1)), (max(nd, 1), max(nh - 1, 1))):
        md, mh, d, h = device_lists(vol, cd, ch)
        assert (md, mh) == (nd, nh), (label, cd, ch)
        got_d, got_h = d[:min(cd, nd)].tolist(), h[:min(ch, nh)].tolist()
        assert set(got_d) <= want_d and len(set(got_d)) == len(got_d) and set(got_h) <= want_h and len(set(got_h)) == len(got_h), (label, cd, ch)
        assert (d[min(cd, nd):] == SENTINEL).all() and (h[min(ch, nh):] == SENTINEL).all(), (label, cd, ch)


PATTERNS = ("none", "all", "every second", "only the first", "only the last")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 600])
def test_device_lists_equal_the_host_lists(n):
    """Unit counts around a wave and a workgroup of k_halo_lists; the dirty units first, last, interleaved or everywhere in the pool."""
    keys = unit_line(n)
    for pattern in PATTERNS if n else PATTERNS[:1]:
        pick = {"none": keys[:0], "all": keys, "every second": keys[::2], "only the first": keys[:1], "only the last": keys[-1:]}[pattern]
        if pattern == "all":  # unpack stamps what it creates
            vol = holding(ps_state_of_zero_units(keys), max_blocks=2048)
        else:
            vol = volume(2048)
            plant_empty(vol, keys)  # pool order = the order of `keys`
            if len(pick):
                stamp(vol, pick)
        assert vol.num_blocks() == n
        check_lists(vol, pick, keys, (n, pattern))
        vol.mark_merged()
        check_lists(vol, keys[:0], keys, (n, pattern, "merged"))


def ps_state_of_zero_units(keys):
    return PR.state_of_planted(ps.empty_units(keys))


def test_device_lists_after_a_prune_of_dirty_units():
    keys = unit_line(130)
    gone, stay = keys[::3], np.concatenate([keys[1::3], keys[2::3]])
    vol = holding(ps_state_of_zero_units(gone), max_blocks=1024)  # dirty and empty
    plant_empty(vol, stay)
    stamp(vol, stay[::2])  # dirty, with a voxel each
    check_lists(vol, np.concatenate([gone, stay[::2]]), keys, "before")
    stats = vol.prune(empty=True)
    assert vol.num_blocks() == len(stay[::2]) and stats is not None
    check_lists(vol, stay[::2], stay[::2], "after")


# ---- c. pack and unpack, bit for bit ---------------------------------------------------------------------------------------------
def plan_with_actions(vol, keys, actions):
    """A stored plan that lists `keys` (in range, distinct) with the given actions (1 or 2): this volume plays rank 1 of 3 - a key it
    keeps is held by ranks 1 and 2, a key it zeroes by ranks 0 and 1; all are dirty on rank 1.  -> the plan as fetched."""
    import torch

    keys, actions = np.asarray(keys, np.int64).reshape(-1, 3), np.asarray(actions)
    assert set(actions.tolist()) <= {1, 2}
    held = [keys[actions == 2], keys, keys[actions == 1]]
    dirty = [keys[:0], keys, keys[:0]]
    case = types.SimpleNamespace(world=3, dirty=dirty, held=held, dirty_counts=np.array([len(x) for x in dirty], np.int64),
                                 held_counts=np.array([len(x) for x in held], np.int64))
    da, dc, ha, hc = EC.padded(case)
    da, ha = cuda(da), cuda(ha)
    torch.cuda.synchronize()
    assert vol.halo_plan_device(da, dc, ha, hc, 3, 1) == len(keys)
    pk, pa = vol.halo_plan_fetch()
    want = {tuple(k): int(a) for k, a in zip(keys.tolist(), actions.tolist())}
    assert {tuple(k): int(a) for k, a in zip(pk.tolist(), pa.tolist())} == want
    return pk, pa


@pytest.mark.parametrize("world", EC.WORLDS)
def test_export_and_planned_pack_equal_the_restated_payload(world):
    import torch

    case = EC.unit_case(world)
    for r, state in enumerate(case.states):
        vol = holding(state)
        assert_state(vol, state, ("planted", r))  # unpack is bit exact: the volume holds what was planted
        want = ER.export_payload(state, case.export_keys)
        got = vol.export_numerators(case.export_keys)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), r
        on_device = torch.full(want.shape, 7.0, dtype=torch.float32, device="cuda")
        vol.export_numerators(case.export_keys, out=on_device)
        assert np.array_equal(bits(on_device.cpu().numpy()), bits(want)), r
        # the planned form: the in-range keys of the list (absent ones among them), in the plan's packed order
        keys = case.keys[ER.in_range(case.keys)]
        pk, _ = plan_with_actions(vol, keys, 1 + np.arange(len(keys)) % 2)
        packed = torch.full((len(pk), NV, 5), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        vol.halo_pack_planned(0, len(pk), packed)
        vol.synchronize()
        assert np.array_equal(bits(packed.cpu().numpy()), bits(ER.export_payload(state, pk))), r
        assert_state(vol, state, ("only read", r))


@pytest.mark.parametrize("world", EC.WORLDS)
def test_halo_unpack_and_import_equal_the_restatement(world):
    """Actions 0, 1 and 2 on held and absent units, an out-of-range key, a reduced weight of 0 under a numerator that is not; host and
    device payloads; import creates what unpack leaves alone."""
    case = EC.unit_case(world)
    total = case.reduced()
    total_d = cuda(total)
    for r, state in enumerate(case.states):
        want = ER.halo_unpack(state, case.keys, total, case.actions[r])
        assert ER.same_state(want, state) is not None
        for payload in (total, total_d):
            vol = holding(state)
            vol.halo_unpack(case.keys, payload, case.actions[r])
            assert vol.num_blocks() == len(state[0])
            assert_state(vol, want, ("halo_unpack", r, type(payload).__name__))
        for payload in (total, total_d):
            vol = holding(state)
            vol.import_numerators(case.keys, payload)
            have = {tuple(k) for k in state[0].tolist()}
            assert vol.num_blocks() == len(state[0]) + sum(1 for k in case.keys.tolist() if tuple(k) not in have and tuple(k) != EC.OUT_OF_RANGE)
            assert_state(vol, ER.import_units(state, case.keys, total), ("import", r, type(payload).__name__))


def test_import_numerators_is_the_loading_hook_the_planted_tests_trust():
    """tests/planted_states.py::plant on an empty volume: the dump is as_dump(states), and the state the restatement's import gives."""
    states = ps.random_units(np.array(EC.POOL_KEYS[:6], np.int64), 3, unobserved=0.3)
    vol = ps.plant(volume(), states)
    for got, want in zip(vol.dump(), ps.as_dump(states)):
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).astype(got.dtype).view(np.uint8))
    assert_state(vol, PR.state_of_planted(states), "plant")
    assert len(vol.dirty_keys()) == 0  # import stamps nothing


@pytest.fixture(scope="module")
def five():
    """Rank 0 of the three-rank unit case, five plan keys (the third one absent) with actions 1, 2, 1, 2, 1, and a payload that
    differs from what the units hold."""
    state = EC.unit_case(3).states[0]
    held = state[0][:4].astype(np.int64)
    keys = np.concatenate([held[:2], np.array([EC.ABSENT_KEYS[1]], np.int64), held[2:4]])
    payload = ER.export_payload(state, keys)
    payload[..., 0] = payload[..., 0] + np.float32(0.125) * payload[..., 1]
    payload[..., 1:] = payload[..., 1:] * np.float32(2)
    payload[2] = ER.export_payload(state, held[:1])[0]  # (numerators for the absent unit: they must go nowhere)
    return state, keys, np.array([1, 2, 1, 2, 1]), payload


def test_planned_unpack_takes_exactly_its_range(five):
    """Every (first, count) of a plan of five units, each on a fresh copy: the units of the range as the restatement leaves them -
    payload row j of the call with plan row first + j and ITS action - and every other unit as before."""
    state, keys, actions, payload = five
    by_key = {tuple(k): i for i, k in enumerate(keys.tolist())}
    for first in range(6):
        for count in range(6 - first):
            vol = holding(state)
            pk, pa = plan_with_actions(vol, keys, actions)
            order = [by_key[tuple(k)] for k in pk.tolist()]  # plan row -> row of `keys`
            part = order[first:first + count]
            sent = cuda(payload[part]) if count else cuda(payload[:1])
            vol.halo_unpack_planned(first, count, sent)
            vol.synchronize()
            want = ER.halo_unpack(state, keys[part], payload[part], actions[part])
            assert_state(vol, want, (first, count))
            assert vol.num_blocks() == len(state[0])
            outside = [tuple(k) for i, k in enumerate(keys.tolist()) if i not in part]
            got = PR.state_of_volume(vol)
            for k in outside:
                u, w = (got[0] == np.array(k)).all(1), (state[0] == np.array(k)).all(1)
                assert all(np.array_equal(got[p][u], state[p][w]) for p in range(1, 4)), (first, count, k)


def test_planned_ranges_outside_the_plan_are_refused_and_write_nothing(five):
    import torch

    from pyslam_amd._lib import HipVolError

    state, keys, actions, payload = five
    vol = holding(state)
    plan_with_actions(vol, keys, actions)
    sent = cuda(payload)
    out = torch.full((6, NV, 5), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for first, count in ((0, 6), (5, 1), (3, 3), (-1, 2), (0, -1), (2, -2), (6, 0)):
        with pytest.raises(HipVolError, match="range outside the plan"):
            vol.halo_unpack_planned(first, count, sent)
        with pytest.raises(HipVolError, match="range outside the plan"):
            vol.halo_pack_planned(first, count, out)
    vol.synchronize()
    assert (out.cpu().numpy() == 7.0).all()
    assert_state(vol, state, "refused")


# ---- d. whole merge windows ------------------------------------------------------------------------------------------------------
def host_plan(dirty, held, world, rank):
    """hv_merge_halo_plan_held (host-only C) on per-rank key lists."""
    from pyslam_amd import _lib as L

    lib = L.load()
    as_i32 = lambda lists: np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32).reshape(-1, 3) for x in lists]))
    dk, hk = as_i32(dirty), as_i32(held)
    dc, hc = np.array([len(x) for x in dirty], np.int64), np.array([len(x) for x in held], np.int64)
    n = ctypes.c_int64()
    L.check(lib.hv_merge_halo_plan_held(L.ptr(dk), L.ptr(dc), L.ptr(hk), L.ptr(hc), world, rank, None, None, 0, ctypes.byref(n)))
    shared, action = np.zeros((n.value, 3), np.int32), np.zeros(n.value, np.uint8)
    if n.value:
        L.check(lib.hv_merge_halo_plan_held(L.ptr(dk), L.ptr(dc), L.ptr(hk), L.ptr(hc), world, rank, L.ptr(shared), L.ptr(action), n.value, ctypes.byref(n)))
    return shared, action


def merge_on_the_host_path(ranks):
    world = len(ranks)
    dirty = [v.dirty_keys().reshape(-1, 3) for v in ranks]
    held = [v.unit_keys().reshape(-1, 3) for v in ranks]
    plans = [host_plan(dirty, held, world, r) for r in range(world)]
    shared = plans[0][0]
    total = ER.reduce_payloads([v.export_numerators(shared) for v in ranks])
    for v, (k, a) in zip(ranks, plans):
        assert np.array_equal(k, shared)
        v.halo_unpack(k, total, a)
        v.mark_merged()
    return plans


def merge_on_the_device_path(ranks):
    import torch

    world = len(ranks)
    lists = []
    for v in ranks:
        cap = max(v.num_blocks(), 1)
        d, h = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda")
        nd, nh = v.halo_lists_device(d, h)
        lists.append((d[:nd].clone(), h[:nh].clone()))
    dc, hc = np.array([len(a) for a, _ in lists], np.int64), np.array([len(b) for _, b in lists], np.int64)
    # the all-gather: rows of the longest list + 3 words, the padding filled with rank 0's held keys where it has any
    fill = lists[0][1][:1] if len(lists[0][1]) else torch.zeros(1, dtype=torch.int64, device="cuda")
    da, ha = fill.repeat(world, int(dc.max()) + 3), fill.repeat(world, int(hc.max()) + 3)
    for r, (a, b) in enumerate(lists):
        da[r, :len(a)] = a
        ha[r, :len(b)] = b
    torch.cuda.synchronize()
    plans, payloads = [], []
    for r, v in enumerate(ranks):
        k = v.halo_plan_device(da, dc, ha, hc, world, r)
        plans.append(v.halo_plan_fetch())
        p = torch.empty((max(k, 1), NV, 5), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        v.halo_pack_planned(0, k, p)
        v.synchronize()
        payloads.append(p[:k])
    total = payloads[0].clone()
    for p in payloads[1:]:
        total += p
    torch.cuda.synchronize()
    k = len(total)
    for v in ranks:
        cut = k // 3  # two buckets
        v.halo_unpack_planned(0, cut, total[:max(cut, 1)].contiguous())
        v.halo_unpack_planned(cut, k - cut, total[cut:].contiguous() if k - cut else total[:1].contiguous())
        v.synchronize()
        v.mark_merged()
    return plans


@pytest.mark.parametrize("world", EC.WORLDS)
def test_two_merge_windows_on_both_paths_equal_the_restatement_and_keep_the_invariant(world):
    host_ranks, dev_ranks = [volume() for _ in range(world)], [volume() for _ in range(world)]
    held_so_far = [set() for _ in range(world)]
    shared_by_window = []
    for window in (0, 1):
        written = EC.window_units(world, window)
        for r, states in EC.window_states(world, window).items():
            for vol in (host_ranks[r], dev_ranks[r]):
                if window == 0:
                    vol.unpack(EC.state_buffer(PR.state_of_planted(states)))  # stamps what it creates
                else:
                    vol.integrate_volume(ps.plant(volume(), states))          # stamps what it updates
        for r in range(world):
            held_so_far[r] |= {tuple(k) for k in written[r].tolist()}
        before = [PR.state_of_volume(v) for v in host_ranks]
        if window == 0:  # unpack is bit exact: the ranks hold what was planted
            for r, states in EC.window_states(world, 0).items():
                assert ER.same_state(before[r], PR.state_of_planted(states)) is None
        for a, v in zip(before, dev_ranks):
            assert_state(v, a, "the two sets of ranks start the window alike")
        for r in range(world):
            assert {tuple(k) for k in before[r][0].tolist()} == held_so_far[r]
            assert {tuple(k) for k in host_ranks[r].dirty_keys().tolist()} == {tuple(k) for k in written[r].tolist()}
        # the restatement on the planted lists and on the states read back before the merge
        dirty, held = [written[r] for r in range(world)], [np.array(sorted(h), np.int64).reshape(-1, 3) for h in held_so_far]
        want_xyz = [ER.plan_held(dirty, held, world, r, order="xyz") for r in range(world)]
        want_packed = [ER.plan_held(dirty, held, world, r, order="packed") for r in range(world)]
        shared = want_xyz[0][0]
        shared_by_window.append({tuple(k) for k in shared.tolist()})
        reduced = ER.reduce_payloads([ER.export_payload(s, shared) for s in before])
        want = [ER.halo_unpack(s, shared, reduced, want_xyz[r][1]) for r, s in enumerate(before)]
        host_plans, dev_plans = merge_on_the_host_path(host_ranks), merge_on_the_device_path(dev_ranks)
        for r in range(world):
            assert rows(*host_plans[r]) == rows(*want_xyz[r]) and rows(*dev_plans[r]) == rows(*want_packed[r]), (window, r)
            assert_state(host_ranks[r], want[r], ("host path", window, r))
            assert_state(dev_ranks[r], want[r], ("device path", window, r))
            assert len(host_ranks[r].dirty_keys()) == 0 and len(dev_ranks[r].dirty_keys()) == 0
        # the invariant: a merged unit is complete on exactly one rank and all zero on the others; the ranks' numerators still add
        # up to what they added up to before (weights and colour sums exactly; tsdf * w went through a product, a quotient and a
        # product again)
        assert len(shared) > 0 and {1, 2} <= {int(a) for p in want_xyz for a in p[1]}
        after = [ER.export_payload(PR.state_of_volume(v), shared) for v in dev_ranks]
        filled = sum((p != 0).any(axis=(1, 2)).astype(np.int64) for p in after)
        assert (filled == 1).all(), filled
        total = ER.reduce_payloads(after)
        assert np.array_equal(total[..., 1:], reduced[..., 1:])
        assert (np.abs(total[..., 0].astype(np.float64) - reduced[..., 0]) <= 3 * 2.0 ** -24 * np.abs(reduced[..., 0].astype(np.float64))).all()
        all_keys = np.array(sorted(set().union(*held_so_far)), np.int64)
        every_before = ER.reduce_payloads([ER.export_payload(s, all_keys) for s in before])
        every_after = ER.reduce_payloads([v.export_numerators(all_keys) for v in dev_ranks])
        assert np.array_equal(every_after[..., 1:], every_before[..., 1:])
    # the second window had units merged before and units only one rank wrote
    second = {tuple(k) for r in range(world) for k in EC.window_units(world, 1)[r].tolist()}
    assert shared_by_window[0] & shared_by_window[1] and second - shared_by_window[1]


# ---- e. warm caches --------------------------------------------------------------------------------------------------------------
WARM_CAMERA = np.array([-9.0, -13.0, 32.0]) / 64.0  # above the planted sphere (planted_states.sphere_and_plane), looking along -z


def _readers(vol, dump):
    from pyslam_amd.volumetric import PinholeCameraIntrinsic

    K = PinholeCameraIntrinsic(ps.W, ps.H, *ps.INTR)
    out = {"ray_cast " + name: a for name, a in vol.ray_cast(K, ps.camera_pose(2, -1, camera=WARM_CAMERA), 0.05, 2.0, weight_threshold=0.0).items()}
    res = vol.sample_points(lc.sample_positions(dump, 500), color=True)
    out.update({"sample " + name: getattr(res, name) for name in ("sdf", "gradient", "color", "weight", "status")})
    return out


@functools.lru_cache(maxsize=None)
def warm_source():
    """A sphere and a plane over a cluster of units (shared: only read)."""
    return ps.sparse_source(1, special=False)


def _warm(vol, dump):
    vol.extract_triangle_mesh()
    vol.extract_point_cloud(normals=True)
    vol.extract_triangle_mesh(dtype=np.float32)
    return _readers(vol, dump)


@pytest.mark.parametrize("writer", ["halo_unpack", "halo_unpack_planned", "import_numerators"])
def test_readers_with_warm_caches_see_what_an_exchange_writer_wrote(writer):
    """The three writers that change voxels without stamping a unit: extraction (mesh, point cloud with normals, float32 mesh), ray
    cast and samples afterwards equal those of a fresh twin that holds the same map."""
    vol = ps.plant(volume(), warm_source())
    dump = vol.dump()
    cold = _warm(vol, dump)
    keys = dump[0]
    actions = np.arange(len(keys)) % 3  # 0: left alone, 1: replaced (the surface moves), 2: zeroed
    assert len(keys) >= 9
    pick = actions != 0 if writer != "import_numerators" else actions == 1
    keys, actions = np.ascontiguousarray(keys[pick]), actions[pick]
    if writer == "halo_unpack_planned":
        keys, actions = plan_with_actions(vol, keys, actions)
    payload = vol.export_numerators(keys)
    payload[..., 0] = payload[..., 0] + np.float32(0.25) * payload[..., 1]
    if writer == "halo_unpack":
        vol.halo_unpack(keys, payload, actions.astype(np.uint8))
    elif writer == "import_numerators":
        vol.import_numerators(keys, payload)
    else:
        vol.halo_unpack_planned(0, len(keys), cuda(payload))
        vol.synchronize()
    assert not np.array_equal(vol.dump()[1], dump[1])
    twin = twin_of(vol)
    same(vol, twin)
    same_normals(vol, twin)
    same_mesh32(vol, twin)
    warm, fresh = _readers(vol, dump), _readers(twin, dump)
    changed = 0
    for name in warm:
        x, y = np.asarray(warm[name]), np.asarray(fresh[name])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), name
        changed += not np.array_equal(np.asarray(cold[name]), x, equal_nan=True) if x.dtype.kind == "f" else not np.array_equal(np.asarray(cold[name]), x)
    assert changed > 0 and warm["ray_cast mask"].any() and cold["ray_cast mask"].any() and (warm["sample weight"] > 0).any()


# ---- f. the pair exchange --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 1], ids=["voting", "probabilistic"])
def staged(request):
    """A grid that holds a few voxels behind the camera; one vote of blank images opens the staged interface."""
    from tests import semantic_planted as sp
    from tests.test_gpu_semantic_planted import GpuGrid

    gpu = GpuGrid(request.param, 8, max_blocks=64, max_points=1 << 12)
    pts = np.array([[0.03, 0.03, -1.0], [0.6, -0.4, -1.5], [-0.7, 0.2, -2.0]])
    gpu.integrate(pts, np.full((3, 3), 0.5, np.float32), np.array([3, 3, 4], np.int32), np.array([2, 2, -1], np.int32), None)
    cls_img, inst_img = sp.images(-1, -1)
    assert gpu.g.assoc_vote(gpu.frustum(sp.INTR, sp.W, sp.H, sp.IDENTITY, 4.0, 0.25), cls_img, inst_img)
    keys, counts = gpu.g.assoc_pairs()
    assert len(keys) == 0 and gpu.num_blocks() > 0
    return gpu


def export_rows(gpu, lists, cap):
    """One grid plays every rank in turn: rank r's pairs are set, then exported into row r of a SENTINEL-filled device buffer."""
    import torch

    msgs = torch.full((len(lists), 1 + 2 * cap), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for r, lst in enumerate(lists):
        gpu.g.assoc_set_pairs(*pack_pairs(lst))
        gpu.g.assoc_pairs_export(msgs[r])
        torch.cuda.synchronize()
    return msgs


def imported(gpu, msgs, world):
    import torch

    gpu.g.assoc_pairs_import(msgs, world)
    torch.cuda.synchronize()
    keys, counts = gpu.g.assoc_pairs()
    return sorted(zip(keys.tolist(), counts.tolist()))


def decided(gpu, ratio, min_votes, next_id):
    from pyslam_amd.volumetric_semantic import get_next_object_id_peek, set_next_object_id

    set_next_object_id(next_id)
    m = dict(gpu.g.assoc_decide(ratio, min_votes))
    return m, get_next_object_id_peek()


@pytest.mark.parametrize("name", [c.name for c in EC.pair_cases()])
def test_pair_messages_and_their_merge_equal_the_restatement(staged, name):
    case = next(c for c in EC.pair_cases() if c.name == name)
    rows_ = export_rows(staged, case.lists, case.cap).cpu().numpy()
    want_rows = np.stack([ER.message(*pack_pairs(lst), case.cap, SENTINEL) for lst in case.lists])
    assert np.array_equal(rows_, want_rows)  # n, the pairs in the order they were set, and the untouched tail
    # the hand-built messages of the case: the same pairs over garbage tails, with the counts it edits
    msgs = case.messages()
    assert np.array_equal(np.where(msgs == np.int64(EC.GARBAGE), SENTINEL, msgs)[:, 1:], want_rows[:, 1:])
    merged = case.merged()
    assert imported(staged, cuda(msgs), case.world) == merged
    for ratio, min_votes, next_id in ((0.5, 1, 40), (2.0 / 3.0, 3, 7)):
        assert imported(staged, cuda(msgs), case.world) == merged  # (decide consumed nothing, but every decision starts from an import)
        assert decided(staged, ratio, min_votes, next_id) == decide(ER.as_pairs(merged), ratio, min_votes, next_id), (name, ratio, min_votes)


def test_more_pairs_than_the_message_holds_are_reported_like_too_many_pairs(staged):
    """hv_assoc_pairs_export with n above cap sends the first cap pairs and raises the flag of the association: the map fetch after
    the decide stage reports it, as the single-GPU flow reports a keyframe with more than 4096 pairs - once."""
    from pyslam_amd._lib import HipVolError

    lst = [(5 + j, 2 * j, 1 + j) for j in range(10)]
    rows_ = export_rows(staged, [lst], 5).cpu().numpy()
    assert np.array_equal(rows_[0], ER.message(*(a[:5] for a in pack_pairs(lst)), 5, SENTINEL))
    with pytest.raises(HipVolError, match=r"more than 4096 \(instance, object\) pairs in one keyframe"):
        decided(staged, 0.5, 1, 30)
    staged.g.assoc_set_pairs(*pack_pairs([(4, 2, 1)]))
    assert decided(staged, 0.5, 1, 50) == ({4: 2}, 50)  # reported once; the stage is usable


def test_a_merged_list_above_4096_pairs_is_reported_by_the_rules_stage_and_changes_nothing(staged):
    from pyslam_amd._lib import HipVolError
    from pyslam_amd.volumetric_semantic import get_next_object_id_peek

    lists = EC.overflow_lists()
    before = staged.dump2()
    msgs = export_rows(staged, lists, 4096)
    assert msgs[:, 0].tolist() == [3000, 3000]
    staged.g.assoc_pairs_import(msgs, 2)
    with pytest.raises(HipVolError, match=r"more than 4096 \(instance, object\) pairs in one keyframe"):
        decided(staged, 0.5, 1, 60)
    assert get_next_object_id_peek() == 60
    for a, b in zip(before, staged.dump2()):
        assert np.array_equal(a, b)
    staged.g.assoc_set_pairs(*pack_pairs([(4, 2, 1)]))
    assert decided(staged, 0.5, 1, 60) == ({4: 2}, 60)
