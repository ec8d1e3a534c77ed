"""CPU: the numpy restatement of the multi-GPU exchange (tests/exchange_reference.py) and the planted inputs of
tests/exchange_cases.py - (a) the restated plan equals hv_merge_halo_plan_held (host-only C) on every key-list case and rank, and its
packed and (x, y, z) orders list the same (key, action) set; (b) every wrong reading of the contract (PLAN_VARIANTS,
UNPACK_VARIANTS, PAIR_VARIANTS) differs from the right one on at least one planted case - the case is printed; (c) the case families
hold what tests/test_gpu_exchange_planted.py relies on; (d) the float32 restatement of N / W is tied to the float64 quotient of the
exact sums."""
import ctypes

import numpy as np
import pytest

from tests import exchange_cases as EC
from tests import exchange_reference as ER
from tests.assoc_rules_reference import SEEN, decide

B = ER.KEY_BIAS


def host_plan(case, rank):
    """hv_merge_halo_plan_held on the case's lists, back to back."""
    from pyslam_amd import _lib as L

    lib = L.load()
    dk, hk = np.ascontiguousarray(np.concatenate(case.dirty)), np.ascontiguousarray(np.concatenate(case.held))
    n = ctypes.c_int64()
    L.check(lib.hv_merge_halo_plan_held(L.ptr(dk), L.ptr(case.dirty_counts), L.ptr(hk), L.ptr(case.held_counts), case.world, rank, None, None, 0,
                                        ctypes.byref(n)))
    shared, action = np.zeros((n.value, 3), np.int32), np.zeros(n.value, np.uint8)
    if n.value:
        L.check(lib.hv_merge_halo_plan_held(L.ptr(dk), L.ptr(case.dirty_counts), L.ptr(hk), L.ptr(case.held_counts), case.world, rank, L.ptr(shared),
                                            L.ptr(action), n.value, ctypes.byref(n)))
    return shared, action


def rows(plan):
    return [tuple(k) + (int(a),) for k, a in zip(plan[0].tolist(), plan[1].tolist())]


def test_packed_keys_round_trip_and_order_by_z_then_y_then_x():
    keys = np.array([(-B, -B, -B), (B - 1, B - 1, B - 1), (0, 0, 0), (1, 0, 0), (0, 0, 1), (-1, 2, -3), (B - 1, -B, 0)], np.int64)
    packed = ER.pack_key(keys)
    assert packed.dtype == np.uint64 and packed[0] == 0 and packed[1] == (1 << 63) - 1 and packed[2] == B | B << 21 | B << 42
    np.testing.assert_array_equal(ER.unpack_key(packed), keys)
    np.testing.assert_array_equal(ER.unpack_key(packed.view(np.int64)), keys)
    assert packed[3] < packed[4] and tuple(keys[4]) < tuple(keys[3])  # (1, 0, 0) before (0, 0, 1) packed, after it as (x, y, z)
    assert not ER.in_range([(B, 0, 0)])[0] and not ER.in_range([(0, -B - 1, 0)])[0] and ER.in_range(keys).all()


@pytest.mark.parametrize("case", EC.key_list_cases(), ids=lambda c: c.name)
def test_restated_plan_equals_the_host_plan_and_both_orders_list_the_same_set(case):
    for rank in range(case.world):
        xyz = ER.plan_held(case.dirty, case.held, case.world, rank, order="xyz")
        host = host_plan(case, rank)
        assert rows(xyz) == rows(host), (case.name, rank)
        packed = ER.plan_held(case.dirty, case.held, case.world, rank, order="packed")
        assert sorted(rows(packed)) == sorted(rows(xyz))
        assert np.array_equal(np.sort(ER.pack_key(packed[0])), ER.pack_key(packed[0]))  # ... in ascending packed order
        # the padded form gives the same lists back, whatever the padding holds
        assert rows(ER.plan_held_padded(*EC.padded(case), case.world, rank)) == rows(packed)


@pytest.mark.parametrize("case", EC.key_list_cases(), ids=lambda c: c.name)
def test_the_older_plan_is_the_held_plan_with_the_dirty_lists_as_held_lists(case):
    """hv_merge_halo_plan(keys, counts) == hv_merge_halo_plan_held(keys, counts, keys, counts), keys and actions, on every rank: a
    key listed by two ranks or more, the lowest lister keeps (a rank lists a key once in its dirty list)."""
    from pyslam_amd import _lib as L

    lib = L.load()
    dk = np.ascontiguousarray(np.concatenate(case.dirty))
    cap = len(dk) + 1
    listers = {}
    for r, d in enumerate(case.dirty):
        for k in d.tolist():
            listers.setdefault(tuple(k), []).append(r)
    assert all(len(set(v)) == len(v) for v in listers.values())
    for rank in range(case.world):
        n_old, n_held = ctypes.c_int64(), ctypes.c_int64()
        old = np.zeros((cap, 3), np.int32), np.zeros(cap, np.uint8)
        held = np.zeros((cap, 3), np.int32), np.zeros(cap, np.uint8)
        L.check(lib.hv_merge_halo_plan(L.ptr(dk), L.ptr(case.dirty_counts), case.world, rank, L.ptr(old[0]), L.ptr(old[1]), cap, ctypes.byref(n_old)))
        L.check(lib.hv_merge_halo_plan_held(L.ptr(dk), L.ptr(case.dirty_counts), L.ptr(dk), L.ptr(case.dirty_counts), case.world, rank,
                                            L.ptr(held[0]), L.ptr(held[1]), cap, ctypes.byref(n_held)))
        assert n_old.value == n_held.value and rows(old) == rows(held), (case.name, rank)
        want = [k + (1 if min(v) == rank else 2,) for k, v in sorted(listers.items()) if len(v) >= 2]
        assert rows(old)[:n_old.value] == want, (case.name, rank)


def _first_difference(right, wrong, cases, label):
    for case in cases:
        for rank in label(case):
            if right(case, rank) != wrong(case, rank):
                return case.name, rank
    return None


@pytest.mark.parametrize("variant", ER.PLAN_VARIANTS)
def test_every_wrong_plan_differs_on_a_planted_key_list(variant):
    right = lambda c, r: rows(ER.plan_held_padded(*EC.padded(c), c.world, r))
    wrong = lambda c, r: rows(ER.plan_held_padded(*EC.padded(c), c.world, r, variant=variant))
    found = _first_difference(right, wrong, EC.key_list_cases(), lambda c: c.ranks())
    print(f"plan variant {variant}: exposed by case {found}")
    assert found is not None, variant


@pytest.mark.parametrize("variant", ER.UNPACK_VARIANTS)
def test_every_wrong_unpack_differs_on_a_planted_unit_case(variant):
    found = None
    for case in EC.unit_cases():
        total = case.reduced()
        for r in range(case.world):
            a = ER.halo_unpack(case.states[r], case.keys, total, case.actions[r])
            b = ER.halo_unpack(case.states[r], case.keys, total, case.actions[r], variant=variant)
            if ER.same_state(a, b) is not None:
                found = (f"units w{case.world}", r, ER.same_state(a, b))
                break
        if found:
            break
    print(f"unpack variant {variant}: exposed by case {found}")
    assert found is not None, variant


@pytest.mark.parametrize("variant", ER.PAIR_VARIANTS)
def test_every_wrong_pair_merge_differs_on_a_planted_pair_list(variant):
    found = next((c.name for c in EC.pair_cases() if c.merged() != c.merged(variant)), None)
    print(f"pair variant {variant}: exposed by case {found}")
    assert found is not None, variant


def test_key_list_cases_hold_what_they_promise():
    cases = {c.name: c for c in EC.key_list_cases()}
    assert {c.world for c in cases.values()} == {1, 2, 3, 8, 64}
    totals = {c.total() for c in cases.values()}
    assert {0, 1, 255, 256, 257} <= totals and any(2800 <= t <= 3300 for t in totals), sorted(totals)
    empty = lambda c, r: c.dirty_counts[r] == 0 and c.held_counts[r] == 0
    busy = lambda c: c.total() > 0
    assert any(busy(c) and empty(c, 0) for c in cases.values()) and any(busy(c) and empty(c, c.world - 1) for c in cases.values())
    assert any(busy(c) and c.world >= 3 and any(empty(c, r) for r in range(1, c.world - 1)) for c in cases.values())
    assert empty(cases["w64 mixed"], 32) and 32 in cases["w64 mixed"].ranks()
    assert any(c.world > 1 and all(empty(c, r) for r in range(c.world)) for c in cases.values())
    # the rules, on the three-rank case: not shared / shared as the comments of _RULES3 say, and a plan with both actions
    c = cases["w3 rules"]
    plans = [dict((tuple(k), int(a)) for k, a in zip(*[x.tolist() for x in ER.plan_held(c.dirty, c.held, 3, r)])) for r in range(3)]
    assert set(plans[0]) == {(0, 0, 1), (2, 2, 2), (-3, 0, 1), (1, 0, -1)}
    assert [p[(0, 0, 1)] for p in plans] == [2, 1, 2] and [p[(2, 2, 2)] for p in plans] == [1, 2, 2] and [p[(1, 0, -1)] for p in plans] == [1, 2, 2]
    assert len(c.dirty[0]) and not (c.held[0] == np.array((0, 0, 1))).all(1).any() and (c.dirty[0] == np.array((0, 0, 1))).all(1).any()
    # the two orders differ on it
    assert ER.plan_held(c.dirty, c.held, 3, 0, order="xyz")[0].tolist() != ER.plan_held(c.dirty, c.held, 3, 0, order="packed")[0].tolist()
    # a rank that lists a key twice as held is one holder: no other case repeats a key within a list
    for c in cases.values():
        repeats = [len(x) - len({tuple(k) for k in x.tolist()}) for x in c.dirty + c.held]
        assert sum(repeats) == len(c.held_twice) and (c.name == "w3 held twice") == bool(c.held_twice), c.name
    c = cases["w3 held twice"]
    assert sorted(map(tuple, c.held[1].tolist())) == [(6, 1, 0), (6, 1, 0), (6, 1, 1), (6, 1, 1)] and c.held[2].tolist().count([6, 1, 1]) == 1
    assert not len(c.held[0]) and sorted(map(tuple, c.dirty[0].tolist())) == [(6, 1, 0), (6, 1, 1)]
    assert [rows(ER.plan_held(c.dirty, c.held, 3, r)) for r in range(3)] == [[(6, 1, 1, 2)], [(6, 1, 1, 1)], [(6, 1, 1, 2)]]
    # a key held by all ranks and dirty on all, its run of 2 * world entries across sorted entries 255 | 256
    for name in ("w8 straddle total 257", "w64 straddle"):
        c = cases[name]
        keys = c.sorted_entry_keys()
        run = np.flatnonzero(keys == ER.pack_key([(0, 0, 0)])[0])
        assert len(run) == 2 * c.world and run[0] <= 255 and run[-1] >= 256 and (np.diff(run) == 1).all(), (name, run[0], run[-1])
        k, a = ER.plan_held(c.dirty, c.held, c.world, 0)
        assert k.tolist() == [[0, 0, 0]] and a.tolist() == [1] and ER.plan_held(c.dirty, c.held, c.world, c.world - 1)[1].tolist() == [2]
    # both ends of the 21-bit range on every axis, shared
    k = ER.plan_held(cases["w2 rim"].dirty, cases["w2 rim"].held, 2, 0)[0]
    assert all((k[:, a] == -B).any() and (k[:, a] == B - 1).any() for a in range(3))
    # stride = longest list + 5, the padding holds live keys of other ranks that the rank itself does not list
    for c in cases.values():
        da, dc, ha, hc = EC.padded(c)
        assert da.shape == (c.world, dc.max(initial=0) + 5) and ha.shape == (c.world, hc.max(initial=0) + 5)
    c = cases["w3 rules"]
    da, dc, ha, hc = EC.padded(c)
    live = set(np.concatenate([ER.pack_key(x) for x in c.held + c.dirty]).tolist())
    assert all(set(da[r, dc[r]:].view(np.uint64).tolist()) <= live for r in range(3))
    # world 1: all_dirty_kept shares every dirty key, the plain plan none
    c = cases["w1 dirty and held"]
    assert len(ER.plan_held(c.dirty, c.held, 1, 0)[0]) == 0
    k, a = ER.plan_held(c.dirty, c.held, 1, 0, all_dirty_kept=True)
    assert len(k) == 3 and (a == 1).all()


def test_unit_cases_hold_what_they_promise():
    assert [c.world for c in EC.unit_cases()] == [2, 3, 8]
    for case in EC.unit_cases():
        held_anywhere = set()
        for keys, bits, weight, sums in case.states:
            assert 0 < len(keys) <= 24 and weight.max() <= 7 and (sums <= 255 * weight[..., None]).all()
            assert ((weight == 0) & (bits != 0)).any() and ((weight == 0) & (bits >> 31 == 1)).any()  # weight 0, tsdf bits set (some negative)
            assert ((weight > 0) & (sums == 0).all(-1)).any() and ((weight > 0) & (sums == 255 * weight[..., None]).all(-1)).any()
            assert ((weight == 0).mean(axis=1) > 0.2).any()  # the unobserved share
            held_anywhere |= {tuple(k) for k in keys.tolist()}
        # one observed voxel at the library's words 0, 1 and 4095
        keys, bits, weight, sums = case.states[0]
        lone = [np.flatnonzero(weight[u]) for u in range(len(keys)) if (weight[u] > 0).sum() == 1]
        assert {0, 1, 4095} <= {int(x[0]) for x in lone}
        total = case.reduced()
        assert total[..., 1:].max() < 2 ** 24 and (total[..., 1:] == np.rint(total[..., 1:])).all()  # exact in float32
        assert ((total[..., 1] == 0) & (total[..., 0] != 0)).sum() >= 10  # reduced weight 0, numerator not
        klist = [tuple(k) for k in case.keys.tolist()]
        assert len(set(klist)) == len(klist) and len(case.export_keys) == len(klist) + 2 and EC.OUT_OF_RANGE in klist
        assert not set(EC.ABSENT_KEYS) & held_anywhere
        for r, act in enumerate(case.actions):
            assert set(act.tolist()) == {0, 1, 2}
            mine = {tuple(k) for k in case.states[r][0].tolist()}
            assert {int(a) for k, a in zip(klist, act) if k not in mine and k != EC.OUT_OF_RANGE} == {0, 1, 2}  # absent under every action
            assert {int(a) for k, a in zip(klist, act) if k in mine} == {0, 1, 2}  # and held under every action


def test_pair_cases_hold_what_they_promise():
    cases = EC.pair_cases()
    assert {c.world for c in cases} == set(EC.PAIR_WORLDS) and {c.cap for c in cases} == set(EC.PAIR_CAPS)
    for cap in EC.PAIR_CAPS:
        assert {len(lst) for c in cases if c.cap == cap for lst in c.lists} >= {0, 1, cap - 1, cap}, cap
    assert any(len(c.merged()) == 4096 for c in cases)
    assert any(n is not None and n < 0 for c in cases for n in c.counts) and any(n is not None and n > c.cap for c in cases for n in c.counts)
    for c in cases:
        msgs = c.messages()
        assert msgs.shape == (c.world, 1 + 2 * c.cap) and msgs.dtype == np.int64
        for r, lst in enumerate(c.lists):  # garbage in every unused slot
            n = len(lst)
            assert (msgs[r, 1 + n:1 + c.cap] == np.int64(EC.GARBAGE)).all() and (msgs[r, 1 + c.cap + n:] == np.int64(EC.GARBAGE)).all()
        merged = ER.as_pairs(c.merged())
        if all((3, SEEN, 1) in lst for lst in c.lists) and all(n is None for n in c.counts):
            assert (3, SEEN, c.world) in merged  # the marker every rank lists adds up to one pair
        decide(merged, 0.5, 2, 40)  # (the rules restatement takes every merged list)
    c = next(c for c in cases if c.name == "w3 cap5 bad counts")
    own = {p[:2] for lst in c.lists for p in lst if p[0] >= 100}
    merged = {p[:2] for p in ER.as_pairs(c.merged())}
    assert {p for p in own if p[0] == 101}.isdisjoint(merged) and {p for p in own if p[0] in (100, 102)} <= merged
    assert len(ER.merge_pairs(np.stack([ER.message(*EC.pack_pairs(lst), 4096, 0) for lst in EC.overflow_lists()]), 4096)) == 6000


@pytest.mark.parametrize("world", EC.WORLDS)
def test_float32_quotient_stays_within_its_bound_of_the_float64_quotient(world):
    case = EC.unit_case(world)
    keys = case.keys[ER.in_range(case.keys)]
    err, bound = ER.quotient_bound(case.states, keys, world)
    assert (bound > 0).sum() > 10000 and (err <= bound).all(), float((err - bound).max())
    print(f"world {world}: worst error / bound = {float((err[bound > 0] / bound[bound > 0]).max()):.3f}")


def test_export_import_round_trip_in_the_restatement():
    """import_units(export_payload) gives the planted integers back and tsdf = (t * w) / w; an absent key is created, an
    out-of-range key dropped, a weight of 0 gives tsdf 0 whatever the numerator."""
    case = EC.unit_case(2)
    state = case.states[0]
    payload = ER.export_payload(state, case.export_keys)
    assert payload.shape == (len(case.export_keys), 4096, 5) and payload.dtype == np.float32
    np.testing.assert_array_equal(payload[-1], payload[0])  # the repeated key
    absent = [i for i, k in enumerate(case.keys.tolist()) if tuple(k) not in {tuple(x) for x in state[0].tolist()}]
    assert len(absent) >= 4 and not payload[absent].any()
    assert (np.signbit(payload[..., 0]) & (payload[..., 0] == 0)).any()  # -0: a negative tsdf times weight 0
    empty = tuple(a[:0] for a in state)
    back = ER.import_units(empty, case.keys, case.reduced())
    assert len(back[0]) == len(case.keys) - 1 and EC.OUT_OF_RANGE not in [tuple(k) for k in back[0].tolist()]
    assert (back[1][back[2] == 0] == 0).all()
