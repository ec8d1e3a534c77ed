"""The multi-GPU exchange of include/hipvol.h ("Multi-GPU merge support", "halo merge", and the message layout of
hv_assoc_pairs_export / _import), restated in numpy - test infrastructure, no GPU, no library.  Written from the header's text, with
dictionaries and sets where the library sorts: it shares no method with hv_halo.hip or hv_semantic_ops.hip.

KEYS      a unit key (x, y, z), each in [-2^20, 2^20), packs into one 64-bit word: 21 bits per axis, bias 2^20, x lowest.  Packed
          order is therefore (z, y, x) order, not (x, y, z) order.
PLAN      plan_held(): a key is SHARED when some rank lists it dirty and two ranks or more hold it; the lowest holding rank gets
          action 1 (keep), every other rank action 2 (zero its copy; a no-op where it has none).  all_dirty_kept: every dirty key
          is shared, with action 1.  The host function lists the shared keys in (x, y, z) order, the device plan in packed order.
STATES    (keys [U,3] int32, tsdf_bits [U,4096] uint32, weight [U,4096] uint32, sums [U,4096,3] uint32) in the library's word
          order k = z * 256 + x * 16 + y: the state of tests/pack_reference.py.
PAYLOAD   export_payload(): [K, 4096, 5] float32 {f32(tsdf) * f32(w), w, sum_r, sum_g, sum_b}, each one float32 operation; zeros
          for an absent or out-of-range key.  halo_unpack() / import_units(): tsdf = N / W in float32 where W > 0, else 0;
          w = uint32(W); colour sums = uint32 of the payload; action 2 zeroes all five planes, action 0 changes nothing; an absent
          unit is untouched by halo_unpack and created by import_units.
PAIRS     merge_pairs(): messages [world, 1 + 2 cap] int64 = [n, keys[cap], votes[cap]]; n is clamped to [0, cap]; votes of equal
          keys are added; the result is a multiset (the device order is unspecified).

Every function takes variant=<name>: the WRONG readings of the contract listed in PLAN_VARIANTS, UNPACK_VARIANTS and
PAIR_VARIANTS.  tests/test_exchange_reference_cpu.py proves that the planted cases of tests/exchange_cases.py tell each of them
from the right reading.
"""
import numpy as np

KEY_BITS = 21
KEY_BIAS = 1 << 20
KEY_MASK = (1 << KEY_BITS) - 1
NV = 4096
F32 = np.float32

PLAN_VARIANTS = ("keeper_lowest_dirty", "keeper_highest_holder", "holders_ge_1", "any_dirty_ignored", "padding_read", "xyz_order")
UNPACK_VARIANTS = ("action2_leaves", "action0_as_2", "no_weight_guard", "colour_uint8", "absent_claimed")
PAIR_VARIANTS = ("votes_max", "n_not_clamped", "rank0_offset")


# ---- keys ----------------------------------------------------------------------------------------------------------------------
def in_range(keys):
    k = np.asarray(keys, np.int64).reshape(-1, 3)
    return ((k >= -KEY_BIAS) & (k < KEY_BIAS)).all(axis=1)


def pack_key(keys):
    """[n,3] integers in [-2^20, 2^20) -> [n] uint64."""
    k = np.asarray(keys, np.int64).reshape(-1, 3)
    assert in_range(k).all()
    u = (k + KEY_BIAS).astype(np.uint64)
    return u[:, 0] | (u[:, 1] << np.uint64(KEY_BITS)) | (u[:, 2] << np.uint64(2 * KEY_BITS))


def unpack_key(packed):
    """[n] uint64 (or int64 holding the same bits) -> [n,3] int32."""
    p = np.asarray(packed).astype(np.uint64).reshape(-1)
    cols = [((p >> np.uint64(s)) & np.uint64(KEY_MASK)).astype(np.int64) - KEY_BIAS for s in (0, KEY_BITS, 2 * KEY_BITS)]
    return np.stack(cols, axis=1).astype(np.int32)


def _tuples(keys):
    return [tuple(int(v) for v in k) for k in np.asarray(keys, np.int64).reshape(-1, 3)]


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def plan_held(dirty_lists, held_lists, world, rank, all_dirty_kept=False, order="packed", variant=None):
    """dirty_lists / held_lists: per rank a [n,3] key array.  -> (shared_keys [n,3] int32, action [n] uint8)."""
    assert order in ("packed", "xyz") and len(dirty_lists) == len(held_lists) == world and 0 <= rank < world
    assert variant is None or variant in PLAN_VARIANTS, variant
    dirty_by, holders = {}, {}
    for r in range(world):
        for k in _tuples(dirty_lists[r]):
            dirty_by.setdefault(k, set()).add(r)
        for k in _tuples(held_lists[r]):
            holders.setdefault(k, set()).add(r)
    if variant == "xyz_order":
        order = "xyz"
    every = set(dirty_by) | set(holders)
    listed = sorted(every, key=(lambda k: (k[2], k[1], k[0])) if order == "packed" else None)
    keys, action = [], []
    for k in listed:
        dirty, held = k in dirty_by, holders.get(k, set())
        if all_dirty_kept:
            if dirty:
                keys.append(k)
                action.append(1)
            continue
        if variant == "any_dirty_ignored":
            dirty = True
        if not dirty or len(held) < (1 if variant == "holders_ge_1" else 2):
            continue
        keeper = min(held)
        if variant == "keeper_highest_holder":
            keeper = max(held)
        elif variant == "keeper_lowest_dirty" and k in dirty_by:
            keeper = min(dirty_by[k])
        keys.append(k)
        action.append(1 if keeper == rank else 2)
    return np.array(keys, np.int32).reshape(-1, 3), np.array(action, np.uint8)


def lists_of_padded(padded, counts, variant=None):
    """The gathered form [world, stride] of packed keys with the per-rank counts -> the ranks' [n,3] lists.  Rank r's list is the
    first counts[r] words of row r, whatever the padding holds."""
    padded, counts = np.asarray(padded), np.asarray(counts, np.int64)
    assert padded.ndim == 2 and len(counts) == padded.shape[0] and (counts >= 0).all() and (counts <= padded.shape[1]).all()
    if variant == "padding_read":  # the stride ignored: the rows taken as lying back to back at the counts' prefixes
        flat, at, out = padded.reshape(-1), 0, []
        for c in counts:
            out.append(unpack_key(flat[at:at + int(c)]))
            at += int(c)
        return out
    return [unpack_key(padded[r, :int(c)]) for r, c in enumerate(counts)]


def plan_held_padded(dirty_all, dirty_counts, held_all, held_counts, world, rank, all_dirty_kept=False, order="packed", variant=None):
    """plan_held on the gathered, padded lists hv_merge_halo_plan_device takes."""
    dl, hl = lists_of_padded(dirty_all, dirty_counts, variant), lists_of_padded(held_all, held_counts, variant)
    return plan_held(dl, hl, world, rank, all_dirty_kept, order, None if variant == "padding_read" else variant)


# ---- pack and unpack -----------------------------------------------------------------------------------------------------------
def _index(state):
    return {k: i for i, k in enumerate(_tuples(state[0]))}


def export_payload(state, keys):
    """-> [K, 4096, 5] float32; a key may repeat."""
    skeys, bits, weight, sums = state
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    at = _index(state)
    out = np.zeros((len(keys), NV, 5), F32)
    ok = in_range(keys)
    for i, k in enumerate(_tuples(keys)):
        u = at.get(k) if ok[i] else None
        if u is None:
            continue
        w = np.asarray(weight[u], np.uint32).astype(F32)
        out[i, :, 0] = np.asarray(bits[u], np.uint32).view(F32) * w
        out[i, :, 1] = w
        out[i, :, 2:5] = np.asarray(sums[u], np.uint32).astype(F32)
    return out


def _copy(state):
    return tuple(np.array(a, copy=True) for a in state)


def _write(planes, u, row, variant):
    """The reduced numerators `row` [4096, 5] into unit u."""
    bits, weight, sums = planes
    N, W = np.asarray(row[:, 0], F32), np.asarray(row[:, 1], F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (N / W).astype(F32)
    t = q if variant == "no_weight_guard" else np.where(W > 0, q, F32(0))
    bits[u] = t.astype(F32).view(np.uint32)
    weight[u] = W.astype(np.int64).astype(np.uint32)
    c = np.asarray(row[:, 2:5], F32).astype(np.int64)
    sums[u] = (c.astype(np.uint8) if variant == "colour_uint8" else c).astype(np.uint32)


def _with_units(state, new_keys):
    keys, bits, weight, sums = state
    n = len(new_keys)
    return (np.concatenate([keys, np.array(new_keys, np.int32).reshape(n, 3)]), np.concatenate([bits, np.zeros((n, NV), np.uint32)]),
            np.concatenate([weight, np.zeros((n, NV), np.uint32)]), np.concatenate([sums, np.zeros((n, NV, 3), np.uint32)]))


def halo_unpack(state, keys, payload, action, variant=None):
    """-> the state afterwards (units in the order of `state`; no key of `keys` may repeat)."""
    assert variant is None or variant in UNPACK_VARIANTS, variant
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    action = np.asarray(action, np.uint8)
    assert len(action) == len(keys) and len(set(_tuples(keys))) == len(keys)
    out = _copy(state)
    ok = in_range(keys)
    if variant == "absent_claimed":
        have = _index(out)
        out = _with_units(out, [k for i, k in enumerate(_tuples(keys)) if ok[i] and action[i] != 0 and k not in have])
    at = _index(out)
    for i, k in enumerate(_tuples(keys)):
        a = int(action[i])
        if variant == "action0_as_2" and a == 0:
            a = 2
        u = at.get(k) if ok[i] else None
        if u is None or a == 0:
            continue
        if a == 1:
            _write(out[1:], u, payload[i], variant)
        elif variant != "action2_leaves":
            out[1][u], out[2][u], out[3][u] = 0, 0, 0
    return out


def import_units(state, keys, payload, variant=None):
    """-> the state afterwards: units the state lacks are appended in the order of their first mention; out-of-range keys are
    dropped; no key may repeat."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    assert len(set(_tuples(keys))) == len(keys)
    ok = in_range(keys)
    have = _index(state)
    out = _with_units(_copy(state), [k for i, k in enumerate(_tuples(keys)) if ok[i] and k not in have])
    at = _index(out)
    for i, k in enumerate(_tuples(keys)):
        if ok[i]:
            _write(out[1:], at[k], payload[i], variant)
    return out


def sorted_state(state):
    """The units in (x, y, z) key order, as dump() lists them."""
    keys = np.asarray(state[0], np.int64).reshape(-1, 3)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return tuple(np.asarray(a)[order] for a in state)


def same_state(a, b):
    """-> the name of the first plane in which two states differ (units in any order), or None."""
    a, b = sorted_state(a), sorted_state(b)
    for name, x, y in zip(("keys", "tsdf bits", "weight", "colour sums"), a, b):
        x, y = np.asarray(x), np.asarray(y)
        if x.shape != y.shape or not np.array_equal(x.astype(np.int64), y.astype(np.int64)):
            return name
    return None


def reduce_payloads(payloads):
    """The all-reduce: float32 additions in rank order."""
    total = np.array(payloads[0], F32, copy=True)
    for p in payloads[1:]:
        total = (total + np.asarray(p, F32)).astype(F32)
    return total


def quotient_bound(states, keys, world):
    """For the units `keys` over the ranks' states: (|float32 restatement of N / W - float64 quotient of the exact sums|, the bound
    (world + 1) * 2^-24 * sum_r |t_r| w_r / W with a 1 % allowance for second-order terms) - one rounding per product, world - 1
    per sum, one for the division.  Both [K, 4096], where W > 0 (0 elsewhere)."""
    total = reduce_payloads([export_payload(s, keys) for s in states])
    exact_n, exact_w, abs_n = np.zeros(total.shape[:2]), np.zeros(total.shape[:2]), np.zeros(total.shape[:2])
    for s in states:
        at = _index(s)
        for i, k in enumerate(_tuples(keys)):
            u = at.get(k)
            if u is None:
                continue
            t, w = np.asarray(s[1][u], np.uint32).view(F32).astype(np.float64), np.asarray(s[2][u], np.float64)
            exact_n[i] += t * w
            exact_w[i] += w
            abs_n[i] += np.abs(t) * w
    seen = exact_w > 0
    np.testing.assert_array_equal(total[..., 1], exact_w)
    with np.errstate(divide="ignore", invalid="ignore"):
        got = np.where(seen, (total[..., 0] / total[..., 1]).astype(F32), F32(0)).astype(np.float64)
        err = np.where(seen, np.abs(got - exact_n / np.where(seen, exact_w, 1.0)), 0.0)
        bound = np.where(seen, 1.01 * (world + 1) * 2.0 ** -24 * abs_n / np.where(seen, exact_w, 1.0), 0.0)
    return err, bound


# ---- pair lists ----------------------------------------------------------------------------------------------------------------
def message(keys, votes, cap, fill, n=None):
    """One rank's message [1 + 2 cap] int64: n (default len(keys)), the keys, the votes; the unused tail holds `fill`."""
    keys = np.asarray(keys, np.uint64)
    assert len(keys) == len(votes) <= cap
    msg = np.full(1 + 2 * cap, fill, np.int64)
    msg[0] = len(keys) if n is None else n
    msg[1:1 + len(keys)] = keys.view(np.int64)
    msg[1 + cap:1 + cap + len(keys)] = np.asarray(votes, np.int64)
    return msg


def merge_pairs(messages, cap, variant=None):
    """messages [world, 1 + 2 cap] int64 -> sorted list of (key, votes): the multiset of the merged pairs."""
    assert variant is None or variant in PAIR_VARIANTS, variant
    messages = np.asarray(messages, np.int64)
    assert messages.ndim == 2 and messages.shape[1] == 1 + 2 * cap
    merged, flat = {}, messages.reshape(-1)
    for r in range(len(messages)):
        base = (0 if variant == "rank0_offset" else r) * (1 + 2 * cap)
        n = max(int(flat[base]), 0)
        if variant == "n_not_clamped":
            n = min(n, len(flat) - (base + 1 + cap))  # (what lies behind the message is read as pairs, to the end of the buffer)
        else:
            n = min(n, cap)
        for i in range(n):
            key, votes = int(flat[base + 1 + i]) & 0xFFFFFFFFFFFFFFFF, int(flat[base + 1 + cap + i].astype(np.int32))
            if key in merged:
                merged[key] = max(merged[key], votes) if variant == "votes_max" else merged[key] + votes
            else:
                merged[key] = votes
    return sorted(merged.items())


def as_pairs(merged):
    """[(key, votes)] -> [(instance, object, votes)] as tests/assoc_rules_reference.py takes them."""
    s32 = lambda v: v - (1 << 32) if v >= 1 << 31 else v
    return [(s32(k >> 32), s32(k & 0xFFFFFFFF), int(n)) for k, n in merged]
