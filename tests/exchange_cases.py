"""Planted inputs for the multi-GPU exchange (hv_halo.hip, hv_assoc_pairs_export / _import) - test infrastructure, no GPU.  Three
families, each built once and only read:

KEY-LIST CASES (key_list_cases): per rank a dirty list and a held list of unit keys, worlds 1, 2, 3, 8 and 64, no voxel content.
  padded(case) gives the gathered form the device plan takes: [world, stride] packed keys with stride = the longest list + 5 and
  the padding filled with LIVE keys of other ranks - a reader that looks behind a rank's count finds plausible entries.  One
  case ("w3 held twice") has a rank list keys twice as held - one holder all the same; every other list is free of repeats.
UNIT STATES (unit_cases): per rank a state of tests/pack_reference.py (word order, tsdf as bit patterns) for 2, 3 and 8 ranks, at
  most 24 units per rank: random units with 30 % unobserved voxels, one-voxel units, voxels of weight 0 whose tsdf bits are not
  zero, colour sums at 0 and at 255 * w; with a key list (absent units under every action, an out-of-range key, for export a
  repeated key) and per rank an action vector that mixes 0, 1 and 2.  Planted weights are at most 7 and colours at most 255, so with
  at most 8 ranks every reduced weight and colour sum is an integer below 2^24, which float32 holds exactly; sums above 2^24 are out
  of scope of these cases (the float32 all-reduce rounds them, and what the unpack then stores is no longer defined by the
  contract's integer planes).
PAIR LISTS (pair_cases): per rank the (instance, object, votes) pairs of one keyframe, worlds 1, 2, 3 and 8, message capacities 1,
  5, 64 and 4096, per-rank counts of 0, 1, cap - 1 and cap, markers every rank lists, pairs only one rank lists, a merged list of
  exactly 4096 distinct pairs, and hand-edited counts (negative, above cap) over garbage tails.
"""
import functools

import numpy as np

from tests import exchange_reference as ER
from tests import pack_reference as PR
from tests import planted_states as ps
from tests.assoc_rules_reference import PENDING, SEEN, pack_pairs

B = ER.KEY_BIAS
NV = ps.NV


# ---- key lists -----------------------------------------------------------------------------------------------------------------
class KeyLists:
    def __init__(self, name, world, entries, seed=0, held_twice=()):
        """entries: [(key, ranks that list it dirty, ranks that hold it)]; each rank's lists come out shuffled.  held_twice:
        [(key, rank)] - the rank lists that key a second time as held; every other list is free of repeats."""
        self.name, self.world = name, world
        rng = np.random.default_rng(1000 + seed)
        self.entries = [(tuple(int(v) for v in k), tuple(sorted(d)), tuple(sorted(h))) for k, d, h in entries]
        assert len({k for k, _, _ in self.entries}) == len(self.entries)
        self.held_twice = tuple((tuple(int(v) for v in k), int(r)) for k, r in held_twice)
        assert all(any(k == e[0] and r in e[2] for e in self.entries) for k, r in self.held_twice) and len(set(self.held_twice)) == len(self.held_twice)
        self.dirty, self.held = [], []
        for r in range(world):
            d = [k for k, dr, _ in self.entries if r in dr]
            h = [k for k, _, hr in self.entries if r in hr] + [k for k, q in self.held_twice if q == r]
            self.dirty.append(np.array([d[i] for i in rng.permutation(len(d))], np.int32).reshape(-1, 3))
            self.held.append(np.array([h[i] for i in rng.permutation(len(h))], np.int32).reshape(-1, 3))
        self.dirty_counts = np.array([len(x) for x in self.dirty], np.int64)
        self.held_counts = np.array([len(x) for x in self.held], np.int64)

    def total(self):
        return int(self.dirty_counts.sum() + self.held_counts.sum())

    def ranks(self):
        """Every rank, or ranks 0, 1, middle and last of a large world."""
        return list(range(self.world)) if self.world <= 8 else [0, 1, self.world // 2, self.world - 1]

    def sorted_entry_keys(self):
        """The packed keys of all entries (dirty and held) in ascending order: the device plan's sorted array."""
        every = [ER.pack_key(x) for x in self.dirty + self.held if len(x)]
        return np.sort(np.concatenate(every)) if every else np.zeros(0, np.uint64)


def _padded(lists, world, foreign):
    """[world, longest + 5] int64: rank r's list, then copies of `foreign(r)` keys (cycled)."""
    stride = max(len(x) for x in lists) + 5
    out = np.zeros((world, stride), np.int64)
    for r, x in enumerate(lists):
        out[r, :len(x)] = ER.pack_key(x).view(np.int64)
        live = foreign(r)
        if len(live) == 0:
            live = np.array([[1, 2, 3], [-1, 0, 5]], np.int32)  # (nothing is live anywhere: still not zeros)
        fill = ER.pack_key(live).view(np.int64)
        out[r, len(x):] = fill[np.arange(stride - len(x)) % len(fill)]
    return out


def padded(case):
    """-> (dirty_all, dirty_counts, held_all, held_counts).  A rank's dirty padding holds what OTHER ranks hold, its held padding
    what other ranks hold or list dirty: read as entries, they would add holders and dirty marks."""
    others = lambda r: np.concatenate([case.held[q] for q in range(case.world) if q != r] + [case.dirty[q] for q in range(case.world) if q != r]
                                      + [np.zeros((0, 3), np.int32)])
    return _padded(case.dirty, case.world, others), case.dirty_counts, _padded(case.held, case.world, others), case.held_counts


def _singles(count, z, world, first=0, skip=()):
    """`count` keys (first + i, i % 7 - 3, z), each held by ONE rank (not in `skip`) and dirty nowhere: one entry each."""
    ranks = [r for r in range(world) if r not in skip]
    return [((first + i, i % 7 - 3, z), (), (ranks[i % len(ranks)],)) for i in range(count)]


def _mixed(count, world, seed, z=3, skip=()):
    """`count` keys with random holders and dirty ranks (a dirty rank need not hold the key)."""
    rng = np.random.default_rng(seed)
    ranks = [r for r in range(world) if r not in skip]
    out = []
    for i in range(count):
        h = [r for r in ranks if rng.random() < (0.5 if world <= 8 else 0.1)]
        d = [r for r in ranks if rng.random() < (0.3 if world <= 8 else 0.05)]
        if not h and not d:
            h = [ranks[i % len(ranks)]]
        out.append(((i - count // 2, (i * 5) % 11 - 5, z + i % 3), d, h))
    return out


# what the issue's list names, on three ranks: (key, dirty on, held by)
_RULES3 = [
    ((1, 0, 0), (0,), (0,)),         # dirty on one rank, held by one: not shared
    ((0, 0, 1), (0,), (1, 2)),       # dirty on a rank that does not hold it, held by two others: shared, rank 1 keeps
    ((4, 4, 4), (), (0, 2)),         # held by two, dirty nowhere: not shared
    ((7, 7, 7), (1,), (1,)),         # dirty and held on one rank only: not shared
    ((2, 2, 2), (2,), (0, 1, 2)),    # dirty on the last rank, held by all: rank 0 keeps
    ((-3, 0, 1), (1, 2), (1, 2)),    # rank 1 keeps
    ((5, -5, 0), (0, 1, 2), ()),     # dirty everywhere, held nowhere (released since): not shared
    ((1, 0, -1), (2,), (2, 0)),      # with (0, 0, 1): (x, y, z) order and packed order differ
]
_RIM = [((-B, 0, 0), (0,), (0, 1)), ((B - 1, 0, 0), (1,), (0, 1)), ((0, -B, 5), (0, 1), (0, 1)), ((0, B - 1, 5), (1,), (1, 0)),
        ((3, 3, -B), (0,), (0, 1)), ((3, 3, B - 1), (1,), (0, 1)), ((-B, -B, -B), (0,), (1, 0)), ((B - 1, B - 1, B - 1), (0, 1), (0, 1)),
        ((B - 1, -B, 0), (1,), (1,)), ((-B, B - 1, 0), (), (0, 1))]


def _straddle(world, below, above, seed, name):
    """(0, 0, 0) held by all and dirty on all - a run of 2 * world entries - with `below` single entries of smaller packed keys
    (z = -1) and `above` of larger (z = 2): the run covers sorted entries [below, below + 2 * world)."""
    everyone = tuple(range(world))
    return KeyLists(name, world, _singles(below, -1, world) + [((0, 0, 0), everyone, everyone)] + _singles(above, 2, world), seed)


def _filled(name, world, entries, total, seed):
    """The entries plus single entries (keys nothing else uses, z = 40) up to exactly `total` entries."""
    short = total - KeyLists(name, world, entries).total()
    assert short >= 0, (name, short)
    return KeyLists(name, world, list(entries) + _singles(short, 40, world, first=-500), seed)


def _on_two_of_three(entries, a, b):
    """Three-rank entries restricted to ranks 0 and 1, which become ranks a and b: the third rank of the world is empty."""
    to = {0: a, 1: b}
    out = [(k, [to[r] for r in d if r < 2], [to[r] for r in h if r < 2]) for k, d, h in entries]
    return [e for e in out if e[1] or e[2]]


@functools.lru_cache(maxsize=None)
def key_list_cases():
    return (
        KeyLists("w1 one entry", 1, [((5, 6, 7), (), (0,))]),
        KeyLists("w1 dirty and held", 1, [((0, 0, 0), (0,), (0,)), ((1, 0, 0), (0,), (0,)), ((0, 0, 1), (), (0,)), ((-B, B - 1, 0), (0,), ())], 1),
        KeyLists("w1 empty", 1, []),
        KeyLists("w2 rim", 2, _RIM, 2),
        _filled("w2 total 255", 2, _mixed(40, 2, 11), 255, 3),
        KeyLists("w3 rules", 3, _RULES3, 4),
        _filled("w3 rules total 256", 3, _RULES3, 256, 21),
        KeyLists("w3 first empty", 3, _on_two_of_three(_RULES3, 1, 2), 5),
        KeyLists("w3 middle empty", 3, _on_two_of_three(_RULES3, 0, 2) + _mixed(30, 3, 12, z=20, skip=(1,)), 6),
        KeyLists("w3 last empty", 3, _on_two_of_three(_RULES3, 0, 1), 7),
        # a rank that lists a key twice as held is ONE holder: (6, 1, 0) has one holder and is not shared, (6, 1, 1) has two, keeper 1
        KeyLists("w3 held twice", 3, [((6, 1, 0), (0,), (1,)), ((6, 1, 1), (0,), (1, 2)), ((6, 1, 2), (2,), (2,))], 15,
                 held_twice=[((6, 1, 0), 1), ((6, 1, 1), 1)]),
        KeyLists("w3 all empty", 3, []),
        KeyLists("w8 all empty", 8, []),
        _straddle(8, 241, 0, 8, "w8 straddle total 257"),  # the run of 16 covers sorted entries 241 .. 256
        KeyLists("w8 mixed 3000", 8, _mixed(470, 8, 13), 9),
        _straddle(64, 200, 40, 10, "w64 straddle"),         # the run of 128 covers sorted entries 200 .. 327
        KeyLists("w64 mixed", 64, _mixed(150, 64, 14, skip=(32,)) + [((90, 9, 9), (5,), (0, 63)), ((90, 9, 10), (63,), (62, 63))], 11),
    )


# ---- unit states ---------------------------------------------------------------------------------------------------------------
POOL_KEYS = ((0, 0, 0), (-1, 0, 0), (0, -1, 2), (3, 1, -2), (B - 1, -B, 7), (-B, 4, B - 1), (2, 2, 2), (-4, 5, 1), (6, -6, 0), (1, 1, 1))
ONE_VOXEL_KEYS = ((10, 0, 0), (10, 1, 0), (10, 2, 0), (10, 3, 0))
ONE_VOXEL_WORDS = (0, NV - 1, 16, 1234)  # dump-order indices: the library's words 0, 4095, 1 (library_word(16)) and library_word(1234)
ABSENT_KEYS = ((50, 50, 50), (51, 50, 50), (52, 50, 50))  # no rank holds them; actions 0, 1 and 2
OUT_OF_RANGE = (B, 0, 0)
WORLDS = (2, 3, 8)


class UnitCase:
    """states[r]: rank r's state; keys: the list for halo_unpack (no repeats); export_keys: the same with a repeated key;
    actions[r]: rank r's action vector over `keys`."""

    def __init__(self, world, seed):
        self.world = world
        rng = np.random.default_rng(seed)
        self.states = []
        for r in range(world):
            hold = [k for i, k in enumerate(POOL_KEYS) if rng.random() < 0.6 or (i + r) % 5 == 0]
            parts = [PR.state_of_planted(ps.random_units(np.array(hold, np.int64), seed * 100 + r, unobserved=0.3))]
            if r < 2:  # two ranks hold the one-voxel units, each its voxel in another unit
                words = ONE_VOXEL_WORDS[r:] + ONE_VOXEL_WORDS[:r]
                parts.append(PR.state_of_planted(ps.one_voxel_units(words, ONE_VOXEL_KEYS)[0]))
            keys, bits, weight, sums = (np.concatenate([p[i] for p in parts]) for i in range(4))
            # weight 0 with tsdf bits that are not zero (a positive and a negative value: the export's product is +0 and -0)
            for u in range(len(hold)):
                at = rng.choice(NV, 6, replace=False)
                weight[u, at], sums[u, at] = 0, 0
                bits[u, at] = np.array([0.5, -0.25, 1.0, -1.0, 1e-3, -0.0], np.float32).view(np.uint32)
                lo, hi = rng.choice(NV, 8, replace=False).reshape(2, 4)
                sums[u, lo] = 0
                sums[u, hi] = 255 * weight[u, hi][:, None]
            assert len(keys) <= 24 and weight.max() <= 7
            self.states.append((keys, bits, weight, sums))
        pool = [POOL_KEYS[i] for i in rng.permutation(len(POOL_KEYS))] + list(ONE_VOXEL_KEYS)
        self.keys = np.array(pool[:5] + [ABSENT_KEYS[0], OUT_OF_RANGE] + pool[5:9] + [ABSENT_KEYS[1]] + pool[9:] + [ABSENT_KEYS[2]], np.int32)
        self.export_keys = np.concatenate([self.keys, self.keys[2:3], self.keys[:1]])
        self.actions = []
        for r in range(world):
            a = (np.arange(len(self.keys)) + r) % 3
            for k, act in zip(ABSENT_KEYS, (0, 1, 2)):
                a[(self.keys == np.array(k)).all(1)] = act
            a[(self.keys == np.array(OUT_OF_RANGE)).all(1)] = 1
            self.actions.append(a.astype(np.uint8))

    def reduced(self):
        """The all-reduce of the ranks' exports over `keys`, with a numerator of 0.75 planted at every eleventh voxel whose reduced
        weight is 0 (a payload no sum of exports holds: the W > 0 guard decides what becomes of it)."""
        total = ER.reduce_payloads([ER.export_payload(s, self.keys) for s in self.states])
        zero_w = np.argwhere(total[..., 1] == 0)[::11]
        total[zero_w[:, 0], zero_w[:, 1], 0] = np.float32(0.75)
        return total


@functools.lru_cache(maxsize=None)
def unit_case(world):
    return UnitCase(world, 7 + world)


def unit_cases():
    return [unit_case(w) for w in WORLDS]


def state_buffer(state):
    """A state as the packed buffer ScalableTSDFVolume.unpack takes: plants bit patterns import_numerators cannot (weight 0 with
    tsdf bits)."""
    return np.frombuffer(PR.pack_reference(*state, voxel_length=ps.VOX, sdf_trunc=ps.TRUNC), np.uint8).copy()


# ---- merge windows -------------------------------------------------------------------------------------------------------------
WINDOW_KEYS = tuple((x, y, 0) for x in range(-2, 2) for y in range(2))  # 8 units


def window_units(world, window):
    """What rank r writes in merge window 0 / 1: {r: key array}.  Window 0: a sliding pair of ranks per key, so every key has
    two writers or one.  Window 1: units merged before written again by their keeper, by a rank that zeroed them and by a rank
    that never held them; and new units only one rank writes."""
    out = {r: [] for r in range(world)}
    for i, k in enumerate(WINDOW_KEYS[:6]):
        if window == 0:
            out[i % world].append(k)
            if i % 3 != 2:
                out[(i + 1) % world].append(k)
        elif i < 3:
            out[(i + window + 1) % world].append(k)
    if window == 1:
        out[0].append(WINDOW_KEYS[0])
        out[world - 1].append(WINDOW_KEYS[6])
        out[0].append(WINDOW_KEYS[7])
    return {r: np.array(sorted(set(v)), np.int64).reshape(-1, 3) for r, v in out.items()}


def window_states(world, window):
    """-> {r: planted_states states} of what rank r adds in the window (values depend on rank, window and key)."""
    return {r: ps.random_units(k, 1000 * window + 10 * world + r, unobserved=0.3) for r, k in window_units(world, window).items() if len(k)}


# ---- pair lists ----------------------------------------------------------------------------------------------------------------
GARBAGE = 0x5A5AA5A5DEADBEE5  # the unused tail of a hand-built message
PAIR_WORLDS = (1, 2, 3, 8)
PAIR_CAPS = (1, 5, 64, 4096)


class PairCase:
    def __init__(self, name, world, cap, lists, counts=None):
        """lists[r]: rank r's distinct (instance, object, votes); counts[r]: what msg[0] says (None: the list's length)."""
        self.name, self.world, self.cap, self.lists = name, world, cap, lists
        self.counts = counts or [None] * world
        for lst in lists:
            assert len(lst) <= cap and len({(i, o) for i, o, _ in lst}) == len(lst)

    def messages(self, fill=GARBAGE):
        return np.stack([ER.message(*pack_pairs(lst), self.cap, fill, n) for lst, n in zip(self.lists, self.counts)])

    def merged(self, variant=None):
        return ER.merge_pairs(self.messages(), self.cap, variant)


def _rank_list(r, n, shared=5):
    """n distinct pairs of rank r: min(shared, n) of the markers and votes every rank lists (the votes of (3, 2) differ by rank),
    then pairs only this rank lists.  A list shorter than `shared` is all common on even ranks and all its own on odd ones."""
    common = [(3, SEEN, 1), (3, 2, 1 + r), (0, SEEN, 1), (9, PENDING, 2), (3, 5, 2)][:shared]
    own = [(100 + r, j, 1 + j % 4) if j % 3 else (20 + j % 50, 1000 + 5000 * r + j, 1 + j % 3) for j in range(n)]
    if n < len(common):
        return common[:n] if r % 2 == 0 else own[:n]
    return common + own[:n - len(common)]


@functools.lru_cache(maxsize=None)
def pair_cases():
    out = []
    for world in PAIR_WORLDS:
        for cap in PAIR_CAPS[:3]:
            choices = (0, 1, cap - 1, cap)
            ns = [choices[(r + world + cap) % 4] for r in range(world)]
            out.append(PairCase(f"w{world} cap{cap}", world, cap, [_rank_list(r, n) for r, n in enumerate(ns)]))
    # cap 4096: n = cap and cap - 1, the merged list exactly 4096 distinct pairs (rank 1 lists all of rank 0's but the first)
    full = [(1 + j // 64, j % 64, 1 + j % 3) for j in range(4096)]
    out.append(PairCase("w2 cap4096 merged 4096", 2, 4096, [full, full[1:]]))
    out.append(PairCase("w3 cap4096 short", 3, 4096, [_rank_list(0, 1), [], _rank_list(2, 70)]))
    # hand-edited counts over plausible slots: a negative one (nothing of the rank counts), one above cap (cap pairs count)
    out.append(PairCase("w3 cap5 bad counts", 3, 5, [_rank_list(r, 5, shared=3) for r in range(3)], [None, -3, 5 + 4]))
    out.append(PairCase("w2 cap64 count above cap", 2, 64, [_rank_list(0, 64), _rank_list(1, 3)], [64 + 9, None]))
    return tuple(out)


def overflow_lists():
    """Two ranks with 3000 disjoint pairs each: a merged list of 6000 > 4096 pairs."""
    return [[(1 + j // 50, 100000 * r + j, 1) for j in range(3000)] for r in range(2)]
