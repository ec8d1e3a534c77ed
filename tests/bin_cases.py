"""TEST INFRASTRUCTURE ONLY - planted inputs for the per-call point bins (pyslam_amd/csrc/hv_bins.h and the bin / fold kernels of
hv_voxel_grid.hip and hv_semantic.hip).  No GPU here: tests/test_bin_cases_cpu.py holds these builders to the CPU oracles, the
GPU files tests/test_gpu_voxel_grid_bins.py and tests/test_gpu_semantic_bins.py feed them to the grids.

A builder returns the inputs of ONE integrate call plus what it planted: which block every point falls into (`bin_of`, `keys`,
`sizes`) and its local voxel (`local`).  Every point sits within 0.25 voxel of a voxel centre, so no key depends on a rounding at a
cell border (that border is tests/test_gpu_voxel_grid.py::test_keys_bit_exact's job); blocks lie at negative and positive indices.

layout     how a bin's points (taken in point-index order, j = 0 .. N-1) fall over the block's voxels
           one_voxel        a single run of N points
           distinct         min(N, bs^3) voxels in a scrambled order, point j in voxel j mod bs^3
           two_alternating  two voxels, even j / odd j
           random
           ends             local voxel 0 for the lower half of the bin's point indices, bs^3 - 1 for the upper half: the packed
                            entry (voxel << index bits | point index) of the call's last points is as close to the all-ones padding
                            of the sorts as the call allows
placement  where a bin's points sit in the call
           contiguous       bin after bin: a wave's 64 lanes share a block and reserve 64 places with one atomic (ladder_bins puts a
                            spacer bin in front of the 257-bin, which then starts at point index 6 mod 64: the lane groups of its
                            waves hold 58, 64, 64, 64, 64 ... points and the fifth asks for places 250 .. 313)
           round_robin      consecutive points lie in different blocks: lane groups as small as the mix of bins allows
           shuffled
           windowed         bins beyond `window_over` get explicit runs of point indices (window_runs), the other bins and filler
                            points of further blocks are scattered over the rest of the call

Payloads are order-sensitive: colours random uint8 or non-dyadic float32, positions full-mantissa, class / instance ids random
with the first two points of every voxel run near (below every depth threshold) and differently labelled - the voting counter of
a two-point run then names the LATER point, and tests/test_bin_cases_cpu.py checks on the oracle that reversing the call changes
every bin that can change.  Depths fall on both sides of the depth thresholds (10 voting, 5 probabilistic)."""
import numpy as np

# The size thresholds the ladders straddle, each written once; tests/test_bin_cases_cpu.py parses the sources and compares.
HV_BIN_K0 = 256        # hv_bins.h: inline entries per table slot
HV_BIN_PG = 256        # hv_bins.h: entries per overflow page
HV_BIN_THREADS = 512   # hv_bins.h: threads (= s_first / s_new_slot entries) of a bin-pass workgroup
HV_VGB_IDX_BITS = 20   # hv_bins.h: point-index bits of a VOXEL_GRID entry
HV_VGB_CAP = 4096      # hv_bins.h: k_vgb_fold's LDS window
HV_VGB_WCAP = 1024     # hv_bins.h: k_vgb_fold_wave's LDS window
HV_VGB_STAGE = 128     # hv_voxel_grid.hip: staged fold
HV_VGB_RANK = 256      # hv_voxel_grid.hip: register rank sort
HV_SEMB_STAGE = 128    # hv_semantic.hip: staged records (frame source)
SEM_WCAP = 512         # hv_semantic.hip: sem_wcap()
WAVE = 64

CONSTANT_SOURCES = {
    "hv_bins.h": ("HV_BIN_K0", "HV_BIN_PG", "HV_BIN_THREADS", "HV_VGB_IDX_BITS", "HV_VGB_CAP", "HV_VGB_WCAP"),
    "hv_voxel_grid.hip": ("HV_VGB_STAGE", "HV_VGB_RANK"),
    "hv_semantic.hip": ("HV_SEMB_STAGE",),
}


def _around(*values):
    return sorted({v + d for v in values for d in (-1, 0, 1)})


# VG: 1 2 63 64 65 127 128 129 255 256 257 511 512 513 767 768 769 1023 1024 1025 4095 4096 4097 5000
VG_LADDER = sorted({1, 2, 5000} | set(_around(WAVE, HV_VGB_STAGE, HV_VGB_RANK, HV_BIN_K0, HV_BIN_K0 + HV_BIN_PG, HV_BIN_K0 + 2 * HV_BIN_PG,
                                               HV_VGB_WCAP, HV_VGB_CAP)))
VG_LADDER_WAVE = [s for s in VG_LADDER if s <= HV_VGB_WCAP + 1]  # one call: ... 1023 1024 1025
VG_LADDER_SMALL = [s for s in VG_LADDER if s <= HV_VGB_WCAP]
# SEM: 1 2 63 64 65 127 128 129 255 256 257 511 512 513 1023 1024 1025 1537
SEM_LADDER = sorted({1, 2, 3 * SEM_WCAP + 1} | set(_around(WAVE, HV_SEMB_STAGE, HV_BIN_K0, SEM_WCAP, HV_BIN_K0 + 3 * HV_BIN_PG)))
FRAME_LADDER = [s for s in SEM_LADDER if s <= HV_BIN_K0 + 3 * HV_BIN_PG + 1]  # ... 1025: 5955 pixels of a 96 x 64 image

LAYOUTS = ("one_voxel", "distinct", "two_alternating", "random", "ends")
PLACEMENTS = ("contiguous", "round_robin", "shuffled")
VOXEL = 0.05
NEAR_DEPTH = 3.0  # below every depth threshold in use
VOTE_THRESHOLD = 10.0  # the voting payloads' depth gate in the tests


class Call:
    """One integrate call and what was planted in it."""

    def __init__(self, voxel, bs, points, colors, class_ids, instance_ids, depths, bin_of, local, keys, sizes, planted):
        self.voxel, self.bs = voxel, bs
        self.points, self.colors, self.class_ids, self.instance_ids, self.depths = points, colors, class_ids, instance_ids, depths
        self.bin_of, self.local = bin_of, local  # per point: row of keys / sizes, local voxel index
        self.keys, self.sizes = keys, sizes      # every block of the call, the `planted` bins first, filler blocks after them
        self.planted = planted

    @property
    def n(self):
        return len(self.bin_of)

    def reversed(self):
        r = slice(None, None, -1)
        c = None if self.colors is None else np.ascontiguousarray(self.colors[r])
        return Call(self.voxel, self.bs, np.ascontiguousarray(self.points[r]), c, self.class_ids[r].copy(), self.instance_ids[r].copy(),
                    self.depths[r].copy(), self.bin_of[r].copy(), self.local[r].copy(), self.keys, self.sizes, self.planted)

    def grid_args(self):
        return self.points, self.colors

    def semantic_args(self, use_inst=True, use_depth=True):
        return self.points, self.colors, self.class_ids, self.instance_ids if use_inst else None, self.depths if use_depth else None

    def voxel_counts(self):
        """-> {block key tuple: counts [bs^3]} of the call."""
        nvox = self.bs ** 3
        flat = np.bincount(self.bin_of.astype(np.int64) * nvox + self.local, minlength=len(self.keys) * nvox).reshape(len(self.keys), nvox)
        return {tuple(int(x) for x in self.keys[b]): flat[b] for b in range(len(self.keys))}


_KEY_POOL = None


def key_pool():
    """4096 distinct block keys in [-8, 8)^3 in a fixed scrambled order."""
    global _KEY_POOL
    if _KEY_POOL is None:
        g = np.arange(-8, 8)
        k = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        _KEY_POOL = k[np.random.default_rng(20240607).permutation(len(k))].astype(np.int32)
    return _KEY_POOL


def bins_of(sizes, first_key=0):
    """(block key, size) pairs: sizes[k] points in block key_pool()[first_key + k]."""
    pool = key_pool()
    return [(tuple(int(x) for x in pool[first_key + k]), int(s)) for k, s in enumerate(sizes)]


def ladder_bins(sizes, first_key=0):
    """bins_of with a spacer bin in front of the first bin beyond the inline entries: that bin then starts at point index 6 mod 64
    of a contiguous call."""
    sizes = list(sizes)
    big = [k for k, s in enumerate(sizes) if s > HV_BIN_K0]
    if big:
        at = big[0]
        lead = sum(sizes[:at])
        sizes.insert(at, (6 - lead) % WAVE or WAVE)
    return bins_of(sizes, first_key)


def window_cap(n):
    """The largest window (512, 1024 or 4096 point indices) that a bin of n points can fill with 3 points to spare."""
    caps = [c for c in (SEM_WCAP, HV_VGB_WCAP, HV_VGB_CAP) if n >= c + 3]
    return caps[-1] if caps else None


def window_runs(n, base):
    """Runs (start, length) of point indices for a bin of n points in the region that starts at `base` (a multiple of 4096), c =
    window_cap(n): [base + c - a, base + 2c + a) fills the window [base + c, base + 2c) and straddles both of its ends; the
    other points follow at base + 4c + 17, behind a window that holds none of the bin.  -> runs, region length."""
    c = window_cap(n)
    a = min(300, (n - c) // 3)
    rest = n - c - 2 * a
    runs = [(base + c - a, c + 2 * a), (base + 4 * c + 17, rest)]
    length = -(-(4 * c + 17 + rest) // HV_VGB_CAP) * HV_VGB_CAP
    return runs, length


def _place(sizes, placement, rng, window_over):
    """-> bin index per call slot (-1: a filler slot, windowed placement only)."""
    sizes = np.asarray(sizes, np.int64)
    nb = len(sizes)
    if placement == "contiguous":
        return np.repeat(np.arange(nb), sizes)
    if placement == "shuffled":
        return rng.permutation(np.repeat(np.arange(nb), sizes))
    if placement == "round_robin":
        rounds = np.concatenate([np.arange(s) for s in sizes])
        who = np.repeat(np.arange(nb), sizes)
        return who[np.lexsort((who, rounds))]
    assert placement == "windowed", placement
    big = [b for b in range(nb) if sizes[b] > window_over]
    base, runs = 0, []
    for b in big:
        r, length = window_runs(int(sizes[b]), base)
        runs += [(b, s, n) for s, n in r]
        base += length
    out = np.full(base + HV_VGB_CAP, -1, np.int64)
    for b, s, n in runs:
        assert (out[s:s + n] == -1).all()
        out[s:s + n] = b
    free = np.nonzero(out == -1)[0]
    small = np.repeat([b for b in range(nb) if sizes[b] <= window_over], [sizes[b] for b in range(nb) if sizes[b] <= window_over])
    assert len(small) <= len(free)
    out[rng.permutation(free)[:len(small)]] = small
    return out


def _layout_local(layout, j, n, nvox, rng, choices=None):
    """Local voxel of the bin's j-th point (j in point-index order), out of `choices` (default: all nvox voxels of the block)."""
    choices = np.arange(nvox) if choices is None else np.asarray(choices)
    m = len(choices)
    if layout == "one_voxel":
        return np.full(n, choices[rng.integers(0, m)])
    if layout == "distinct":
        return choices[rng.permutation(m)][j % m]
    if layout == "two_alternating":
        a, b = rng.choice(m, 2, replace=False) if m > 1 else (0, 0)
        return np.where(j % 2 == 0, choices[a], choices[b])
    if layout == "random":
        return choices[rng.integers(0, m, n)]
    assert layout == "ends", layout
    return np.where(j < (n + 1) // 2, choices[0], choices[-1])


def _run_ranks(bin_of, local, nvox):
    """Rank of every point inside its voxel's run (point-index order)."""
    gid = bin_of.astype(np.int64) * nvox + local
    order = np.argsort(gid, kind="stable")
    g = gid[order]
    start = np.r_[True, g[1:] != g[:-1]]
    first = np.maximum.accumulate(np.where(start, np.arange(len(g)), 0))
    rank = np.empty(len(g), np.int64)
    rank[order] = np.arange(len(g)) - first
    return rank, order


def vote_states(cls, inst, gate):
    """The two voting payloads' label state after one voxel run (update_voxel_direct over voxel_data_semantic.h:168-198 and
    voxel_data_semantic2.h's separate object / class counters), restated: -> ((object, class, counter), (object, class, smaller counter))."""
    o = c = k = 0
    o2 = c2 = ko = kc = 0
    for j in range(len(cls)):
        if not gate[j]:
            continue
        oj, cj = int(inst[j]) + 1, int(cls[j]) + 1
        if j == 0:
            o, c, k = oj, cj, 1
            o2, c2, ko, kc = oj, cj, 1, 1
            continue
        if o == oj and c == cj:
            k += 1
        else:
            k -= 1
            if k <= 0:
                o, c, k = oj, cj, 1
        if o2 == oj:
            ko += 1
        else:
            ko -= 1
            if ko <= 0:
                o2, ko = oj, 1
        if c2 == cj:
            kc += 1
        else:
            kc -= 1
            if kc <= 0:
                c2, kc = cj, 1
    return (o, c, k), (o2, c2, min(ko, kc))  # (what a dump shows of the second: the ids and the smaller counter)


def _order_sensitive(cls, inst, dep):
    """Both voting payloads end differently when the run arrives reversed - with the depth gate (threshold 10) and without it."""
    for gate in (dep < VOTE_THRESHOLD, np.ones(len(dep), bool)):
        f, r = vote_states(cls, inst, gate), vote_states(cls[::-1], inst[::-1], gate[::-1])
        if f[0] == r[0] or f[1] == r[1]:
            return False
    return True


def _labels(bin_of, local, nvox, rng, depths=None):
    """Class ids in 0..2, instance ids in 0..1 (<= 6 pairs and <= 3 + 2 marginal entries per voxel: inside the inline label slots),
    depths in (0, 20) unless given.  The first two points of a voxel run carry different classes and (drawn depths) are near: a
    two-point run names its later point.  A bin without a two-point run gets the labels of its longest run drawn again until
    the run is order-sensitive for both voting payloads (vote_states)."""
    n = len(bin_of)
    cls = rng.integers(0, 3, n).astype(np.int32)
    inst = rng.integers(0, 2, n).astype(np.int32)
    dep = (rng.random(n) * 20.0).astype(np.float32) if depths is None else np.asarray(depths, np.float32)
    rank, order = _run_ranks(bin_of, local, nvox)
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    second = np.nonzero(rank == 1)[0]
    head = order[pos[second] - 1]
    cls[second] = (cls[head] + 1) % 3
    if depths is None:
        near = rank <= 1
        dep[near] = (0.5 + rng.random(int(near.sum())) * (NEAR_DEPTH - 0.5)).astype(np.float32)
    # run lengths per point, then per bin: is there a two-point run, and which run is the longest
    gid = bin_of.astype(np.int64) * nvox + local
    length = np.bincount(gid)[gid]
    for b in np.unique(bin_of):
        at = np.nonzero(bin_of == b)[0]
        if (length[at] == 2).any() or length[at].max() < 3:
            continue
        run = at[local[at] == local[at[np.argmax(length[at])]]]  # ascending point indices
        for _ in range(200):
            if _order_sensitive(cls[run], inst[run], dep[run]):
                break
            cls[run[2:]] = rng.integers(0, 3, len(run) - 2)
            inst[run[2:]] = rng.integers(0, 2, len(run) - 2)
        else:
            raise AssertionError("no order-sensitive labels found")
    return cls, inst, dep


def _make_sums_order_sensitive(x, bin_of, local, nvox, redraw):
    """x: one float32 addend per point (in place).  In every bin that has a voxel run of three or more points, some run's float32 sum
    in point order differs from its sum in reversed order; where none does, redraw(point indices) supplies the longest run's
    addends again."""
    gid = bin_of.astype(np.int64) * nvox + local
    length = np.bincount(gid)[gid]
    order = np.argsort(gid, kind="stable")
    order = order[length[order] >= 3]
    if len(order) == 0:
        return
    g = gid[order]
    runs = np.split(order, np.nonzero(g[1:] != g[:-1])[0] + 1)
    by_bin = {}
    for r in runs:
        by_bin.setdefault(int(bin_of[r[0]]), []).append(r)

    def differs(r):
        return np.add.accumulate(x[r])[-1] != np.add.accumulate(x[r[::-1]])[-1]

    for rs in by_bin.values():
        if any(differs(r) for r in rs):
            continue
        longest = max(rs, key=len)
        for _ in range(200):
            x[longest] = redraw(longest)
            if differs(longest):
                break
        else:
            raise AssertionError("no order-sensitive positions found")


def _colors(kind, n, rng):
    if kind == "none":
        return None
    if kind == "u8":
        return rng.integers(0, 256, (n, 3), dtype=np.uint8)
    assert kind == "f32", kind
    return rng.random((n, 3), dtype=np.float32)


def _positions(vox, voxel, dtype, bin_of, local, nvox, rng):
    """Points within 0.25 voxel of the centres of the voxels `vox` [n,3]; x is drawn again where a bin's sums would not depend on order."""
    vs = float(np.float32(voxel))
    pts = ((vox + 0.5 + (rng.random(vox.shape) - 0.5) * 0.5) * vs).astype(dtype)
    x = pts[:, 0].astype(np.float32)  # (the addend the voxel sums take)
    _make_sums_order_sensitive(x, bin_of, local, nvox, lambda at: ((vox[at, 0] + 0.5 + (rng.random(len(at)) - 0.5) * 0.5) * vs).astype(dtype).astype(np.float32))
    changed = x != pts[:, 0].astype(np.float32)
    pts[changed, 0] = x[changed]
    return np.ascontiguousarray(pts)


def points_call(voxel, bs, bins, layout, placement, seed, dtype=np.float32, color="u8", window_over=HV_VGB_WCAP, filler=40):
    """One integrate call with bins[k] = (block key, size) planted.  `filler`: the largest filler block (windowed placement)."""
    rng = np.random.default_rng(seed)
    nvox = bs ** 3
    keys = [k for k, _ in bins]
    sizes = [s for _, s in bins]
    assert len(set(keys)) == len(keys)
    bin_of = _place(sizes, placement, rng, window_over)
    free = np.nonzero(bin_of < 0)[0]
    if len(free):  # filler points of further blocks
        used, pool, at = set(keys), key_pool(), 0
        left = len(free)
        fill_sizes = []
        while left:
            k = tuple(int(x) for x in pool[at])
            at += 1
            if k in used:
                continue
            s = min(left, int(rng.integers(1, filler + 1)))
            keys.append(k)
            fill_sizes.append(s)
            left -= s
        bin_of[rng.permutation(free)] = np.repeat(np.arange(len(sizes), len(sizes) + len(fill_sizes)), fill_sizes)
        sizes = sizes + fill_sizes
    n = len(bin_of)
    local = np.zeros(n, np.int64)
    for b in range(len(sizes)):
        at = np.nonzero(bin_of == b)[0]  # ascending point indices
        lay = layout if b < len(bins) else "random"
        local[at] = _layout_local(lay, np.arange(len(at)), len(at), nvox, rng)
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    l3 = np.stack([local % bs, (local // bs) % bs, local // (bs * bs)], 1)
    vox = keys[bin_of].astype(np.int64) * bs + l3
    pts = _positions(vox, voxel, dtype, bin_of, local, nvox, rng)
    cls, inst, dep = _labels(bin_of, local, nvox, rng)
    return Call(voxel, bs, pts, _colors(color, n, rng), cls, inst, dep, bin_of, local, keys,
                np.asarray(sizes, np.int64), len(bins))


class Frame:
    """One posed RGB-D keyframe (depth f32, rgb u8, class / instance images i32) whose pixels plant `call`'s bins: pixel order is
    point order, depth-0 pixels are invalid."""

    def __init__(self, depth, rgb, cls, inst, intrinsics, T_cw, call):
        self.depth, self.rgb, self.cls, self.inst, self.intrinsics, self.T_cw, self.call = depth, rgb, cls, inst, intrinsics, T_cw, call


def frame_call(voxel, bs, sizes, layout, placement, seed, width=96, height=64, focal=60000.0, column=(-13, 21), z_block=6):
    """A frame source for sizes[k] points in the blocks (column's block, z_block + k): with the long focal length and the camera in the
    middle of voxel column `column` (x, y voxel indices) every pixel unprojects into that column (|x| <= 47.5 * z / focal < 0.15 voxel
    up to z = 9.2 m), and a pixel's depth alone picks its block and voxel along z.  Depths stay below 10: the voting payloads'
    gate passes every pixel, the probabilistic ones (threshold 5) see both sides."""
    rng = np.random.default_rng(seed)
    npx = width * height
    sizes = [int(s) for s in sizes]
    assert sum(sizes) <= npx
    vs = float(np.float32(voxel))
    assert 0.5 * width * (z_block + len(sizes)) * bs * vs / focal < 0.2 * vs
    which = _place(sizes, placement, rng, HV_VGB_WCAP)
    slot_bin = np.full(npx, -1, np.int64)
    if placement == "contiguous":
        slot_bin[:len(which)] = which
    else:  # the invalid pixels are scattered between the valid ones
        slot_bin[np.sort(rng.permutation(npx)[:len(which)])] = which
    valid = slot_bin >= 0
    bin_of = slot_bin[valid]
    n = len(bin_of)
    lz = np.zeros(n, np.int64)
    for b in range(len(sizes)):
        at = np.nonzero(bin_of == b)[0]
        lz[at] = _layout_local(layout, np.arange(len(at)), len(at), bs, rng)
    kx, ky = column
    local = (kx % bs) + (ky % bs) * bs + lz * bs * bs
    keys = np.array([[kx // bs, ky // bs, z_block + b] for b in range(len(sizes))], np.int32)
    vz = keys[bin_of, 2].astype(np.int64) * bs + lz
    z = ((vz + 0.5 + (rng.random(n) - 0.5) * 0.5) * vs).astype(np.float32)
    _make_sums_order_sensitive(z, bin_of, local, bs ** 3, lambda at: ((vz[at] + 0.5 + (rng.random(len(at)) - 0.5) * 0.5) * vs).astype(np.float32))
    depth = np.zeros(npx, np.float32)
    depth[valid] = z
    rgb = rng.integers(0, 256, (npx, 3), dtype=np.uint8)
    cls_v, inst_v, _ = _labels(bin_of, local, bs ** 3, rng, depths=z)
    cls, inst = np.zeros(npx, np.int32), np.zeros(npx, np.int32)
    cls[valid], inst[valid] = cls_v, inst_v
    T_cw = np.eye(4)
    T_cw[:3, 3] = [-(kx + 0.5) * vs, -(ky + 0.5) * vs, 0.0]
    intr = (focal, focal, (width - 1) / 2.0, (height - 1) / 2.0)
    call = Call(voxel, bs, None, None, cls_v, inst_v, z, bin_of, local, keys, np.asarray(sizes, np.int64), len(sizes))
    return Frame(depth.reshape(height, width), rgb.reshape(height, width, 3), cls.reshape(height, width), inst.reshape(height, width),
                 intr, T_cw, call)


# ---- the calls of the GPU files (tests/test_bin_cases_cpu.py walks the same lists) -----------------------------------------------
def vg_ladder(layout, placement, color="u8", dtype=np.float32, bs=8, seed=1):
    return points_call(VOXEL, bs, ladder_bins(VG_LADDER_WAVE), layout, placement, seed, dtype, color)


def vg_small_ladder(layout="random", placement="shuffled", bs=8, seed=2, color="f32"):
    return points_call(VOXEL, bs, ladder_bins(VG_LADDER_SMALL), layout, placement, seed, np.float32, color)


def vg_full_ladder(layout="random", bs=8, seed=3, color="f32"):
    """The whole VG ladder, the bins beyond 1024 in explicit point-index runs."""
    return points_call(VOXEL, bs, bins_of(VG_LADDER), layout, "windowed", seed, np.float32, color, window_over=HV_VGB_WCAP)


def vg_two_small(bs=8, seed=4, color="f32"):
    """Two small calls onto the ladder's blocks."""
    return [points_call(VOXEL, bs, bins_of([70, 3, 200, 1, 300], first_key=k), "random", "shuffled", seed + k, np.float32, color) for k in (0, 3)]


def stale_calls(bs=8, seed=10, color="u8"):
    """A: 600 points in each of 12 blocks (inline places + two pages each).  B: 10 points in the same blocks and 300 in 12 others
    (pages claimed under a new epoch, the other parity).  C: 9 further blocks.  D: 300 points in A's blocks - page 0 of each is
    claimed again under a new epoch with 44 entries where A left 256, page 1 stays A's - and 600 in B's others."""
    a = points_call(VOXEL, bs, bins_of([600] * 12), "random", "shuffled", seed, np.float32, color)
    b = points_call(VOXEL, bs, bins_of([10] * 12 + [300] * 12), "random", "shuffled", seed + 1, np.float32, color)
    c = points_call(VOXEL, bs, bins_of([5, 64, 257, 300, 1, 129, 513, 2, 90], first_key=40), "random", "shuffled", seed + 2, np.float32, color)
    d = points_call(VOXEL, bs, bins_of([300] * 12 + [600] * 12), "random", "shuffled", seed + 3, np.float32, color)
    return a, b, c, d


def firsts_calls(bs=8, seed=20, color="u8"):
    """1536 points in 1536 distinct new blocks: every bin-pass workgroup holds HV_BIN_THREADS first points of HV_BIN_THREADS new blocks;
    then 513 points in 513 blocks, 256 of them new: one full workgroup plus one thread."""
    a = points_call(VOXEL, bs, bins_of([1] * (3 * HV_BIN_THREADS), first_key=100), "random", "contiguous", seed, np.float32, color)
    b = points_call(VOXEL, bs, bins_of([1] * (HV_BIN_THREADS + 1), first_key=100 + 3 * HV_BIN_THREADS - 257), "random", "contiguous", seed + 1,
                    np.float32, color)
    return a, b


def many_pages_call(max_points=1 << 17, bs=8, seed=30):
    """Exactly max_points points in blocks of HV_BIN_K0 + 1 (the remainder in a last block): every block owns a page of one entry."""
    per = HV_BIN_K0 + 1
    sizes = [per] * (max_points // per)
    if max_points % per:
        sizes.append(max_points % per)
    return points_call(VOXEL, bs, bins_of(sizes), "random", "shuffled", seed, np.float32, "u8")


def sem_ladder(layout, placement, dtype=np.float32, bs=8, seed=5, color="u8"):
    return points_call(VOXEL, bs, ladder_bins(SEM_LADDER), layout, placement, seed, dtype, color)


def sem_big_calls(bs=8, seed=40):
    """-> {name: Call}: 1537 points in one voxel in explicit runs (a window of 512 consecutive point indices all in that voxel), 1025
    points over one 64-voxel range, 1025 points over all ranges."""
    nvox = bs ** 3
    one = points_call(VOXEL, bs, bins_of([3 * SEM_WCAP + 1, 40, 7]), "one_voxel", "windowed", seed, np.float32, "u8", window_over=SEM_WCAP, filler=200)
    out = {"one_voxel_1537_windowed": one}
    for name, choices in (("one_range_1025", np.arange(64, 128) % nvox), ("all_ranges_1025", np.arange(nvox))):
        c = points_call(VOXEL, bs, bins_of([2 * SEM_WCAP + 1, 30]), "random", "shuffled", seed + 1, np.float32, "u8")
        rng = np.random.default_rng(seed + 2)
        big = np.nonzero(c.bin_of == 0)[0]
        c.local[big] = choices[rng.integers(0, len(choices), len(big))]
        out[name] = _rebuild(c, seed + 3)
    return out


def _rebuild(c, seed):
    """Positions and labels of `c` again after its local voxels were edited."""
    rng = np.random.default_rng(seed)
    bs, local = c.bs, c.local
    l3 = np.stack([local % bs, (local // bs) % bs, local // (bs * bs)], 1)
    vox = c.keys[c.bin_of].astype(np.int64) * bs + l3
    c.points = _positions(vox, c.voxel, c.points.dtype, c.bin_of, local, bs ** 3, rng)
    c.class_ids, c.instance_ids, c.depths = _labels(c.bin_of, local, bs ** 3, rng)
    return c


def frame_ladder(layout="random", placement="shuffled", bs=8, seed=50):
    return frame_call(VOXEL, bs, FRAME_LADDER, layout, placement, seed)


def window_facts(call, b, cap):
    """For bin b of a call and windows [w, w + cap), w a multiple of cap: (a window filled by the bin alone, a window without a point of
    the bin between two windows that hold some, a run of consecutive point indices of the bin across a multiple of cap)."""
    idx = np.nonzero(call.bin_of == b)[0]
    per = np.bincount(idx // cap, minlength=call.n // cap + 1)
    hit = np.nonzero(per)[0]
    full = bool((per == cap).any())
    empty = bool((per[hit[0]:hit[-1] + 1] == 0).any())
    here = np.zeros(call.n + 1, bool)
    here[idx] = True
    edges = np.arange(cap, call.n, cap)
    straddle = bool((here[edges - 1] & here[edges]).any())
    return full, empty, straddle
