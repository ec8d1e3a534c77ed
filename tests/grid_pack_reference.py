"""The packed grid format of include/hipvol.h ("Packed grids"), restated in numpy from that comment - test infrastructure, no GPU.

A STATE here is (keys [B,3] int32, words [B, bs^3, record_bytes / 4] uint32, extra) with the voxels of a block in local order
k = lx + ly * bs + lz * bs^2, blocks in any order: `words` are the records as 32-bit words (padding and the chain link are ignored
and written as zero), `extra` maps (block row, k) to the voxel's label pairs beyond the six inline ones, [(id, class, log-probability
bits as uint32), ...] in insertion order.  record() builds one record's words from named fields.
"""
import math
import struct

import numpy as np

MAGIC = b"HVGRIDPK"
VERSION = 1
HEADER_BYTES = 192
SECTIONS = ("keys", "offsets", "masks", "records", "extras", "extra_obj", "extra_cls", "extra_logp")
KEY_BIAS = 1 << 20
MODES = (0, 1, 2, 11, 12)
MAP_MODES = (2, 12)
RECORD_BYTES = {0: 32, 1: 64, 11: 64, 2: 128, 12: 128}
# the words of a record that are content: everything but the padding and the chain link
CONTENT_WORDS = {0: 7, 1: 13, 11: 14, 2: 29, 12: 29}
INLINE, NODE, MAX_PAIRS = 6, 10, 254
_HEADER = struct.Struct("<8sIIdiiiiffqqqq8Q48x")
assert _HEADER.size == HEADER_BYTES


def _align(x):
    return (x + 63) & ~63


def mask_words(bs):
    return (bs ** 3 + 63) // 64


def section_sizes(mode, bs, B, N, P):
    return [12 * B, 8 * (B + 1), 8 * mask_words(bs) * B, RECORD_BYTES[mode] * N, N if mode in MAP_MODES else 0, 4 * P, 4 * P, 4 * P]


def layout(mode, bs, B, N, P):
    cur, offs = HEADER_BYTES, []
    for size in section_sizes(mode, bs, B, N, P):
        offs.append(cur)
        cur = _align(cur + size)
    return offs, cur


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def record(mode, count=0, pos=(0.0, 0.0, 0.0), col=(0.0, 0.0, 0.0), obj=-1, cls=-1, counter=0, cls_counter=0, pairs=(), best=(-1, -1)):
    """One record's words.  pairs = the label list [(id, class, log-probability)] of modes 2 / 12 (all of it: the first six go inline,
    the rest is returned as the voxel's `extra` list); best = cached best indices (mode 2: the first only).  -> (words, extra)."""
    w = np.zeros(RECORD_BYTES[mode] // 4, np.uint32)
    w[0] = np.uint32(np.int32(count).view(np.uint32))
    extra = []
    if mode == 0:
        w[1:4] = np.asarray(pos, np.float32).view(np.uint32)
        w[4:7] = np.asarray(col, np.float32).view(np.uint32)
    elif mode in (1, 11):
        w[1:4] = np.asarray([obj + 1, cls + 1, counter], np.int32).view(np.uint32)
        w[4:10] = np.asarray(pos, np.float64).view(np.uint32)
        w[10:13] = np.asarray(col, np.float32).view(np.uint32)
        if mode == 11:
            w[13] = np.uint32(np.int32(cls_counter).view(np.uint32))
    else:
        n = len(pairs)
        assert n <= MAX_PAIRS
        w[1] = n | ((best[0] + 1) << 8) | (((best[1] + 1) << 16) if mode == 12 else 0)
        w[2:8] = np.asarray(pos, np.float64).view(np.uint32)
        w[8:11] = np.asarray(col, np.float32).view(np.uint32)
        for i, (o, c, lp) in enumerate(pairs[:INLINE]):
            w[11 + i] = np.uint32(np.int32(o).view(np.uint32))
            w[17 + i] = np.uint32(np.int32(c).view(np.uint32))
            w[23 + i] = f32_bits(lp)
        extra = [(int(o), int(c), f32_bits(lp)) for o, c, lp in pairs[INLINE:]]
    return w, extra


def pack_reference(mode, bs, keys, words, extra=None, voxel_size=1.0 / 16.0, next_object_id=1, depth_threshold=10.0, depth_decay_rate=0.07):
    extra = extra or {}
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    B, nvox, rw, W = len(keys), bs ** 3, RECORD_BYTES[mode] // 4, mask_words(bs)
    words = np.asarray(words, np.uint32).reshape(B, nvox, rw).copy()
    words[:, :, CONTENT_WORDS[mode]:] = 0
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0])) if B else np.zeros(0, np.int64)
    stored = (words != 0).any(axis=2)  # [B, nvox]
    masks = np.zeros((B, W), np.uint64)
    offsets = np.zeros(B + 1, np.uint64)
    recs, extras, eo, ec, el = [], [], [], [], []
    for r, b in enumerate(order):
        for k in np.flatnonzero(stored[b]):
            masks[r, k >> 6] |= np.uint64(1) << np.uint64(k & 63)
            recs.append(words[b, k])
            if mode in MAP_MODES:
                more = extra.get((int(b), int(k)), [])
                assert len(more) == max(int(words[b, k, 1] & 0xFF) - INLINE, 0)
                extras.append(len(more))
                for o, c, lp in more:
                    eo.append(o), ec.append(c), el.append(lp)
        offsets[r + 1] = len(recs)
    N, P = len(recs), len(eo)
    offs, total = layout(mode, bs, B, N, P)
    out = bytearray(total)
    out[:HEADER_BYTES] = _HEADER.pack(MAGIC, VERSION, HEADER_BYTES, voxel_size, mode, bs, RECORD_BYTES[mode], next_object_id, depth_threshold,
                                      depth_decay_rate, B, N, P, total, *offs)
    parts = [keys[order].astype("<i4"), offsets.astype("<u8"), masks.astype("<u8"),
             np.asarray(recs, "<u4").reshape(N, rw), np.asarray(extras if mode in MAP_MODES else [], np.uint8),
             np.asarray(eo, "<i4"), np.asarray(ec, "<i4"), np.asarray(el, "<u4")]
    for off, part in zip(offs, parts):
        raw = part.tobytes()
        out[off:off + len(raw)] = raw
    return bytes(out)


HEADER_FIELDS = ("voxel_size", "mode", "block_size", "record_bytes", "version", "next_object_id", "depth_threshold", "depth_decay_rate", "blocks",
                 "voxels", "extra_pairs", "bytes", "chain_nodes")


def header_reference(buf):
    """The header's fields as packed_info names them (chain_nodes: None), plus "magic", "header_bytes" and "offsets" (no validation)."""
    f = _HEADER.unpack_from(buf, 0)
    return {"magic": f[0], "version": f[1], "header_bytes": f[2], "voxel_size": f[3], "mode": f[4], "block_size": f[5], "record_bytes": f[6],
            "next_object_id": f[7], "depth_threshold": f[8], "depth_decay_rate": f[9], "blocks": f[10], "voxels": f[11], "extra_pairs": f[12],
            "bytes": f[13], "offsets": list(f[14:22]), "chain_nodes": None}


def check_reference(buf):
    """The rules of hv_grid_packed_check, in its order.  ValueError naming the first rule that fails; -> the header otherwise."""
    buf = bytes(buf)
    if len(buf) < HEADER_BYTES:
        raise ValueError("header")
    h = header_reference(buf)
    if h["magic"] != MAGIC:
        raise ValueError("magic")
    if h["version"] != VERSION:
        raise ValueError("version")
    if h["header_bytes"] != HEADER_BYTES:
        raise ValueError("header_bytes")
    mode, bs = h["mode"], h["block_size"]
    if mode not in MODES:
        raise ValueError("mode")
    if not 1 <= bs <= 16:
        raise ValueError("block_size")
    if h["record_bytes"] != RECORD_BYTES[mode]:
        raise ValueError("record_bytes")
    B, N, P = h["blocks"], h["voxels"], h["extra_pairs"]
    if B < 0 or N < 0 or P < 0:
        raise ValueError("negative")
    if mode not in MAP_MODES and P != 0:
        raise ValueError("no maps")
    if B > len(buf) // 12 or N > len(buf) // RECORD_BYTES[mode] or P > len(buf) // 12:
        raise ValueError("exceed")
    if h["bytes"] != len(buf):
        raise ValueError("total_bytes")
    sizes = section_sizes(mode, bs, B, N, P)
    for off in h["offsets"]:
        if off % 64:
            raise ValueError("aligned")
    for off, size in zip(h["offsets"], sizes):
        if off < HEADER_BYTES or off > len(buf) or size > len(buf) - off:
            raise ValueError("outside")
    for a in range(8):
        for b in range(a + 1, 8):
            oa, ob = h["offsets"][a], h["offsets"][b]
            if sizes[a] and sizes[b] and not (oa + sizes[a] <= ob or ob + sizes[b] <= oa):
                raise ValueError("overlap")
    W, nvox = mask_words(bs), bs ** 3
    keys = np.frombuffer(buf, "<i4", 3 * B, h["offsets"][0]).reshape(B, 3).astype(np.int64)
    offsets = np.frombuffer(buf, "<u8", B + 1, h["offsets"][1])
    masks = np.frombuffer(buf, "<u8", W * B, h["offsets"][2]).reshape(B, W)
    if ((keys < -KEY_BIAS) | (keys >= KEY_BIAS)).any():
        raise ValueError("out of range")
    for b in range(1, B):
        if not tuple(keys[b - 1]) < tuple(keys[b]):
            raise ValueError("ascending")
    if offsets[0] != 0:
        raise ValueError("offsets[0]")
    if (offsets[1:] < offsets[:-1]).any():
        raise ValueError("decrease")
    if int(offsets[B]) != N:
        raise ValueError("offsets[B]")
    pop = np.unpackbits(masks.view(np.uint8).reshape(B, W * 8), axis=1).sum(axis=1).astype(np.uint64)
    if (pop != offsets[1:] - offsets[:-1]).any():
        raise ValueError("popcount")
    if nvox % 64 and B and (masks[:, W - 1] >> np.uint64(nvox % 64)).any():
        raise ValueError("high bits")
    extras = np.frombuffer(buf, np.uint8, sizes[4], h["offsets"][4])
    if (extras > MAX_PAIRS - INLINE).any():
        raise ValueError("extras entry")
    if int(extras.sum(dtype=np.int64)) != P:
        raise ValueError("extras sum")
    h["chain_nodes"] = int(((extras.astype(np.int64) + NODE - 1) // NODE).sum())
    return h


# the words of the library's message that name each rule of check_reference
RULE_WORDS = {"header": "fewer than", "magic": "bad magic", "version": "unsupported version", "header_bytes": "header_bytes is", "mode": "mode is",
              "block_size": "block_size is", "record_bytes": "record_bytes is", "negative": "negative blocks", "no maps": "has no label maps",
              "exceed": "exceed what a buffer", "total_bytes": "total_bytes", "aligned": "not 64-byte aligned", "outside": "lies outside the buffer",
              "overlap": "overlap", "out of range": "out of range", "ascending": "not strictly ascending", "offsets[0]": "offsets[0] is",
              "decrease": "offsets decrease", "offsets[B]": "offsets[B]", "popcount": "mask popcount", "high bits": "at or above block_size^3",
              "extras entry": "more than 248", "extras sum": "sum of extras"}


# ---- decoding ----------------------------------------------------------------------------------------------------------------------
def _expf(x):
    return np.float32(math.exp(float(x))) if x < 700 else np.float32(np.inf)


def _logf(x):
    x = float(x)
    return np.float32(-np.inf) if x == 0.0 else np.float32(math.log(x)) if x > 0 else np.float32(np.nan)


def _log_add_exp(a, b):
    if a == -np.inf:
        return b
    if b == -np.inf:
        return a
    m = b if a < b else a
    return np.float32(m + _logf(np.float32(_expf(np.float32(a - m)) + _expf(np.float32(b - m)))))


def _prob_voxel(meta, pairs):
    """Mode 2, hv_semantic.h: -> (object id, class id, confidence f32)."""
    n, best = meta & 0xFF, ((meta >> 8) & 0xFF) - 1
    if n == 0:
        return -1, -1, np.float32(0)
    key = lambda p: (p[0], p[1])
    if best < 0:
        for i, p in enumerate(pairs):
            if best < 0 or p[2] > pairs[best][2] or (p[2] == pairs[best][2] and key(p) < key(pairs[best])):
                best = i
    o, c, lp = pairs[best]
    if o == -1 or c == -1:
        return o, c, np.float32(0)
    acc = np.float32(-np.inf)
    for p in sorted(pairs, key=key):
        acc = _log_add_exp(acc, p[2])
    return o, c, _expf(np.float32(lp - acc))


def _prob2_map(meta, pairs, which):
    """Mode 12: the most likely entry of map `which` (0 object, 1 class) -> (id, log-probability, any entry, log normalisation)."""
    cached = (((meta >> 8) if which == 0 else (meta >> 16)) & 0xFF) - 1
    mine = [p for p in pairs if p[1] == which]
    if cached >= 0:
        best = (pairs[cached][0], pairs[cached][2], True)
    else:
        bid, blp, won = -1, np.float32(-np.inf), False
        for o, _, lp in pairs:
            if _ != which:
                continue
            if lp > blp:
                bid, blp, won = o, lp, True
            elif won and lp == blp and o < bid:
                bid = o
        best = (bid, blp, bool(mine))
    if not mine:
        return best + (np.float32(0),)
    mx = np.float32(-np.inf)
    for _, _, lp in mine:
        if lp > mx:
            mx = lp
    total = np.float32(0)
    for _, _, lp in sorted(mine, key=lambda p: p[0]):
        total = np.float32(total + _expf(np.float32(lp - mx)))
    return best + (np.float32(mx + _logf(total)),)


def _prob2_voxel(meta, pairs):
    """-> (object id, class id, confidence, object confidence, class confidence), float32 each as hv_semantic.h computes them."""
    o, c = _prob2_map(meta, pairs, 0), _prob2_map(meta, pairs, 1)
    marg = [np.float32(0) if (not m[2] or m[0] == -1) else _expf(np.float32(m[1] - m[3])) for m in (o, c)]
    if o[0] == -1 or c[0] == -1 or not o[2] or not c[2]:
        conf = np.float32(0)
    else:
        conf = _expf(np.float32(np.float32(o[1] + c[1]) - np.float32(o[3] + c[3])))
    return o[0], c[0], conf, marg[0], marg[1]


def _ratio(counter, count):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float32(counter) / np.float32(count)
    return np.float32(r if r < 1 else 1)


def unpack_reference(buf):
    """-> dict of per-block arrays in key order, comparable to the grids' dumps:
    keys [B,3]; mode 0: counts [B,nv] int32, sums [B,nv,6] float32 (dump());
    semantic: ints [B,nv,4] {count, object id, class id, confidence counter}, pos [B,nv,3] f64, col [B,nv,3] f32, conf [B,nv] f32, nlab
    [B,nv], labels [B,nv,254,2], logp [B,nv,254] (dump2(max_labels=254)), obj_conf / cls_conf [B,nv] f32 (dump_marginals()); and
    "stored" [B,nv] bool, "words" [B,nv,record words] for every mode."""
    h = check_reference(buf)
    mode, bs, B, N, P, o = h["mode"], h["block_size"], h["blocks"], h["voxels"], h["extra_pairs"], h["offsets"]
    nv, W, rw = bs ** 3, mask_words(bs), RECORD_BYTES[mode] // 4
    keys = np.frombuffer(buf, "<i4", 3 * B, o[0]).reshape(B, 3).astype(np.int32)
    masks = np.frombuffer(buf, "<u8", W * B, o[2]).reshape(B, W)
    stored = np.unpackbits(masks.view(np.uint8).reshape(B, W * 8), axis=1, bitorder="little").astype(bool)[:, :nv]
    words = np.zeros((B, nv, rw), np.uint32)
    words[stored] = np.frombuffer(buf, "<u4", N * rw, o[3]).reshape(N, rw)  # row-major over (block, k) = the record order
    out = {"keys": keys, "stored": stored, "words": words, "header": h}
    i32 = lambda a: a.view(np.int32)
    if mode == 0:
        out["counts"] = i32(words[..., 0]).copy()
        out["sums"] = words[..., 1:7].view(np.float32).copy()
        return out
    first = 4 if mode in (1, 11) else 2
    count = i32(words[..., 0])
    out["pos"] = np.ascontiguousarray(words[..., first:first + 6]).view(np.float64).reshape(B, nv, 3)
    out["col"] = words[..., first + 6:first + 9].view(np.float32).copy()
    ints = np.zeros((B, nv, 4), np.int32)
    ints[..., 0] = count
    conf, oc, cc = np.zeros((B, nv), np.float32), np.full((B, nv), -1, np.float32), np.full((B, nv), -1, np.float32)
    # (dump2 fills the slots behind a voxel's last pair with (-1, -1) and log-probability 0)
    nlab, labels, logp = np.zeros((B, nv), np.int32), np.full((B, nv, MAX_PAIRS, 2), -1, np.int32), np.zeros((B, nv, MAX_PAIRS), np.float32)
    if mode in (1, 11):
        ints[..., 1], ints[..., 2] = i32(words[..., 1]) - 1, i32(words[..., 2]) - 1
        a, c2 = i32(words[..., 3]), i32(words[..., 13])
        for b, k in zip(*np.nonzero(count)):
            if mode == 1:
                conf[b, k] = _ratio(a[b, k], count[b, k])
            else:
                oc[b, k], cc[b, k] = _ratio(a[b, k], count[b, k]), _ratio(c2[b, k], count[b, k])
                conf[b, k] = min(oc[b, k], cc[b, k])
        ints[..., 3] = a if mode == 1 else np.minimum(a, c2)
        if mode == 11:
            oc[count == 0], cc[count == 0] = 0, 0
    else:
        extras = np.frombuffer(buf, np.uint8, N, o[4]).astype(np.int64)
        start = np.concatenate([[0], np.cumsum(extras)])
        eo, ec = np.frombuffer(buf, "<i4", P, o[5]), np.frombuffer(buf, "<i4", P, o[6])
        el = np.frombuffer(buf, "<u4", P, o[7]).view(np.float32)
        ints[..., 1:3] = -1
        if mode == 12:
            oc[:], cc[:] = 0, 0
        for i, (b, k) in enumerate(zip(*np.nonzero(stored))):
            w = words[b, k]
            n = int(w[1] & 0xFF)
            assert extras[i] == max(n - INLINE, 0), (b, k, n, extras[i])
            pairs = [(int(i32(w[11 + j:12 + j])[0]), int(i32(w[17 + j:18 + j])[0]), w[23 + j:24 + j].view(np.float32)[0]) for j in range(min(n, INLINE))]
            pairs += [(int(eo[j]), int(ec[j]), el[j]) for j in range(start[i], start[i + 1])]
            nlab[b, k] = n
            for j, (po, pc, lp) in enumerate(pairs):
                labels[b, k, j], logp[b, k, j] = (po, pc), lp
            if mode == 2:
                ints[b, k, 1], ints[b, k, 2], conf[b, k] = _prob_voxel(int(w[1]), pairs)
            else:
                ints[b, k, 1], ints[b, k, 2], conf[b, k], oc[b, k], cc[b, k] = _prob2_voxel(int(w[1]), pairs)
            ints[b, k, 3] = np.int32(np.float32(conf[b, k] * np.float32(count[b, k])))
    out.update(ints=ints, conf=conf, nlab=nlab, labels=labels, logp=logp, obj_conf=oc, cls_conf=cc)
    return out


# ---- the corrupt buffers of the tests ----------------------------------------------------------------------------------------
def _patched(buf, at, fmt, value):
    out = bytearray(buf)
    struct.pack_into(fmt, out, at, value)
    return bytes(out)


def corrupt_buffers(buf):
    """A valid buffer with B >= 3 whose block 0 stores a voxel -> {name: (corrupt buffer, rule check_reference names)}: each violates
    that rule and no earlier one.  The extras cases are made for map modes with P >= 1 only; "high bit set" when bs^3 % 64 != 0."""
    h = header_reference(buf)
    mode, bs, B, N, P, o = h["mode"], h["block_size"], h["blocks"], h["voxels"], h["extra_pairs"], h["offsets"]
    assert B >= 3 and N >= 1
    W, nvox = mask_words(bs), bs ** 3
    key = lambda b: buf[o[0] + 12 * b:o[0] + 12 * (b + 1)]
    with_keys = lambda ks: buf[:o[0]] + b"".join(ks) + buf[o[0] + 12 * B:]
    keys = [key(b) for b in range(B)]
    off1 = struct.unpack_from("<Q", buf, o[1] + 8)[0]
    assert off1 >= 1  # block 0 stores a voxel
    word = next(w for w in range(W) if struct.unpack_from("<Q", buf, o[2] + 8 * w)[0])
    mask = struct.unpack_from("<Q", buf, o[2] + 8 * word)[0]
    other_mode = {0: 1, 1: 2, 2: 1, 11: 2, 12: 1}[mode]  # a mode with another record size
    out = {
        "wrong magic": (b"HVGRIDPX" + buf[8:], "magic"),
        "version 2": (_patched(buf, 8, "<I", 2), "version"),
        "header_bytes 128": (_patched(buf, 12, "<I", 128), "header_bytes"),
        "mode 3": (_patched(buf, 24, "<i", 3), "mode"),
        "block_size 17": (_patched(buf, 28, "<i", 17), "block_size"),
        "another mode's record size": (_patched(buf, 24, "<i", other_mode), "record_bytes"),
        "negative voxels": (_patched(buf, 56, "<q", -1), "negative"),
        "too many blocks": (_patched(buf, 48, "<q", len(buf)), "exceed"),
        "one byte cut off": (buf[:-1], "total_bytes"),
        "one byte appended": (buf + b"\0", "total_bytes"),
        "offset off 64": (_patched(buf, 80 + 8 * 3, "<Q", o[3] + 4), "aligned"),
        "section past the end": (_patched(buf, 80 + 8 * 3, "<Q", _align(len(buf))), "outside"),
        "records over masks": (_patched(buf, 80 + 8 * 3, "<Q", o[2]), "overlap"),
        "two keys swapped": (with_keys([keys[1], keys[0]] + keys[2:]), "ascending"),
        "duplicated key": (with_keys([keys[0], keys[0]] + keys[2:]), "ascending"),
        "key out of range": (_patched(buf, o[0] + 12 * (B - 1), "<i", KEY_BIAS), "out of range"),
        "offsets[0] != 0": (_patched(buf, o[1], "<Q", 1), "offsets[0]"),
        "decreasing offset": (_patched(buf, o[1] + 8 * 2, "<Q", off1 - 1), "decrease"),
        "offsets[B] != N": (_patched(buf, o[1] + 8 * B, "<Q", N + 1), "offsets[B]"),
        "mask bit flipped": (_patched(buf, o[2] + 8 * word, "<Q", mask & (mask - 1)), "popcount"),
    }
    if mode not in MAP_MODES:
        out["pairs without maps"] = (_patched(buf, 64, "<q", 1), "no maps")
    if nvox % 64:
        # move block 0's lowest stored bit of its last word above bs^3: same popcount, a bit out of range
        last = struct.unpack_from("<Q", buf, o[2] + 8 * (W - 1))[0]
        if last:
            out["high bit set"] = (_patched(buf, o[2] + 8 * (W - 1), "<Q", (last & (last - 1)) | (1 << 63)), "high bits")
    if mode in MAP_MODES and P >= 1:
        i = next(j for j in range(N) if buf[o[4] + j])
        out["extras entry 249"] = (_patched(buf, o[4] + i, "<B", 249), "extras entry")
        out["extras sum off"] = (_patched(buf, o[4] + i, "<B", buf[o[4] + i] - 1), "extras sum")
    return out
