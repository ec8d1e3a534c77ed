"""The packed TSDF map format of include/hipvol.h ("Packed maps"), restated in numpy - test infrastructure, no GPU.

A STATE here is (keys [U,3] int32, tsdf_bits [U,4096] uint32, weight [U,4096] uint32, sums [U,4096,3] uint32) in the library's
WORD order k = z * 256 + x * 16 + y (what export_numerators exposes); units in any order.  to_word_order() turns the dump()
order x * 256 + y * 16 + z into it.  state_of_planted() / state_of_volume() build a state from tests/planted_states.py states and
from a volume's own dump() + export_numerators(unit_keys()): the tsdf bit patterns come from dump(), which copies them; weights
and colour sums from the numerators, whose float32 values are exact integers below 2^24 for every planted state.
"""
import struct

import numpy as np

R = 16
NV = R ** 3
MASK_WORDS = NV // 32
MAGIC = b"HVTSDFPK"
VERSION = 1
HEADER_BYTES = 128
SECTIONS = ("keys", "offsets", "masks", "tsdf", "weight", "sum_r", "sum_g", "sum_b")
KEY_BIAS = 1 << 20
_HEADER = struct.Struct("<8sIIddiiqqq8Q")
assert _HEADER.size == HEADER_BYTES


def to_word_order(a):
    """[U, 4096, ...] in dump order (x * 256 + y * 16 + z) -> the same in word order (z * 256 + x * 16 + y)."""
    a = np.asarray(a)
    tail = a.shape[2:]
    axes = (0, 3, 1, 2) + tuple(range(4, 4 + len(tail)))
    return np.ascontiguousarray(a.reshape((a.shape[0], R, R, R) + tail).transpose(axes).reshape((a.shape[0], NV) + tail))


def state_of_planted(states):
    """tests/planted_states.py states (dump order, float weights, mean colours) -> a state as a volume holds them once planted."""
    from tests.planted_states import as_dump

    keys, tsdf, weight, colour = as_dump(states)
    w = to_word_order(weight).astype(np.uint32)
    sums = np.rint(to_word_order(colour) * to_word_order(weight)[..., None]).astype(np.uint32)
    return np.asarray(keys, np.int32), to_word_order(tsdf).view(np.uint32), w, sums


def state_of_volume(volume):
    """The state of a ScalableTSDFVolume from its own dump() and export_numerators(unit_keys())."""
    keys, tsdf, _, _ = volume.dump()
    ukeys = volume.unit_keys()
    num = volume.export_numerators(ukeys)
    order = np.lexsort((ukeys[:, 2], ukeys[:, 1], ukeys[:, 0]))
    assert np.array_equal(ukeys[order], keys)
    num = num[order]
    assert (num[..., 1:] == np.rint(num[..., 1:])).all() and num[..., 1:].max(initial=0) < 2 ** 24
    return keys, to_word_order(tsdf).view(np.uint32), num[..., 1].astype(np.uint32), num[..., 2:5].astype(np.uint32)


def _align(x):
    return (x + 63) & ~63


def section_sizes(U, N):
    return [12 * U, 8 * (U + 1), 4 * MASK_WORDS * U] + [4 * N] * 5


def layout(U, N):
    """-> (offsets of the eight sections, total_bytes): the sections in order, each on the next 64-byte boundary."""
    cur, offs = HEADER_BYTES, []
    for size in section_sizes(U, N):
        offs.append(cur)
        cur = _align(cur + size)
    return offs, cur


def pack_reference(keys, tsdf_bits, weight, sums, voxel_length=0.02, sdf_trunc=0.08):
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    U = len(keys)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    keys = keys[order]
    planes = np.stack([np.asarray(tsdf_bits, np.uint32).reshape(U, NV)[order], np.asarray(weight, np.uint32).reshape(U, NV)[order]]
                      + [np.asarray(sums, np.uint32).reshape(U, NV, 3)[order][..., c] for c in range(3)])  # [5, U, 4096]
    stored = (planes != 0).any(axis=0)  # [U, 4096]
    counts = stored.sum(axis=1).astype(np.uint64)
    offsets = np.concatenate([np.zeros(1, np.uint64), np.cumsum(counts, dtype=np.uint64)])
    N = int(offsets[-1])
    bits = stored.reshape(U, MASK_WORDS, 32).astype(np.uint64)
    masks = (bits << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    offs, total = layout(U, N)
    out = bytearray(total)
    out[:HEADER_BYTES] = _HEADER.pack(MAGIC, VERSION, HEADER_BYTES, voxel_length, sdf_trunc, R, 0, U, N, total, *offs)
    parts = [keys.astype("<i4"), offsets.astype("<u8"), masks.astype("<u4")] + [planes[p][stored].astype("<u4") for p in range(5)]
    for off, part in zip(offs, parts):
        raw = part.tobytes()
        out[off:off + len(raw)] = raw
    return bytes(out)


def header_reference(buf):
    """The header's fields as ScalableTSDFVolume.packed_info names them, plus "offsets" (no validation)."""
    f = _HEADER.unpack_from(buf, 0)
    return {"magic": f[0], "version": f[1], "header_bytes": f[2], "voxel_length": f[3], "sdf_trunc": f[4], "resolution": f[5],
            "units": f[7], "voxels": f[8], "bytes": f[9], "offsets": list(f[10:18])}


def check_reference(buf):
    """The rules of hv_tsdf_packed_check, in its order.  ValueError naming the first rule that fails; -> the header otherwise."""
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
    if h["resolution"] != R:
        raise ValueError("resolution")
    U, N = h["units"], h["voxels"]
    if U < 0 or N < 0:
        raise ValueError("negative")
    if U > len(buf) // 12 or N > len(buf) // 4:
        raise ValueError("exceed")
    if h["bytes"] != len(buf):
        raise ValueError("total_bytes")
    sizes = section_sizes(U, N)
    for off in h["offsets"]:
        if off % 64:
            raise ValueError("aligned")
    for off, size in zip(h["offsets"], sizes):
        if off < HEADER_BYTES or off + size > len(buf):
            raise ValueError("outside")
    for a in range(8):
        for b in range(a + 1, 8):
            oa, ob = h["offsets"][a], h["offsets"][b]
            if sizes[a] and sizes[b] and not (oa + sizes[a] <= ob or ob + sizes[b] <= oa):
                raise ValueError("overlap")
    keys = np.frombuffer(buf, "<i4", 3 * U, h["offsets"][0]).reshape(U, 3).astype(np.int64)
    offsets = np.frombuffer(buf, "<u8", U + 1, h["offsets"][1])
    masks = np.frombuffer(buf, "<u4", MASK_WORDS * U, h["offsets"][2]).reshape(U, MASK_WORDS)
    if ((keys < -KEY_BIAS) | (keys >= KEY_BIAS)).any():
        raise ValueError("out of range")
    for u in range(1, U):
        if not tuple(keys[u - 1]) < tuple(keys[u]):
            raise ValueError("ascending")
    if offsets[0] != 0:
        raise ValueError("offsets[0]")
    if (offsets[1:] < offsets[:-1]).any():
        raise ValueError("decrease")
    if int(offsets[U]) != N:
        raise ValueError("offsets[U]")
    pop = np.unpackbits(masks.view(np.uint8), axis=1).sum(axis=1).astype(np.uint64)
    if (pop != offsets[1:] - offsets[:-1]).any():
        raise ValueError("popcount")
    return h


# the words of the library's message that name each rule of check_reference
RULE_WORDS = {"header": "fewer than", "magic": "bad magic", "version": "unsupported version", "header_bytes": "header_bytes is",
              "resolution": "resolution is", "negative": "negative units", "exceed": "exceed what a buffer", "total_bytes": "total_bytes",
              "aligned": "not 64-byte aligned", "outside": "lies outside the buffer", "overlap": "overlap", "out of range": "out of range",
              "ascending": "not strictly ascending", "offsets[0]": "offsets[0] is", "decrease": "offsets decrease",
              "offsets[U]": "offsets[U]", "popcount": "mask popcount"}


def unpack_reference(buf):
    """-> (keys [U,3] int32, tsdf_bits, weight [U,4096] uint32, sums [U,4096,3] uint32) in word order, units in key order."""
    h = check_reference(buf)
    U, N = h["units"], h["voxels"]
    o = h["offsets"]
    keys = np.frombuffer(buf, "<i4", 3 * U, o[0]).reshape(U, 3).astype(np.int32)
    masks = np.frombuffer(buf, "<u4", MASK_WORDS * U, o[2]).reshape(U, MASK_WORDS)
    stored = np.unpackbits(masks.view(np.uint8), axis=1, bitorder="little").astype(bool)  # [U, 4096]: bit k & 31 of word k >> 5
    planes = np.zeros((5, U, NV), np.uint32)
    for p in range(5):
        planes[p][stored] = np.frombuffer(buf, "<u4", N, o[3 + p])  # row-major over (unit, word) = the record order
    return keys, planes[0], planes[1], np.stack([planes[2], planes[3], planes[4]], axis=-1)


# ---- the corrupt buffers of the tests ----------------------------------------------------------------------------------------
def _patched(buf, at, fmt, value):
    out = bytearray(buf)
    struct.pack_into(fmt, out, at, value)
    return bytes(out)


def corrupt_buffers(buf):
    """A valid buffer with U >= 3 whose unit 0 stores a voxel -> {name: (corrupt buffer, rule check_reference names)}."""
    h = header_reference(buf)
    U, N, o = h["units"], h["voxels"], h["offsets"]
    assert U >= 3 and N >= 1
    key = lambda u: buf[o[0] + 12 * u:o[0] + 12 * (u + 1)]
    with_keys = lambda ks: buf[:o[0]] + b"".join(ks) + buf[o[0] + 12 * U:]
    keys = [key(u) for u in range(U)]
    swapped = [keys[1], keys[0]] + keys[2:]
    doubled = [keys[0], keys[0]] + keys[2:]
    off1 = struct.unpack_from("<Q", buf, o[1] + 8)[0]
    assert off1 >= 1  # unit 0 stores a voxel, so offsets[1] can be moved below ... and a set mask bit can be cleared
    word = next(w for w in range(MASK_WORDS) if struct.unpack_from("<I", buf, o[2] + 4 * w)[0])
    mask = struct.unpack_from("<I", buf, o[2] + 4 * word)[0]
    return {
        "wrong magic": (b"HVTSDFPX" + buf[8:], "magic"),
        "version 2": (_patched(buf, 8, "<I", 2), "version"),
        "one byte cut off": (buf[:-1], "total_bytes"),
        "one byte appended": (buf + b"\0", "total_bytes"),
        "offset off 64": (_patched(buf, 64 + 8 * 3, "<Q", o[3] + 4), "aligned"),
        "two keys swapped": (with_keys(swapped), "ascending"),
        "duplicated key": (with_keys(doubled), "ascending"),
        "key out of range": (_patched(buf, o[0] + 12 * (U - 1), "<i", KEY_BIAS), "out of range"),
        "offsets[U] != N": (_patched(buf, o[1] + 8 * U, "<Q", N + 1), "offsets[U]"),
        "mask bit flipped": (_patched(buf, o[2] + 4 * word, "<I", mask & (mask - 1)), "popcount"),
        "decreasing offset": (_patched(buf, o[1] + 8 * 2, "<Q", off1 - 1), "decrease"),
    }
