"""numpy restatement of the block grids' point lookup (include/hipvol.h, hv_lookup_points) on a grid's own dump - no GPU, no compiled
code.

A state is made from a dump: plain_state(VoxelBlockGrid.dump()) or semantic_state(grid.dump2()) (also the oracle grids' dump(), which
has the same leading five arrays).  lookup() then answers, point by point, exactly as the contract is written:

* own voxel: a float32 point is keyed in float32, floor(float32(p) * inv) with inv = float32(1) / float32(voxel); a float64 point in
  float64, floor(p * float64(inv)).  No voxel (LOOKUP_INVALID): a coordinate that is not finite, |p * inv| >= 1e9 (the plain grid
  forms the product in the point's dtype, the semantic grids in float64), a block key floor_div(v, bs) outside [-2^20, 2^20);
* qualifies: block held, count >= max(min_count, 1), semantic: float32 confidence >= float32 min_confidence;
* choice: the own voxel if it qualifies (OWN); else among the qualifying voxels at offsets [-r, r]^3, in offset-index order
  (dz + r)(2r + 1)^2 + (dy + r)(2r + 1) + (dx + r), the first with the smallest d2 = ((m0 - p0)^2 + (m1 - p1)^2) + (m2 - p2)^2 in
  float64 to the mean position m (NEAR); else MISSING;
* m: semantic float64 sum / float64(count); plain float32 sum / float32(count), widened.  colour: float32 sum / float32(count).

`variant=` names a WRONG reading of one rule (VARIANTS); tests/test_lookup_reference_cpu.py shows that the planted cases of
tests/lookup_cases.py tell each of them from the right one.
"""
import numpy as np

VARIANTS = ("nearest_by_centre", "own_not_first", "tie_last", "min_count_strict", "trunc_key", "f32_key_for_f64", "conf_strict")
MISSING, OWN, NEAR, INVALID = 0, 1, 2, 3
F32, F64 = np.float32, np.float64
KEY_LIMIT = 1 << 20


def plain_state(dump):
    keys, _, counts, sums = dump
    return dict(plain=True, keys=np.asarray(keys, np.int64), count=np.asarray(counts), pos=np.asarray(sums)[..., :3], col=np.asarray(sums)[..., 3:])


def semantic_state(dump):
    keys, ints, pos, col, conf = dump[:5]
    ints = np.asarray(ints)
    return dict(plain=False, keys=np.asarray(keys, np.int64), count=ints[..., 0], obj=ints[..., 1], cls=ints[..., 2], pos=np.asarray(pos),
                col=np.asarray(col), conf=np.asarray(conf, F32))


def _index(state, bs):
    """{voxel coordinate: (block, local index)} of the voxels with count >= 1."""
    if state.get("_index_bs") != bs:
        idx = {}
        B, L = np.nonzero(state["count"] >= 1)
        for b, l in zip(B.tolist(), L.tolist()):
            k = state["keys"][b]
            idx[(int(k[0]) * bs + l % bs, int(k[1]) * bs + (l // bs) % bs, int(k[2]) * bs + l // (bs * bs))] = (b, l)
        state["_index"], state["_index_bs"] = idx, bs
    return state["_index"]


def own_voxel(state, p, voxel, bs, variant=None):
    """p: one point [3] in ITS dtype -> voxel coordinate (3 ints), or None when the point has no voxel."""
    inv32 = F32(1.0) / F32(voxel)
    wide = p.dtype == F64 and variant != "f32_key_for_f64"
    with np.errstate(all="ignore"):
        x = p.astype(F64 if wide else F32)
        prod = x * (F64(inv32) if wide else inv32)
        if state["plain"]:
            ok = bool(np.all(np.isfinite(x)) and np.all(np.abs(prod) < (F64 if wide else F32)(1.0e9)))
        else:
            ok = bool(np.all(np.isfinite(p)) and np.all(np.abs(p.astype(F64) * F64(inv32)) < 1.0e9))
        if not ok:
            return None
        v = (np.trunc(prod) if variant == "trunc_key" else np.floor(prod)).astype(np.int64)
    b = v // bs
    if np.any(b < -KEY_LIMIT) or np.any(b >= KEY_LIMIT):
        return None
    return tuple(int(a) for a in v)


def _qualifies(state, at, min_count, min_confidence, variant):
    b, l = at
    c = int(state["count"][b, l])
    need = max(int(min_count), 1)
    if not (c > need if variant == "min_count_strict" else c >= need):
        return False
    if state["plain"]:
        return True
    conf, lim = F32(state["conf"][b, l]), F32(min_confidence)
    return bool(conf > lim if variant == "conf_strict" else conf >= lim)


def mean_position(state, at):
    b, l = at
    c = state["count"][b, l]
    if state["plain"]:
        return (state["pos"][b, l].astype(F32) / F32(c)).astype(F64)
    return state["pos"][b, l].astype(F64) / F64(c)


def lookup(state, points, voxel, bs, min_count=1, min_confidence=0.0, radius=0, variant=None):
    """-> dict(status u8 [n], count i32 [n], position f64 [n,3], color f32 [n,3], class_id / object_id i32 [n], confidence f32 [n]);
    the three label arrays are None for a plain state."""
    assert variant is None or variant in VARIANTS, variant
    if radius not in (0, 1, 2):
        raise ValueError(f"radius must be 0, 1 or 2, got {radius}")
    points = np.asarray(points)
    assert points.dtype in (np.dtype(F32), np.dtype(F64)) and points.ndim == 2 and points.shape[1] == 3
    n, r, w = len(points), int(radius), 2 * int(radius) + 1
    idx = _index(state, bs)
    sem = not state["plain"]
    out = dict(status=np.zeros(n, np.uint8), count=np.zeros(n, np.int32), position=np.zeros((n, 3), F64), color=np.zeros((n, 3), F32),
               class_id=np.full(n, -1, np.int32) if sem else None, object_id=np.full(n, -1, np.int32) if sem else None,
               confidence=np.zeros(n, F32) if sem else None)
    for i in range(n):
        p = points[i]
        v = own_voxel(state, p, voxel, bs, variant)
        if v is None:
            out["status"][i] = INVALID
            continue
        found, status = None, MISSING
        own = idx.get(v)
        if variant != "own_not_first" and own is not None and _qualifies(state, own, min_count, min_confidence, variant):
            found, status = own, OWN
        elif r > 0 or variant == "own_not_first":
            q = [float(a) for a in p.astype(F64)]
            best = None
            for c in range(w * w * w):
                d = (c % w - r, (c // w) % w - r, c // (w * w) - r)
                cv = (v[0] + d[0], v[1] + d[1], v[2] + d[2])
                if any(a // bs < -KEY_LIMIT or a // bs >= KEY_LIMIT for a in cv):
                    continue
                at = idx.get(cv)
                if at is None or not _qualifies(state, at, min_count, min_confidence, variant):
                    continue
                if variant == "nearest_by_centre":
                    m = [(a + 0.5) * float(voxel) for a in cv]
                else:
                    m = [float(a) for a in mean_position(state, at)]
                e0, e1, e2 = m[0] - q[0], m[1] - q[1], m[2] - q[2]
                d2 = (e0 * e0 + e1 * e1) + e2 * e2
                if best is None or (d2 <= best[0] if variant == "tie_last" else d2 < best[0]):
                    best = (d2, at, d)
            if best is not None:
                found, status = best[1], (OWN if best[2] == (0, 0, 0) else NEAR)
        out["status"][i] = status
        if found is None:
            continue
        b, l = found
        c = state["count"][b, l]
        out["count"][i] = c
        out["position"][i] = mean_position(state, found)
        out["color"][i] = state["col"][b, l].astype(F32) / F32(c)
        if sem:
            out["class_id"][i] = state["cls"][b, l]
            out["object_id"][i] = state["obj"][b, l]
            out["confidence"][i] = state["conf"][b, l]
    return out


FIELDS = ("status", "count", "position", "color", "class_id", "object_id", "confidence")


def same(a, b):
    """Bitwise equality of two lookup results (dicts, or objects with the fields as attributes); -> the first field that differs, or None."""
    get = lambda r, f: r[f] if isinstance(r, dict) else getattr(r, f)
    for f in FIELDS:
        x, y = get(a, f), get(b, f)
        if x is None or y is None:
            if x is not y:
                return f
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return f
    return None


def status_counts(status):
    """-> (points, own, near, missing, invalid), the order of LookupStats."""
    s = np.asarray(status)
    return (int(s.size), int((s == OWN).sum()), int((s == NEAR).sum()), int((s == MISSING).sum()), int((s == INVALID).sum()))
