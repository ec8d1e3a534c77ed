"""numpy restatement of hv_orb_detect (rules F1 - F11) and hv_match_descriptors (rules M1 - M5) of include/hipvol.h.  Integer
arithmetic throughout; the library is held to it bit for bit (tests/test_gpu_features.py).  The descriptor pattern comes from the
generator that also writes pyslam_amd/csrc/orb_pattern.h (tools/gen_orb_pattern.py)."""
import numpy as np

from tools import gen_orb_pattern as gp

RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2),
        (-1, -3))  # (dx, dy), F3
BORDER, CELL, MIN_SIDE = 16, 32, 33
PATTERN = np.array(gp.pattern(), np.int32)              # [256,4]
ROTATED = np.array(gp.rotated(gp.pattern()), np.int32)  # [32,256,4]
CX, CY = (np.array(t, np.int64) for t in gp.direction_tables())
_DY, _DX = np.mgrid[-15:16, -15:16]
DISC = (_DX * _DX + _DY * _DY) <= 225


def grey(image):
    """F1"""
    a = np.asarray(image)
    assert a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3))
    if a.ndim == 2:
        return a.astype(np.int32)
    c = a.astype(np.int32)
    return (c[..., 0] + 2 * c[..., 1] + c[..., 2] + 2) >> 2


def pyramid(g, levels):
    """F2: the levels that yield keypoints."""
    out = []
    for _ in range(levels):
        if g.shape[0] < MIN_SIDE or g.shape[1] < MIN_SIDE:
            break
        out.append(g)
        h, w = g.shape[0] // 2, g.shape[1] // 2
        g = (g[0:2 * h:2, 0:2 * w:2] + g[0:2 * h:2, 1:2 * w:2] + g[1:2 * h:2, 0:2 * w:2] + g[1:2 * h:2, 1:2 * w:2] + 2) >> 2
    return out


def capacity(height, width, levels, per_cell):
    """The bound the outputs are sized to: cells of the yielding levels times per_cell."""
    n = 0
    for _ in range(levels):
        if height < MIN_SIDE or width < MIN_SIDE:
            break
        n += ((height + CELL - 1) // CELL) * ((width + CELL - 1) // CELL) * per_cell
        height, width = height // 2, width // 2
    return n


def fast_score(g, t):
    """F3, F4: V [H,W] int32, 0 for a non-corner and outside the candidate region."""
    H, W = g.shape
    V = np.zeros((H, W), np.int32)
    b = BORDER
    c = g[b:H - b, b:W - b]
    ring = np.stack([g[b + dy:H - b + dy, b + dx:W - b + dx] for dx, dy in RING])
    bright, dark = ring - c > t, c - ring > t

    def arc(m):
        m2 = np.concatenate([m, m[:8]])
        hit = np.zeros(m.shape[1:], bool)
        for i in range(16):
            hit |= m2[i:i + 9].all(axis=0)
        return hit

    corner = arc(bright) | arc(dark)
    score = np.maximum((bright * (ring - c - t)).sum(axis=0), (dark * (c - ring - t)).sum(axis=0))
    V[b:H - b, b:W - b] = np.where(corner, score, 0)
    return V


def suppress(V):
    """F5: the survivors as a bool map."""
    H, W = V.shape
    P = np.zeros((H + 2, W + 2), V.dtype)
    P[1:-1, 1:-1] = V
    keep = V > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            n = P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            later = dy > 0 or (dy == 0 and dx > 0)
            keep &= (V > n) | ((V == n) & later)
    return keep


def select(V, keep, per_cell):
    """F6, F7 within one level: [(x, y, V)] in cell order, then rank."""
    H, W = V.shape
    out = []
    for cy in range(0, H, CELL):
        for cx in range(0, W, CELL):
            ys, xs = np.nonzero(keep[cy:cy + CELL, cx:cx + CELL])  # row-major: the index ascends
            if len(ys) == 0:
                continue
            v = V[cy + ys, cx + xs]
            order = np.argsort(-v, kind="stable")[:per_cell]
            out += [(cx + int(xs[k]), cy + int(ys[k]), int(v[k])) for k in order]
    return out


def moments(g, x, y):
    """F8: (m10, m01) of the disc around (x, y)."""
    patch = g[y - 15:y + 16, x - 15:x + 16].astype(np.int64) * DISC
    return int((patch * _DX).sum()), int((patch * _DY).sum())


def orientation_bin(m10, m01):
    return int(np.argmax(m10 * CX + m01 * CY))  # the first maximum: the smallest bin


def box5(g):
    """F9: s [H,W]; entries within 2 pixels of the edge are not defined (never read)."""
    H, W = g.shape
    s = np.zeros((H, W), np.int32)
    acc = np.zeros((H - 4, W - 4), np.int32)
    for dy in range(5):
        for dx in range(5):
            acc += g[dy:H - 4 + dy, dx:W - 4 + dx]
    s[2:H - 2, 2:W - 2] = acc
    return s


def describe(s, x, y, b):
    """F10, F11: 32 bytes."""
    p = ROTATED[b]
    bits = s[y + p[:, 1], x + p[:, 0]] < s[y + p[:, 3], x + p[:, 2]]
    return np.packbits(bits, bitorder="little")


def detect(image, levels=3, threshold=20, per_cell=8):
    """-> keypoints int32 [N,5] (x, y, level, score, bin), descriptors uint8 [N,32], in the F7 order."""
    kps, descs = [], []
    for level, g in enumerate(pyramid(grey(image), levels)):
        V = fast_score(g, threshold)
        chosen = select(V, suppress(V), per_cell)
        if not chosen:
            continue
        s = box5(g)
        for x, y, v in chosen:
            b = orientation_bin(*moments(g, x, y))
            kps.append((x, y, level, v, b))
            descs.append(describe(s, x, y, b))
    if not kps:
        return np.zeros((0, 5), np.int32), np.zeros((0, 32), np.uint8)
    return np.array(kps, np.int32), np.array(descs, np.uint8)


def level0_xy(keypoints):
    k = np.asarray(keypoints).astype(np.float64)
    scale = 2.0 ** k[:, 2]
    return np.stack([(k[:, 0] + 0.5) * scale - 0.5, (k[:, 1] + 0.5) * scale - 0.5], axis=1).astype(np.float32)


def hamming(query, train):
    """M1: [Nq,Nt] int32."""
    q = np.unpackbits(np.asarray(query, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    t = np.unpackbits(np.asarray(train, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    return (q @ (1.0 - t).T + (1.0 - q) @ t.T).astype(np.int32)  # (sums of at most 256 ones: exact in float32)


def match(query, train, offsets=None, max_distance=64, ratio_percent=80, cross_check=1):
    """M2 - M5 -> index int32 [S,Nq], distance uint16 [S,Nq], second uint16 [S,Nq], counts int32 [S]."""
    query, train = np.asarray(query, np.uint8).reshape(-1, 32), np.asarray(train, np.uint8).reshape(-1, 32)
    Nq, Nt = len(query), len(train)
    offsets = np.array([0, Nt] if offsets is None else offsets, np.int64)
    S = len(offsets) - 1
    D = hamming(query, train)
    owner = D.argmin(axis=0) if Nt else np.zeros(0, np.int64)  # M4: the smallest query index attaining each train's minimum
    index = np.full((S, Nq), -1, np.int32)
    distance = np.full((S, Nq), 65535, np.uint16)
    second = np.full((S, Nq), 65535, np.uint16)
    rows = np.arange(Nq)
    for s in range(S):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        if hi == lo:
            continue
        seg = D[:, lo:hi]
        j1 = seg.argmin(axis=1)
        d1 = seg[rows, j1]
        d2 = np.full(Nq, 65535, np.int32)
        if hi - lo > 1:
            rest = seg.copy()
            rest[rows, j1] = 1 << 20
            d2 = rest.min(axis=1)
        ok = d1 <= max_distance
        if ratio_percent != 0:
            ok &= 100 * d1.astype(np.int64) < ratio_percent * d2.astype(np.int64)
        if cross_check:
            ok &= owner[lo + j1] == rows
        index[s] = np.where(ok, lo + j1, -1)
        distance[s], second[s] = d1, d2
    return index, distance, second, (index >= 0).sum(axis=1).astype(np.int32)
