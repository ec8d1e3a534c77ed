"""numpy restatement of volume-to-volume fusion (include/hipvol.h, hv_tsdf_integrate_volume) on dump() tuples - test
infrastructure, no GPU.

The arithmetic follows the contract operation by operation in float64 (every product and sum its own numpy call: nothing is
contracted), so a dump produced here and the library's are meant to agree bit for bit; where a decision sits on a boundary of the
rules (some component of r within 1e-9 of 0, 0.5 or 1) the voxel is marked FRAGILE for the tests that compare two implementations.
Colour sums are recovered from the dumps' running means (sum = rint(mean * weight), exact for integer sums below 2^32) and handed back
as means again, the way hv_tsdf_dump does it.
"""
import numpy as np

from tests import raycast_reference as rr

R = 16
NV = R ** 3
FRAGILE_BAND = 1e-9
_LX, _LY, _LZ = (a.reshape(-1) for a in np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij"))  # x * 256 + y * 16 + z


def check_rigid(T):
    """The contract's argument checks -> None or the reason T is refused."""
    T = np.asarray(T, np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        return "not finite"
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        return "bottom row"
    Rm = T[:3, :3]
    if np.abs(Rm.T @ Rm - np.eye(3)).sum(axis=1).max() > 1e-6 or np.linalg.det(Rm) < 0:
        return "not rigid"
    return None


def locate(T, gi, voxel_length):
    """Destination voxels (global indices gi [..., 3] int64) -> (g0 [3][...] int64, r [3][...] float64, ok [...]): the contract's
    `locate` step, in its order."""
    T = np.asarray(T, np.float64)
    vl = np.float64(voxel_length)
    d = [(gi[..., a].astype(np.float64) + 0.5) * vl - T[a, 3] for a in range(3)]
    g0, r = [], []
    ok = np.ones(gi.shape[:-1], bool)
    for a in range(3):
        p = (T[0, a] * d[0] + T[1, a] * d[1]) + T[2, a] * d[2]
        g = p / vl - 0.5
        with np.errstate(invalid="ignore"):
            ok &= np.abs(g) < 1.0e9
        f = np.floor(g)
        g0.append(np.where(ok, f, 0.0).astype(np.int64))
        r.append(g - f)
    return g0, r, ok


def _lerp(r, f):
    return (1 - r[0]) * ((1 - r[1]) * ((1 - r[2]) * f[0] + r[2] * f[4]) + r[1] * ((1 - r[2]) * f[3] + r[2] * f[7])) + \
        r[0] * ((1 - r[1]) * ((1 - r[2]) * f[1] + r[2] * f[5]) + r[1] * ((1 - r[2]) * f[2] + r[2] * f[6]))


def candidate_units(src_keys, T, voxel_length):
    """Destination units that can hold a voxel whose nearest source voxel lies in one of the source units `src_keys` [n,3]: the
    bounding boxes of the transformed unit boxes, padded by 1e-3 voxel.  -> unique [m,3] int64 (a superset; the rules decide)."""
    T = np.asarray(T, np.float64)
    k = np.asarray(src_keys, np.int64).reshape(-1, 3)
    if len(k) == 0:
        return np.zeros((0, 3), np.int64)
    L = float(voxel_length) * R
    corners = np.stack([(k + np.array([c & 1, (c >> 1) & 1, c >> 2])) * L for c in range(8)], axis=1)  # [n,8,3]
    q = corners @ T[:3, :3].T + T[:3, 3]
    lo = np.floor(np.ceil(q.min(1) / voxel_length - 0.5 - 1e-3) / R).astype(np.int64)
    hi = np.floor(np.floor(q.max(1) / voxel_length - 0.5 + 1e-3) / R).astype(np.int64)
    assert (hi - lo).max() <= 2
    out = []
    for i in range(3):
        for j in range(3):
            for l in range(3):
                u = lo + np.array([i, j, l])
                out.append(u[np.all(u <= hi, axis=1)])
    u = np.unique(np.concatenate(out), axis=0)
    return u[np.all((u >= -rr._BIAS) & (u < rr._BIAS), axis=1)]


def sample_units(src_dump, T, voxel_length, unit_keys, chunk=64):
    """The contract's locate + sample for every voxel of the destination units `unit_keys` [m,3].
    -> dict of [m, 4096] arrays: w_s (float64, 0 = not touched), tsdf_s (float64), gain [m,4096,3] (float64 integers),
    trilinear (bool), fragile (bool)."""
    keys = np.asarray(unit_keys, np.int64).reshape(-1, 3)
    m = len(keys)
    out = {"w_s": np.zeros((m, NV)), "tsdf_s": np.zeros((m, NV)), "gain": np.zeros((m, NV, 3)), "trilinear": np.zeros((m, NV), bool),
           "fragile": np.zeros((m, NV), bool)}
    if m == 0:
        return out
    grid = rr._Grid(src_dump)
    colour = np.asarray(src_dump[3], np.float64).reshape(len(grid.codes), -1, 3)
    local = np.stack([_LX, _LY, _LZ], axis=-1)
    for lo in range(0, m, chunk):
        sel = slice(lo, min(lo + chunk, m))
        gi = keys[sel][:, None, :] * R + local[None, :, :]
        g0, r, ok = locate(T, gi, voxel_length)
        near = [g0[a] + (r[a] >= 0.5) for a in range(3)]
        row, word = grid.locate(*near)
        wn = np.where(ok & (row >= 0), grid.weight[np.maximum(row, 0), word], np.float32(0)).astype(np.float64)
        frag = np.zeros(wn.shape, bool)
        for a in range(3):
            frag |= (np.abs(r[a]) < FRAGILE_BAND) | (np.abs(r[a] - 0.5) < FRAGILE_BAND) | (np.abs(r[a] - 1.0) < FRAGILE_BAND)
        out["fragile"][sel] = frag
        upd = wn > 0
        ix = np.nonzero(upd)
        if ix[0].size == 0:
            continue
        g0u, ru = [x[ix] for x in g0], [x[ix] for x in r]
        wnu = wn[ix]
        all8 = np.ones(wnu.shape, bool)
        f_t, f_c = [], []
        for _i, sx, sy, sz in rr._corners():
            crow, cword = grid.locate(g0u[0] + sx, g0u[1] + sy, g0u[2] + sz)
            rr_ = np.maximum(crow, 0)
            cw = np.where(crow >= 0, grid.weight[rr_, cword], np.float32(0)).astype(np.float64)
            all8 &= cw > 0
            f_t.append(grid.tsdf[rr_, cword].astype(np.float64))
            f_c.append(colour[rr_, cword])
        nrow, nword = row[ix], word[ix]
        ts = np.where(all8, _lerp(ru, f_t), grid.tsdf[nrow, nword].astype(np.float64))
        mean = np.stack([np.where(all8, _lerp(ru, [c[:, k] for c in f_c]), colour[nrow, nword, k]) for k in range(3)], axis=-1)
        full = (ix[0] + lo, ix[1])
        out["w_s"][full] = wnu
        out["tsdf_s"][full] = ts
        out["gain"][full] = np.floor(mean * wnu[:, None] + 0.5)
        out["trilinear"][full] = all8
    return out


def merge_reference(dst_dump, src_dump, T, voxel_length, detail=False):
    """-> (dump of the destination after the call, (units_source, units_claimed, voxels_updated, voxels_trilinear, voxels_nearest))
    and, with detail=True, a dict {keys [K,3] of the units sampled, updated, trilinear, fragile [K,4096]} as third item."""
    dkeys, dtsdf, dweight, dcolour = (np.asarray(x) for x in dst_dump)
    skeys, _stsdf, sweight, _scolour = (np.asarray(x) for x in src_dump)
    dkeys = dkeys.reshape(-1, 3).astype(np.int64)
    nd = len(dkeys)
    held = sweight.reshape(len(skeys), -1).max(axis=1) > 0 if len(skeys) else np.zeros(0, bool)
    cand = candidate_units(skeys.reshape(-1, 3)[held], T, voxel_length)
    s = sample_units(src_dump, T, voxel_length, cand)
    keep = (s["w_s"] > 0).any(axis=1)
    kept = cand[keep]
    w_s, tsdf_s, gain, tri = s["w_s"][keep], s["tsdf_s"][keep], s["gain"][keep], s["trilinear"][keep]
    stats_vox = (int((w_s > 0).sum()), int(tri.sum()), int(((w_s > 0) & ~tri).sum()))
    # the destination's units: former ones first, then the new ones; rows of the kept units in that list
    index = {tuple(k): i for i, k in enumerate(dkeys.tolist())}
    rows = np.array([index.setdefault(tuple(k), len(index)) for k in kept.tolist()], np.int64)
    n = len(index)
    keys = np.zeros((n, 3), np.int64)
    keys[:nd] = dkeys
    if len(kept):
        keys[rows] = kept
    tsdf = np.zeros((n, NV), np.float32)
    weight = np.zeros((n, NV), np.float64)
    sums = np.zeros((n, NV, 3), np.float64)
    tsdf[:nd] = dtsdf.reshape(nd, NV)
    weight[:nd] = dweight.reshape(nd, NV)
    sums[:nd] = np.rint(np.asarray(dcolour, np.float64).reshape(nd, NV, 3) * weight[:nd, :, None])
    if len(kept):
        t0, w0 = tsdf[rows].astype(np.float64), weight[rows]
        w1 = w0 + w_s
        upd = w_s > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            t1 = ((t0 * w0 + tsdf_s * w_s) / w1).astype(np.float32)
        tsdf[rows] = np.where(upd, t1, tsdf[rows])
        weight[rows] = w1
        sums[rows] = sums[rows] + gain
    with np.errstate(invalid="ignore", divide="ignore"):
        colour = np.where(weight[..., None] > 0, sums / weight[..., None], 0.0)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    dump = (keys[order].astype(np.int32), tsdf[order], weight[order].astype(np.float32), colour[order])
    stats = (int(held.sum()), n - nd, stats_vox[0], stats_vox[1], stats_vox[2])
    if not detail:
        return dump, stats
    return dump, stats, {"keys": cand, "updated": s["w_s"] > 0, "trilinear": s["trilinear"], "fragile": s["fragile"]}


def empty_dump():
    return (np.zeros((0, 3), np.int32), np.zeros((0, NV), np.float32), np.zeros((0, NV), np.float32), np.zeros((0, NV, 3), np.float64))
