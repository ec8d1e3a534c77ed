"""A numpy restatement of hv_tsdf_ray_cast (the contract in include/hipvol.h) - test infrastructure, no GPU.

Input is a dump() tuple of a TSDF volume (keys [U,3]; tsdf, weight [U,R^3] float32; colour [U,R^3,3] as the 0..255 running mean;
voxel order x * R^2 + y * R + z) and a pinhole camera.  Every ray is marched at once, one numpy pass per march step; the arithmetic
follows the kernel operation by operation in float32 (the normal in float64, as GetNormalAt), so the two agree to rounding of the
camera inverse and of the mean colour - what the GPU tests bound.
"""
import numpy as np

R = 16
# the named constants of include/hipvol.h (tests/test_raycast_reference_cpu.py checks that they match)
STEP_FRAC = 0.8
REFINE_ITERS = 4
UNIT_EPS = 0.01
ATTRIBUTES = ("depth", "vertex", "normal", "color", "mask")

_f32 = np.float32
_BIAS = 1 << 20


def _pack(x, y, z):
    return (x + _BIAS) | ((y + _BIAS) << 21) | ((z + _BIAS) << 42)


class _Grid:
    """The dumped units, looked up by unit index (vectorised)."""

    def __init__(self, dump):
        keys, tsdf, weight, colour = dump
        keys = np.asarray(keys, np.int64).reshape(-1, 3)
        codes = _pack(keys[:, 0], keys[:, 1], keys[:, 2])
        self.order = np.argsort(codes, kind="stable")
        self.codes = codes[self.order]
        self.tsdf = np.asarray(tsdf, np.float32).reshape(len(keys), -1)
        self.weight = np.asarray(weight, np.float32).reshape(len(keys), -1)
        self.colour = np.asarray(colour, np.float64).reshape(len(keys), -1, 3).astype(np.float32)

    def unit(self, ux, uy, uz):
        """-> dump row of each unit, -1 where absent."""
        ok = (ux >= -_BIAS) & (ux < _BIAS) & (uy >= -_BIAS) & (uy < _BIAS) & (uz >= -_BIAS) & (uz < _BIAS)
        out = np.full(ux.shape, -1, np.int64)
        if len(self.codes) == 0 or not ok.any():
            return out
        c = _pack(ux[ok], uy[ok], uz[ok])
        pos = np.minimum(np.searchsorted(self.codes, c), len(self.codes) - 1)
        out[ok] = np.where(self.codes[pos] == c, self.order[pos], -1)
        return out

    def locate(self, gx, gy, gz):
        """global voxel indices -> (dump row or -1, voxel index inside the unit)"""
        return self.unit(gx >> 4, gy >> 4, gz >> 4), ((gx & 15) * R + (gy & 15)) * R + (gz & 15)


def _corners():
    for i in range(8):
        yield i, int(i in (1, 2, 5, 6)), int(i in (2, 3, 6, 7)), int(i >= 4)


def _lerp(r, f):
    one = _f32(1)
    return (one - r[0]) * ((one - r[1]) * ((one - r[2]) * f[0] + r[2] * f[4]) + r[1] * ((one - r[2]) * f[3] + r[2] * f[7])) + \
        r[0] * ((one - r[1]) * ((one - r[2]) * f[1] + r[2] * f[5]) + r[1] * ((one - r[2]) * f[2] + r[2] * f[6]))


def _cell(p, vl):
    g = [(p[a] - _f32(0.5) * vl) / vl for a in range(3)]
    fl = [np.floor(x) for x in g]
    return [x.astype(np.int64) for x in fl], [g[a] - fl[a] for a in range(3)]


def _tri_tsdf(grid, p, vl, thr):
    """trilinear tsdf at p [3][n] float32 -> (valid, value)"""
    g0, r = _cell(p, vl)
    n = p[0].shape[0]
    valid = np.ones(n, bool)
    f = []
    for _i, sx, sy, sz in _corners():
        row, word = grid.locate(g0[0] + sx, g0[1] + sy, g0[2] + sz)
        rr = np.maximum(row, 0)
        valid &= (row >= 0) & (grid.weight[rr, word] > thr)
        f.append(np.where(row >= 0, grid.tsdf[rr, word], _f32(0)))
    return valid, _lerp(r, f)


def _color(grid, p, vl, thr):
    g0, r = _cell(p, vl)
    n = p[0].shape[0]
    valid = np.ones(n, bool)
    c = []
    for _i, sx, sy, sz in _corners():
        row, word = grid.locate(g0[0] + sx, g0[1] + sy, g0[2] + sz)
        rr = np.maximum(row, 0)
        valid &= (row >= 0) & (grid.weight[rr, word] > thr)
        c.append(np.where(valid[:, None], grid.colour[rr, word], _f32(0)))
    tri = np.stack([_lerp(r, [ci[:, k] for ci in c]) / _f32(255) for k in range(3)], axis=-1)
    gv = [np.floor(p[a] / vl).astype(np.int64) for a in range(3)]
    row, word = grid.locate(*gv)
    rr = np.maximum(row, 0)
    w = np.where(row >= 0, grid.weight[rr, word], _f32(0))
    near = np.where((w > 0)[:, None], grid.colour[rr, word] / _f32(255), _f32(0))
    return np.where(valid[:, None], tri, near).astype(np.float32)


def tsdf_at(grid, p, voxel_length):
    """GetTSDFAt (hv_tsdf_at) at p [n,3] float64: trilinear, no weights; a missing unit of p gives 0, missing neighbours 0."""
    vl = float(voxel_length)
    ul = vl * R
    p_locate = p - 0.5 * vl
    index0 = np.floor(p_locate / ul).astype(np.int64)
    p_grid = (p_locate - index0.astype(np.float64) * ul) / vl
    q = np.clip(np.floor(p_grid).astype(np.int64), 0, R - 1)
    r = p_grid - q
    own = grid.unit(index0[:, 0], index0[:, 1], index0[:, 2])
    f = []
    for _i, sx, sy, sz in _corners():
        x, y, z = q[:, 0] + sx, q[:, 1] + sy, q[:, 2] + sz
        row = grid.unit(index0[:, 0] + (x >= R), index0[:, 1] + (y >= R), index0[:, 2] + (z >= R))
        word = ((x & 15) * R + (y & 15)) * R + (z & 15)
        f.append(np.where(row >= 0, grid.tsdf[np.maximum(row, 0), word], np.float32(0)).astype(np.float64))
    r = [r[:, 0], r[:, 1], r[:, 2]]
    val = (1 - r[0]) * ((1 - r[1]) * ((1 - r[2]) * f[0] + r[2] * f[4]) + r[1] * ((1 - r[2]) * f[3] + r[2] * f[7])) + \
        r[0] * ((1 - r[1]) * ((1 - r[2]) * f[1] + r[2] * f[5]) + r[1] * ((1 - r[2]) * f[2] + r[2] * f[6]))
    return np.where(own >= 0, val, 0.0)


def normal_at(grid, p, voxel_length):
    """GetNormalAt: normalised central differences of tsdf_at at +/- 0.99 voxel (zero stays zero)."""
    h = 0.99 * float(voxel_length)
    nn = np.zeros_like(p)
    for i in range(3):
        e = np.zeros(3)
        e[i] = h
        nn[:, i] = tsdf_at(grid, p + e, voxel_length) - tsdf_at(grid, p - e, voxel_length)
    q = (nn * nn).sum(-1)
    s = np.sqrt(q)
    return np.where((q > 0)[:, None], nn / np.where(q > 0, s, 1.0)[:, None], nn)


def ray_cast(dump, voxel_length, sdf_trunc, intr, T_cw, height, width, depth_min=0.1, depth_max=3.0, weight_threshold=3.0,
             depth_scale=1.0, render_attributes=ATTRIBUTES):
    """-> dict like ScalableTSDFVolume.ray_cast (host arrays)."""
    grid = _Grid(dump)
    H, W = int(height), int(width)
    fx, fy, cx, cy = (_f32(x) for x in intr)
    T_wc = np.linalg.inv(np.asarray(T_cw, np.float64))
    rot = T_wc[:3, :3].astype(np.float32)
    orig = T_wc[:3, 3].astype(np.float32)
    vl, trunc = _f32(voxel_length), _f32(sdf_trunc)
    eps = _f32(UNIT_EPS) * vl
    zmin, zmax, thr = _f32(depth_min), _f32(depth_max), _f32(weight_threshold)
    max_steps = int(min(np.ceil(4.0 * (float(depth_max) - float(depth_min)) / float(voxel_length)), 1e8))

    v, u = np.mgrid[0:H, 0:W]
    dc0 = (u.reshape(-1).astype(np.float32) - cx) / fx
    dc1 = (v.reshape(-1).astype(np.float32) - cy) / fy
    d = [rot[a, 0] * dc0 + rot[a, 1] * dc1 + rot[a, 2] for a in range(3)]
    n = H * W
    z = np.full(n, zmin, np.float32)
    z_prev = np.zeros(n, np.float32)
    f_prev = np.zeros(n, np.float32)
    f_hit = np.zeros(n, np.float32)
    have_prev = np.zeros(n, bool)
    hit = np.zeros(n, bool)
    active = np.ones(n, bool)
    for _ in range(max_steps):
        active &= z < zmax
        ix = np.flatnonzero(active)
        if ix.size == 0:
            break
        zi = z[ix]
        di = [d[a][ix] for a in range(3)]
        p = [orig[a] + zi * di[a] for a in range(3)]
        gv = [np.floor(p[a] / vl).astype(np.int64) for a in range(3)]
        row, word = grid.locate(*gv)
        absent = row < 0
        # missing unit: to the exit of its box
        t = np.full(ix.size, np.inf, np.float32)
        for a in range(3):
            ub = gv[a] >> 4
            with np.errstate(divide="ignore", invalid="ignore"):
                hi = ((ub + 1) * R).astype(np.float32) * vl
                lo = (ub * R).astype(np.float32) * vl
                t = np.where(di[a] > 0, np.minimum(t, (hi - orig[a]) / di[a]),
                             np.where(di[a] < 0, np.minimum(t, (lo - orig[a]) / di[a]), t))
        rr = np.maximum(row, 0)
        w = grid.weight[rr, word]
        observed = ~absent & (w > thr)
        unobserved = ~absent & ~observed
        fv = grid.tsdf[rr, word]
        hp = have_prev[ix]
        hitnow = observed & hp & (f_prev[ix] > 0) & (fv <= 0)
        go = observed & ~hitnow
        step = np.where(fv > 0, np.maximum(vl, _f32(STEP_FRAC) * fv * trunc), vl)
        z_new = np.where(absent, np.maximum(t, zi) + eps, np.where(unobserved, zi + vl, np.where(go, zi + step, zi)))
        z[ix] = z_new
        have_prev[ix] = np.where(absent | unobserved, False, np.where(go, True, hp))
        z_prev[ix] = np.where(go, zi, z_prev[ix])
        f_prev[ix] = np.where(go, fv, f_prev[ix])
        hit[ix[hitnow]] = True
        f_hit[ix[hitnow]] = fv[hitnow]
        active[ix[hitnow]] = False

    # refinement of the hits
    hx = np.flatnonzero(hit)
    dh = [d[a][hx] for a in range(3)]

    def point(zz):
        return [orig[a] + zz * dh[a] for a in range(3)]

    za, fa, zb, fb = z_prev[hx].copy(), f_prev[hx].copy(), z[hx].copy(), f_hit[hx].copy()
    # each end one voxel outwards where the trilinear sample there is valid and of its sign, else in place (trilinear or nearest)
    za_out, zb_out = np.maximum(za - vl, zmin), np.minimum(zb + vl, zmax)
    ok_o, t_o = _tri_tsdf(grid, point(za_out), vl, thr)
    ok, t = _tri_tsdf(grid, point(za), vl, thr)
    out_a = ok_o & (t_o > 0)
    fa = np.where(out_a, t_o, np.where(ok & (t > 0), t, fa))
    za = np.where(out_a, za_out, za)
    ok_o, t_o = _tri_tsdf(grid, point(zb_out), vl, thr)
    ok, t = _tri_tsdf(grid, point(zb), vl, thr)
    out_b = ok_o & (t_o <= 0)
    fb = np.where(out_b, t_o, np.where(ok & (t <= 0), t, fb))
    zb = np.where(out_b, zb_out, zb)
    zs = zb.copy()
    side = np.zeros(hx.size, np.int8)
    alive = np.ones(hx.size, bool)
    for _ in range(REFINE_ITERS):
        zn = za + fa * (zb - za) / (fa - fb)
        zs = np.where(alive, zn, zs)
        ok, fs = _tri_tsdf(grid, point(zs), vl, thr)
        alive &= ok
        pos = alive & (fs > 0)
        neg = alive & ~(fs > 0)
        fb = np.where(pos & (side == 1), fb * _f32(0.5), fb)
        fa = np.where(neg & (side == -1), fa * _f32(0.5), fa)
        za, fa = np.where(pos, zs, za), np.where(pos, fs, fa)
        zb, fb = np.where(neg, zs, zb), np.where(neg, fs, fb)
        side = np.where(pos, 1, np.where(neg, -1, side)).astype(np.int8)

    ph = point(zs)
    out = {}
    attrs = tuple(render_attributes)
    if "depth" in attrs:
        out["depth"] = np.zeros(n, np.float32)
        out["depth"][hx] = zs * _f32(depth_scale)
        out["depth"] = out["depth"].reshape(H, W)
    if "vertex" in attrs:
        out["vertex"] = np.zeros((n, 3), np.float32)
        out["vertex"][hx] = np.stack(ph, axis=-1)
        out["vertex"] = out["vertex"].reshape(H, W, 3)
    if "normal" in attrs:
        out["normal"] = np.zeros((n, 3), np.float32)
        if hx.size:
            out["normal"][hx] = normal_at(grid, np.stack(ph, axis=-1).astype(np.float64), voxel_length).astype(np.float32)
        out["normal"] = out["normal"].reshape(H, W, 3)
    if "color" in attrs:
        out["color"] = np.zeros((n, 3), np.float32)
        if hx.size:
            out["color"][hx] = _color(grid, ph, vl, thr)
        out["color"] = out["color"].reshape(H, W, 3)
    if "mask" in attrs:
        out["mask"] = hit.reshape(H, W).copy()
    return out
