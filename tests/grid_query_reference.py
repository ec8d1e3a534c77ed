"""numpy restatement of the VOXEL_GRID read / edit operations, on a grid's own dump() - no GPU, no compiled code.

dump = (keys [B,3] i32, hashes [B] u64, counts [B,bs^3] i32, sums [B,bs^3,6] f32), local index l = lx + ly*bs + lz*bs^2.

Restated from cpp/volumetric: voxel_block_grid.hpp (get_voxels, get_voxels_in_bb, iterate_voxels_in_camera_frustrum),
camera_frustrum.cpp (contains, frustum corners and bbox), voxel_grid_carving.h, voxel_data.h.  float32 and float64 sit exactly where
the reference has them:

* a row is sum / float32(count), one float32 division per component (0 / 0 = NaN: the release build has no zero-count check);
* the box / frustum-bbox bounds become voxel keys as floor(bound * float64(float32(1) / float32(voxel))), block keys by FLOOR division;
  a block outside the block range, then a voxel outside the voxel-key range, is skipped before any position is looked at;
* the box test is closed and done in float64 on the float32 position;
* the frustum test transforms the position in float64, (r0*x + r1*y + r2*z) + t, narrows the depth to float32 for the closed depth
  test, projects in float64, narrows u and v to float32: 0 <= u < W, 0 <= v < H;
* carve visits the frustum's voxels with count >= 1, reads the pixel (int)v, (int)u (truncation), skips image depths <= 0 or not
  finite and resets the voxel when float32 point_depth < float32(image_depth - threshold), strictly.

`variant=` names a WRONG reading of one of these rules (VARIANTS); tests use them to show that their inputs tell the right rule from
the wrong one.  classify() names, in float64, the decisions a case's voxels sit on.
"""
import numpy as np

VARIANTS = ("open_faces", "no_key_prefilter", "closed_image_edge", "open_depth_limits", "round_pixel", "transposed_pixel", "carve_le",
            "carve_ignores_invalid", "local_z_major", "min_count_strict", "trunc_div")

F32, F64 = np.float32, np.float64


def _check(variant):
    assert variant is None or variant in VARIANTS, variant


def positions(dump):
    """-> float32 [B, nvox, 6]: position and colour = sums / float32(count)."""
    _, _, counts, sums = dump
    with np.errstate(invalid="ignore", divide="ignore"):
        return sums / counts.astype(F32)[..., None]


def rows_of(dump, mask):
    r = positions(dump)[mask]
    return np.ascontiguousarray(r[:, :3]), np.ascontiguousarray(r[:, 3:])


def count_ok(dump, min_count, variant=None):
    c = dump[2]
    return c > min_count if variant == "min_count_strict" else c >= min_count


def inv_voxel(voxel):
    """The grid's float32 inv_voxel_size_ (1.0f / voxel_size), promoted to double where a double bound is keyed."""
    return F64(F32(1.0) / F32(voxel))


def voxel_keys(dump, bs, variant=None):
    """-> int64 [B, nvox, 3]: block key * bs + the local coordinates decoded from the local index."""
    keys = dump[0].astype(np.int64)
    l = np.arange(bs ** 3, dtype=np.int64)
    if variant == "local_z_major":
        loc = np.stack([l // (bs * bs), (l // bs) % bs, l % bs], axis=1)
    else:
        loc = np.stack([l % bs, (l // bs) % bs, l // (bs * bs)], axis=1)
    return keys[:, None, :] * bs + loc[None, :, :]


def key_range(bb, voxel, bs, variant=None):
    """-> (vmin, vmax, bmin, bmax), int64 [3] each."""
    bb = np.asarray(bb, F64)
    inv = inv_voxel(voxel)
    vmin = np.floor(bb[:3] * inv).astype(np.int64)
    vmax = np.floor(bb[3:] * inv).astype(np.int64)
    if variant == "trunc_div":
        div = lambda a: np.sign(a) * (np.abs(a) // bs)
    else:
        div = lambda a: a // bs
    return vmin, vmax, div(vmin), div(vmax)


def key_prefilter(dump, bb, voxel, bs, variant=None):
    """-> bool [B, nvox]: block inside the block range and voxel key inside the voxel-key range."""
    B, nvox = dump[2].shape
    if variant == "no_key_prefilter":
        return np.ones((B, nvox), bool)
    vmin, vmax, bmin, bmax = key_range(bb, voxel, bs, variant)
    keys = dump[0].astype(np.int64)
    block_ok = ((keys >= bmin) & (keys <= bmax)).all(axis=1)
    vk = voxel_keys(dump, bs, variant)
    return block_ok[:, None] & ((vk >= vmin) & (vk <= vmax)).all(axis=2)


def select_all(dump, min_count, variant=None):
    _check(variant)
    mask = count_ok(dump, min_count, variant)
    return (mask,) + rows_of(dump, mask)


def box_contains(p32, bb, variant=None):
    bb = np.asarray(bb, F64)
    p = p32.astype(F64)
    with np.errstate(invalid="ignore"):
        if variant == "open_faces":
            return ((p > bb[:3]) & (p < bb[3:])).all(axis=-1)
        return ((p >= bb[:3]) & (p <= bb[3:])).all(axis=-1)


def select_box(dump, bb, min_count, voxel, bs, variant=None):
    _check(variant)
    pos = positions(dump)[..., :3]
    mask = count_ok(dump, min_count, variant) & key_prefilter(dump, bb, voxel, bs, variant) & box_contains(pos, bb, variant)
    return (mask,) + rows_of(dump, mask)


def frustum_bbox(intr, W, H, T_cw, dmax, dmin):
    """World bbox [6] of the eight frustum corners, float64."""
    intr = np.asarray(intr, F32).astype(F64)
    T = np.asarray(T_cw, F64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    Rwc = R.T
    twc = -((Rwc[:, 0] * t[0] + Rwc[:, 1] * t[1]) + Rwc[:, 2] * t[2])
    lo, hi = np.full(3, np.finfo(F64).max), np.full(3, -np.finfo(F64).max)
    for cu, cv in ((0.0, 0.0), (F64(W), 0.0), (F64(W), F64(H)), (0.0, F64(H))):
        xn = (cu - intr[2]) / intr[0]
        yn = (cv - intr[3]) / intr[1]
        for d in (F64(F32(dmin)), F64(F32(dmax))):
            pc = np.array([xn * d, yn * d, d])
            w = ((Rwc[:, 0] * pc[0] + Rwc[:, 1] * pc[1]) + Rwc[:, 2] * pc[2]) + twc
            lo, hi = np.minimum(lo, w), np.maximum(hi, w)
    return np.concatenate([lo, hi])


def project(p32, intr, T_cw):
    """-> (pc float64 [...,3], u, v, depth float32 [...]) of float32 world points: CameraFrustrum::contains' arithmetic."""
    intr = np.asarray(intr, F32).astype(F64)
    T = np.asarray(T_cw, F64).reshape(4, 4)
    p = p32.astype(F64)
    pc = np.stack([((T[r, 0] * p[..., 0] + T[r, 1] * p[..., 1]) + T[r, 2] * p[..., 2]) + T[r, 3] for r in range(3)], axis=-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = (intr[0] * (pc[..., 0] / pc[..., 2]) + intr[2]).astype(F32)
        v = (intr[1] * (pc[..., 1] / pc[..., 2]) + intr[3]).astype(F32)
        depth = pc[..., 2].astype(F32)
    return pc, u, v, depth


def frustum_contains(p32, intr, W, H, T_cw, dmax, dmin, variant=None):
    """-> (inside bool, u, v, depth)."""
    _, u, v, depth = project(p32, intr, T_cw)
    dmax, dmin = F32(dmax), F32(dmin)
    with np.errstate(invalid="ignore"):
        if variant == "open_depth_limits":
            in_depth = (depth > dmin) & (depth < dmax)
        else:
            in_depth = (depth >= dmin) & (depth <= dmax)
        if variant == "closed_image_edge":
            in_image = (u >= 0) & (u <= F32(W)) & (v >= 0) & (v <= F32(H))
        else:
            in_image = (u >= 0) & (u < F32(W)) & (v >= 0) & (v < F32(H))
    return in_depth & in_image, u, v, depth


def select_frustum(dump, intr, W, H, T_cw, dmax, dmin, min_count, voxel, bs, variant=None):
    _check(variant)
    pos = positions(dump)[..., :3]
    bb = frustum_bbox(intr, W, H, T_cw, dmax, dmin)
    inside = frustum_contains(pos, intr, W, H, T_cw, dmax, dmin, variant)[0]
    mask = count_ok(dump, min_count, variant) & key_prefilter(dump, bb, voxel, bs, variant) & inside
    return (mask,) + rows_of(dump, mask)


def pixel_index(u, v, W, H, variant=None):
    """Flat index into the H x W depth image of float32 (u, v) inside the image; a variant's index is clamped into the buffer."""
    with np.errstate(invalid="ignore"):
        if variant == "round_pixel":
            iu = np.clip(np.rint(u), 0, W - 1).astype(np.int64)
            iv = np.clip(np.rint(v), 0, H - 1).astype(np.int64)
        else:
            iu, iv = np.trunc(u).astype(np.int64), np.trunc(v).astype(np.int64)
    idx = iu * H + iv if variant == "transposed_pixel" else iv * W + iu
    return np.clip(idx, 0, W * H - 1) if variant is not None else idx


def _reset(dump, where):
    keys, hashes, counts, sums = dump
    counts, sums = counts.copy(), sums.copy()
    counts[where] = 0
    sums[where] = 0.0
    return keys, hashes, counts, sums


def carve_decisions(dump, intr, W, H, T_cw, dmax, dmin, depth, threshold, voxel, bs, variant=None):
    """-> (visited [B,nvox] bool, image_depth [n] f32, point_depth [n] f32, valid [n] bool, reset [n] bool) over the n visited voxels."""
    pos = positions(dump)[..., :3]
    visited = select_frustum(dump, intr, W, H, T_cw, dmax, dmin, 1, voxel, bs, variant)[0]
    _, u, v, pd = frustum_contains(pos[visited], intr, W, H, T_cw, dmax, dmin, variant)
    image = np.ascontiguousarray(depth, F32).reshape(-1)[pixel_index(u, v, W, H, variant)]
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.ones(len(image), bool) if variant == "carve_ignores_invalid" else (image > 0) & np.isfinite(image)
        limit = image - F32(threshold)  # float32 arithmetic
        reset = valid & ((pd <= limit) if variant == "carve_le" else (pd < limit))
    return visited, image, pd, valid, reset


def carve(dump, intr, W, H, T_cw, dmax, dmin, depth, threshold, voxel, bs, variant=None):
    """-> the dump after carve(frustum, depth image [H,W] f32, threshold)."""
    _check(variant)
    visited, _, _, _, reset = carve_decisions(dump, intr, W, H, T_cw, dmax, dmin, depth, threshold, voxel, bs, variant)
    where = np.zeros_like(visited)
    where[visited] = reset
    return _reset(dump, where)


def remove_low_count(dump, min_count, variant=None):
    """-> the dump after remove_low_count_voxels(min_count): every voxel with count < min_count is reset, blocks stay."""
    _check(variant)
    return _reset(dump, ~count_ok(dump, min_count, variant))


# ---- which decision a voxel sits on ---------------------------------------------------------------------------------------------
CLASSES = ("box_face_on", "box_face_ulp_inside", "box_face_ulp_outside", "box_pos_in_key_out", "box_key_in_pos_out", "image_edge",
           "depth_limit", "pc_z_zero", "carve_on_threshold", "carve_invalid_pixel")


def _next32(x, toward):
    return np.nextafter(x.astype(F32), F32(toward))


def classify_box(dump, bb, voxel, bs):
    """-> {class: bool [B,nvox]} over the observed voxels (count > 0), for a box query."""
    bb = np.asarray(bb, F64)
    obs = dump[2] > 0
    pos = positions(dump)[..., :3]
    p = pos.astype(F64)
    lo, hi = bb[:3], bb[3:]
    with np.errstate(invalid="ignore"):
        on = (p == lo) | (p == hi)
        up, down = _next32(pos, np.inf).astype(F64), _next32(pos, -np.inf).astype(F64)
        ulp_in = ((p > lo) & (down <= lo)) | ((p < hi) & (up >= hi))
        ulp_out = ((p < lo) & (up >= lo)) | ((p > hi) & (down <= hi))
        others_in = np.stack([np.delete((p >= lo) & (p <= hi), a, axis=-1).all(axis=-1) for a in range(3)], axis=-1)
    inside = box_contains(pos, bb)
    pre = key_prefilter(dump, bb, voxel, bs)
    return {
        "box_face_on": obs & (on & others_in).any(axis=-1),
        "box_face_ulp_inside": obs & (ulp_in & ~on & others_in).any(axis=-1),
        "box_face_ulp_outside": obs & (ulp_out & others_in).any(axis=-1),
        "box_pos_in_key_out": obs & inside & ~pre,
        "box_key_in_pos_out": obs & pre & ~inside,
    }


def classify_frustum(dump, intr, W, H, T_cw, dmax, dmin, voxel, bs, depth=None, threshold=None):
    """-> {class: bool [B,nvox]} over the observed voxels for a frustum query; with a depth image, for a carve."""
    obs = dump[2] > 0
    pos = positions(dump)[..., :3]
    pc, u, v, d = project(pos, intr, T_cw)
    dmax, dmin = F32(dmax), F32(dmin)
    with np.errstate(invalid="ignore"):
        in_depth = (d >= dmin) & (d <= dmax)
        edge = lambda x, n: (x == 0) | (x == F32(n)) | (x == np.nextafter(F32(n), F32(0)))
        out = {
            "image_edge": obs & in_depth & (edge(u, W) | edge(v, H)),
            "depth_limit": obs & ((d == dmin) | (d == dmax) | (d == np.nextafter(dmin, F32(-np.inf))) | (d == np.nextafter(dmax, F32(np.inf)))),
            "pc_z_zero": obs & (pc[..., 2] == 0),
        }
    if depth is not None:
        visited, image, pd, valid, _ = carve_decisions(dump, intr, W, H, T_cw, dmax, dmin, depth, threshold, voxel, bs)
        with np.errstate(invalid="ignore", over="ignore"):
            on = valid & (pd == image - F32(threshold))
        for name, flag in (("carve_on_threshold", on), ("carve_invalid_pixel", ~valid)):
            m = np.zeros_like(visited)
            m[visited] = flag
            out[name] = m
    return out


def classify(dump, step, voxel, bs):
    """-> {class: bool [B,nvox]} for one step of a case (tests/grid_query_cases.py); {} for a step that decides nothing geometric."""
    kind = step[0]
    if kind == "box":
        return classify_box(dump, step[1], voxel, bs)
    if kind == "frustum":
        f = step[1]
        return classify_frustum(dump, f["intr"], f["W"], f["H"], f["T_cw"], f["dmax"], f["dmin"], voxel, bs)
    if kind == "carve":
        f = step[1]
        return classify_frustum(dump, f["intr"], f["W"], f["H"], f["T_cw"], f["dmax"], f["dmin"], voxel, bs, step[2], step[3])
    return {}


def apply_step(dump, step, voxel, bs, variant=None):
    """One step of a case on a dump -> ("rows", mask, points, colors) for a query, ("dump", new dump) for an edit, None for a step the
    restatement does not model (integrate)."""
    kind = step[0]
    if kind == "all":
        return ("rows",) + select_all(dump, step[1], variant)
    if kind == "box":
        return ("rows",) + select_box(dump, step[1], step[2], voxel, bs, variant)
    if kind == "frustum":
        f = step[1]
        return ("rows",) + select_frustum(dump, f["intr"], f["W"], f["H"], f["T_cw"], f["dmax"], f["dmin"], step[2], voxel, bs, variant)
    if kind == "carve":
        f = step[1]
        return ("dump", carve(dump, f["intr"], f["W"], f["H"], f["T_cw"], f["dmax"], f["dmin"], step[2], step[3], voxel, bs, variant))
    if kind == "remove":
        return ("dump", remove_low_count(dump, step[1], variant))
    return None
