"""A numpy restatement of hv_tsdf_track_color (the hybrid contract in include/hipvol.h) - test infrastructure, no GPU.

Only what is photometric is here; the flow (association, the sums, the call's loop, the step-by-step checker) is the one of
tests/track_reference.py, handed the photometric term.  The model is whatever the caller hands in per pyramid level: (depth, world normal, mask, colour [h,w,3] float32 in [0, 1]) at the initial pose.  Source intensity, model
intensity and gradients are float32 in the kernels' operation order, the photometric term float64 in theirs, so per pixel both sides
agree bit for bit and the sums differ only by their summation order.
"""
import numpy as np

from tests import track_reference as tr

COLOR_TRACE_STRIDE = 58

_f32 = np.float32


def intensity_level0(rgb, bgr=False):
    """uint8 [h,w,3] -> float32 ((0.299f R + 0.587f G) + 0.114f B) / 255f."""
    c = np.asarray(rgb).astype(_f32)
    r, g, b = (c[..., 2], c[..., 1], c[..., 0]) if bgr else (c[..., 0], c[..., 1], c[..., 2])
    return (((_f32(0.299) * r + _f32(0.587) * g) + _f32(0.114) * b) / _f32(255)).astype(_f32)


def intensity_down(i):
    """level l -> l + 1: (((c0 + c1) + c2) + c3) * 0.25f over the children (2u,2v), (2u+1,2v), (2u,2v+1), (2u+1,2v+1)."""
    h, w = i.shape[0] // 2, i.shape[1] // 2
    s = ((i[0:2 * h:2, 0:2 * w:2] + i[0:2 * h:2, 1:2 * w:2]) + i[1:2 * h:2, 0:2 * w:2]) + i[1:2 * h:2, 1:2 * w:2]
    return (s * _f32(0.25)).astype(_f32)


def intensity_pyramid(rgb, n_levels, bgr=False):
    levels = [intensity_level0(rgb, bgr)]
    for _ in range(1, n_levels):
        levels.append(intensity_down(levels[-1]))
    return levels


def model_record(color, mdepth, mmask, trunc):
    """-> (I_m, g_x, g_y float32 [h,w], has-gradient bool [h,w]).  A pixel has a gradient iff it is off the border, the mask is set
    at it and its four neighbours and |z(neighbour) - z| <= trunc (float64 difference of the float32 depths); g = 0 elsewhere."""
    c = np.asarray(color, _f32)
    I = ((_f32(0.299) * c[..., 0] + _f32(0.587) * c[..., 1]) + _f32(0.114) * c[..., 2]).astype(_f32)
    h, w = I.shape
    gx, gy, ok = np.zeros((h, w), _f32), np.zeros((h, w), _f32), np.zeros((h, w), bool)
    if h < 3 or w < 3:
        return I, gx, gy, ok
    z = np.asarray(mdepth).astype(np.float64)
    m = np.asarray(mmask, bool)
    ctr = (slice(1, -1), slice(1, -1))
    nb = [(slice(1, -1), slice(2, None)), (slice(1, -1), slice(0, -2)), (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1))]
    good = m[ctr].copy()
    for s in nb:
        good &= m[s] & (np.abs(z[s] - z[ctr]) <= trunc)
    ok[ctr] = good
    gx[ctr] = np.where(good, _f32(0.5) * (I[nb[0]] - I[nb[1]]), _f32(0))
    gy[ctr] = np.where(good, _f32(0.5) * (I[nb[2]] - I[nb[3]]), _f32(0))
    return I, gx, gy, ok


def photometric(A, pc, K, Im, gx, gy, Is):
    """r_I and J_I of fixed associations: pc [N,3] source camera points; Im, gx, gy [N] the associated model records; Is [N] the
    source intensities.  The offsets x' - u', y' - v' follow from the projection of A pc and the model pixel round(x'), round(y')."""
    fx, fy, cx, cy = (float(k) for k in K)
    p = np.stack(tr.transform(A, pc[:, 0], pc[:, 1], pc[:, 2]), axis=1)
    xf, yf = fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy
    return _photometric(p, xf - np.floor(xf + 0.5), yf - np.floor(yf + 0.5), fx, fy, Im, gx, gy, Is)


def _photometric(p, dx, dy, fx, fy, Im, gx, gy, Is):
    Im, gx, gy, Is = (np.asarray(a).astype(np.float64) for a in (Im, gx, gy, Is))
    r = ((Im + gx * dx) + gy * dy) - Is
    a = gx * fx / p[:, 2]
    b = gy * fy / p[:, 2]
    c = -(a * p[:, 0] + b * p[:, 1]) / p[:, 2]
    J = np.stack([p[:, 1] * c - p[:, 2] * b, p[:, 2] * a - p[:, 0] * c, p[:, 0] * b - p[:, 1] * a, a, b, c], axis=1)
    return r, J


def term(isrc, K, record, lam, idelta):
    """-> the photometric term of one level for tr.linearise: (A, inliers of tr.associate) -> (r_I, J_I, w_I) of the inliers whose
    model pixel has a gradient.  isrc the level's source intensity, record = model_record(...) of its model."""
    I, gx, gy, ok = record

    def photometric_term(A, a):
        pk = ok[a["vi"], a["ui"]]
        p = np.stack(tr.transform(A, a["pc"][pk, 0], a["pc"][pk, 1], a["pc"][pk, 2]), axis=1)
        us, vs = a["ui"][pk], a["vi"][pk]
        rI, JI = _photometric(p, a["dx"][pk], a["dy"][pk], float(K[0]), float(K[1]), I[vs, us], gx[vs, us], gy[vs, us],
                              isrc[a["v"][pk], a["u"][pk]])
        return rI, JI, lam * tr.huber(rI, idelta)

    return photometric_term


def terms(rgb, n_levels, trunc, lam, idelta, bgr=False):
    """-> the photometric argument of tr.track and tr.check_call: (level, K_level, maps) -> term(...) of the level."""
    ints = intensity_pyramid(rgb, n_levels, bgr)
    return lambda level, Kl, maps: term(ints[level], Kl, model_record(maps[3], maps[0], maps[2], trunc), lam, idelta)


def linearise(src, isrc, model, K, A, R0, trunc, delta, lam, idelta, record=None):
    """tr.linearise of the combined system.  model = (depth, world normal, mask, colour); record = model_record(...) of it if
    already at hand."""
    if record is None:
        record = model_record(model[3], model[0], model[2], trunc)
    return tr.linearise(src, model, K, A, R0, trunc, delta, term(isrc, K, record, lam, idelta))


def track(depth, rgb, K, T_init, model, iterations=(10, 5, 4), depth_scale=1.0, depth_min=0.1, depth_max=3.0, trunc=0.07, delta=0.05,
          lam=0.01, idelta=0.1, bgr=False):
    """tr.track of the hybrid call.  model(level, K_level, h, w) -> (depth, world normal, mask, colour) of the map cast at T_init."""
    return tr.track(depth, K, T_init, model, iterations, depth_scale, depth_min, depth_max, trunc, delta,
                    terms(rgb, len(iterations), trunc, lam, idelta, bgr))


class Result:
    """track()'s dict in the shape of an OdometryResult, so that check_call can be held against the restatement's own call."""

    def __init__(self, out):
        self.transformation, self.information = out["T_cw"], out["information"]
        self.fitness, self.inlier_rmse, self.success = out["fitness"], out["inlier_rmse"], out["success"]
        self.iterations, self.degenerate, self.inliers, self.valid = out["iterations"], out["degenerate"], out["inliers"], out["valid"]
        self.photometric_inliers, self.intensity_rmse = out["photometric_inliers"], out["intensity_rmse"]
        self.trace = [dict(r) for r in out["trace"]]


def check_call(out, depth, rgb, K, T_init, model, iterations, depth_scale=1.0, depth_min=0.1, depth_max=3.0, trunc=0.07, delta=0.05,
               lam=0.01, idelta=0.1, bgr=False):
    """Hold one traced hv_tsdf_track_color result to this restatement, step by step: tr.check_call with the photometric term."""
    return tr.check_call(out, depth, K, T_init, model, iterations, depth_scale, depth_min, depth_max, trunc, delta,
                         terms(rgb, len(iterations), trunc, lam, idelta, bgr))
