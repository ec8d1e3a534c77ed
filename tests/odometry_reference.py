"""A numpy restatement of hv_rgbd_odometry (the contract in include/hipvol.h) - test infrastructure, no GPU.

Frame-to-frame alignment is the tracker's schedule with another model: what tests/track_reference.py and
tests/track_color_reference.py restate (source pyramid, level intrinsics, association, linearisation, the sums, the solve, the
stopping rule) is used from there, with R0 = identity.  What is new is here: the target model built from the second frame
(target_model), the call with its state A = T_target_source starting at T_init (odometry), and the step-by-step checker (check_call;
tr.check_call derives R0 and the result pose from T_init and cannot serve).  float32 pyramids and records, float64 geometry in the
kernels' operation order: per pixel both sides agree bit for bit, the sums differ only by their summation order.
"""
import numpy as np

from tests import track_color_reference as tc
from tests import track_reference as tr

_f32 = np.float32


def target_model(z, intensity, K, trunc):
    """One level's model from the target frame.  z [h,w] float32 (0 = invalid), intensity [h,w] float32 or None, K the level's
    (fx, fy, cx, cy).  -> dict(depth = z, normal [h,w,3] float32, mask [h,w] bool, record [h,w,4] float32 or None).
    mask: off the border, z > 0 at the pixel and its four neighbours, |z(nb) - z| <= trunc (float64), and the cross product of the
    central differences of the back-projected points has a finite length > 0; the normal is that product normalised, facing the
    camera; record = {I, g_x, g_y, has-gradient}, gradient and flag only where the mask is set."""
    z = np.asarray(z, _f32)
    h, w = z.shape
    fx, fy, cx, cy = (float(k) for k in K)
    normal = np.zeros((h, w, 3), _f32)
    mask = np.zeros((h, w), bool)
    record = None
    if intensity is not None:
        record = np.zeros((h, w, 4), _f32)
        record[..., 0] = np.asarray(intensity, _f32)
    if h < 3 or w < 3:
        return {"depth": z, "normal": normal, "mask": mask, "record": record}
    zd = z.astype(np.float64)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    P = np.stack([zd * ((u - cx) / fx), zd * ((v - cy) / fy), zd], axis=-1)
    ctr = (slice(1, -1), slice(1, -1))
    nb = [(slice(1, -1), slice(2, None)), (slice(1, -1), slice(0, -2)), (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1))]
    ok = z[ctr] > 0
    for s in nb:
        ok &= (z[s] > 0) & (np.abs(zd[s] - zd[ctr]) <= trunc)
    dx, dy = P[nb[0]] - P[nb[1]], P[nb[2]] - P[nb[3]]
    c = np.stack([dy[..., 1] * dx[..., 2] - dy[..., 2] * dx[..., 1], dy[..., 2] * dx[..., 0] - dy[..., 0] * dx[..., 2],
                  dy[..., 0] * dx[..., 1] - dy[..., 1] * dx[..., 0]], axis=-1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        length = np.sqrt((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2])
        ok &= np.isfinite(length) & (length > 0)
        n = c / length[..., None]
        Pc = P[ctr]
        flip = (n[..., 0] * Pc[..., 0] + n[..., 1] * Pc[..., 1]) + n[..., 2] * Pc[..., 2] > 0
        n = np.where(flip[..., None], -n, n)
        normal[ctr] = np.where(ok[..., None], n, 0.0).astype(_f32)
    mask[ctr] = ok
    if record is not None:
        I = record[..., 0]
        record[..., 1][ctr] = np.where(ok, _f32(0.5) * (I[nb[0]] - I[nb[1]]), _f32(0))
        record[..., 2][ctr] = np.where(ok, _f32(0.5) * (I[nb[2]] - I[nb[3]]), _f32(0))
        record[..., 3][ctr] = ok.astype(_f32)
    return {"depth": z, "normal": normal, "mask": mask, "record": record}


def model_level(target_depth, target_rgb, K, level, depth_scale=1.0, depth_min=0.1, depth_max=3.0, trunc=0.07, bgr=False):
    """What hv_rgbd_odometry_model returns for `level`: the target pyramid down to it, then target_model at its intrinsics."""
    z = tr.pyramid(target_depth, level + 1, depth_scale, depth_min, depth_max, trunc)[level]
    I = None if target_rgb is None else tc.intensity_pyramid(target_rgb, level + 1, bgr)[level]
    return target_model(z, I, tr.level_intrinsics(K, level), trunc)


class _Levels:
    """The per-level operands of one call, made on first use: source depth (and intensity), the target model, the photometric term."""

    def __init__(self, source_depth, target_depth, K, n_levels, source_rgb, target_rgb, depth_scale, depth_min, depth_max, trunc, lam,
                 idelta, bgr):
        self.K, self.trunc, self.lam, self.idelta = K, trunc, lam, idelta
        self.src = tr.pyramid(source_depth, n_levels, depth_scale, depth_min, depth_max, trunc)
        self.tgt = tr.pyramid(target_depth, n_levels, depth_scale, depth_min, depth_max, trunc)
        self.hybrid = source_rgb is not None
        if self.hybrid:
            self.isrc = tc.intensity_pyramid(source_rgb, n_levels, bgr)
            self.itgt = tc.intensity_pyramid(target_rgb, n_levels, bgr)
        self.made = {}

    def __call__(self, level):
        """-> (source depth, model (depth, normal, mask), K_level, photometric term or None)"""
        if level not in self.made:
            Kl = tr.level_intrinsics(self.K, level)
            m = target_model(self.tgt[level], self.itgt[level] if self.hybrid else None, Kl, self.trunc)
            term = None
            if self.hybrid:
                r = m["record"]
                term = tc.term(self.isrc[level], Kl, (r[..., 0], r[..., 1], r[..., 2], r[..., 3] != 0), self.lam, self.idelta)
            self.made[level] = (self.src[level], (m["depth"], m["normal"], m["mask"]), Kl, term)
        return self.made[level]


R0 = np.eye(3)  # the model's normals are already in the anchor (target camera) frame


def odometry(source_depth, target_depth, K, T_init=None, source_rgb=None, target_rgb=None, iterations=(10, 5, 4), depth_scale=1.0,
             depth_min=0.1, depth_max=3.0, trunc=0.07, delta=0.05, lam=0.01, idelta=0.1, bgr=False):
    """The whole call.  -> dict(transformation = T_target_source, fitness, inlier_rmse, information, success, iterations, degenerate,
    inliers, valid, trace) and, with colours, photometric_inliers and intensity_rmse."""
    assert (source_rgb is None) == (target_rgb is None)
    nl = len(iterations)
    T_init = np.eye(4) if T_init is None else np.asarray(T_init, np.float64)
    levels = _Levels(source_depth, target_depth, K, nl, source_rgb, target_rgb, depth_scale, depth_min, depth_max, trunc, lam, idelta, bgr)
    A = T_init.copy()
    trace, iters, degenerate, last = [], [0] * nl, 0, None
    for level in range(nl - 1, -1, -1):
        if iterations[level] == 0:
            continue
        src, model, Kl, term = levels(level)
        for it in range(iterations[level]):
            lin = tr.linearise(src, model, Kl, A, R0, trunc, delta, term)
            xi, deg = tr.solve(lin["H"], lin["g"], lin["inliers"])
            row = dict(lin, level=level, iteration=it, A=A.copy(), xi=xi)
            iters[level] += 1
            if level == 0:
                last = lin
            if deg:
                row["status"] = 2
                trace.append(row)
                degenerate |= 1 << level
                break
            A = tr.exp_twist(xi) @ A
            row["status"] = 1 if tr.converged(xi) else 0
            trace.append(row)
            if row["status"] == 1:
                break
    inl, val = last["inliers"], last["valid"]
    started = not (degenerate & 1 and iters[0] == 1)  # a level-0 linearisation left the level running
    out = {"transformation": A if started else T_init.copy(), "fitness": inl / val if val else 0.0,
           "inlier_rmse": float(np.sqrt(last["sq_error"] / inl)) if inl else 0.0, "information": last["H"],
           "success": not (degenerate & 1) and inl >= tr.MIN_INLIERS, "iterations": tuple(iters), "degenerate": degenerate,
           "inliers": inl, "valid": val, "trace": trace}
    if levels.hybrid:
        pin = last["photometric_inliers"]
        out.update(photometric_inliers=pin, intensity_rmse=float(np.sqrt(last["sq_intensity_error"] / pin)) if pin else 0.0)
    return out


class Result:
    """odometry()'s dict in the shape of an OdometryResult, so that check_call can be held against the restatement's own call."""

    def __init__(self, out):
        self.transformation, self.information = out["transformation"], out["information"]
        self.fitness, self.inlier_rmse, self.success = out["fitness"], out["inlier_rmse"], out["success"]
        self.iterations, self.degenerate, self.inliers, self.valid = out["iterations"], out["degenerate"], out["inliers"], out["valid"]
        self.photometric_inliers, self.intensity_rmse = out.get("photometric_inliers"), out.get("intensity_rmse")
        self.trace = [dict(r) for r in out["trace"]]


def check_call(out, source_depth, target_depth, K, T_init=None, source_rgb=None, target_rgb=None, iterations=(10, 5, 4), depth_scale=1.0,
               depth_min=0.1, depth_max=3.0, trunc=0.07, delta=0.05, lam=0.01, idelta=0.1, bgr=False):
    """Hold one traced hv_rgbd_odometry result (an OdometryResult with trace) to this restatement, step by step, as tr.check_call
    holds a tracking result: every traced row is linearised here at the row's own state A against target_model of the level, so
      - valid, inliers and (hybrid) photometric_inliers are equal;
      - H, g and the squared errors are within the float64 summation bound 2 (n + 2) 2^-53 S of tr.check_call;
      - the row's H, g solved here give its xi and its degenerate decision (a pivot within rounding of the threshold is reported
        instead), status 1 iff converged(xi); the first row's A is T_init exactly, the next row's A is exp(xi) A, or A after status 2.
    Then the schedule and the outputs; transformation is the last A itself, or T_init when level 0's first linearisation was
    degenerate.  -> dict(rows, near_pivot [(row, level, iteration)], xi_rel)."""
    nl = len(iterations)
    T_init = np.eye(4) if T_init is None else np.asarray(T_init, np.float64)
    hybrid = source_rgb is not None
    levels = _Levels(source_depth, target_depth, K, nl, source_rgb, target_rgb, depth_scale, depth_min, depth_max, trunc, lam, idelta, bgr)
    rows = out.trace
    assert rows is not None and len(rows) == sum(out.iterations), (len(rows), out.iterations)
    assert len(out.iterations) == nl and out.degenerate >> nl == 0, (out.iterations, out.degenerate)

    # schedule
    k = 0
    for level in range(nl - 1, -1, -1):
        if iterations[level] == 0:
            assert out.iterations[level] == 0 and not out.degenerate >> level & 1, level
            continue
        start = k
        while k < len(rows) and rows[k]["level"] == level:
            k += 1
        grp = rows[start:k]
        assert 1 <= len(grp) <= iterations[level], (level, len(grp), iterations)
        assert [r["iteration"] for r in grp] == list(range(len(grp))), level
        assert all(r["status"] == 0 for r in grp[:-1]), (level, [r["status"] for r in grp])
        assert grp[-1]["status"] in (1, 2) or len(grp) == iterations[level], (level, grp[-1]["status"], len(grp))
        assert out.iterations[level] == len(grp), (level, out.iterations)
        assert bool(out.degenerate >> level & 1) == (grp[-1]["status"] == 2), (level, out.degenerate)
    assert k == len(rows), "rows out of the coarse-to-fine order"

    # every step
    near, xi_rel = [], 0.0
    A_next = T_init
    for k, row in enumerate(rows):
        level = row["level"]
        what = (k, level, row["iteration"])
        if k == 0:
            assert np.array_equal(row["A"], T_init), what
        else:
            assert np.abs(row["A"] - A_next).max() <= tr.A_REL * max(1.0, np.abs(A_next).max()), (what, row["A"], A_next)
        src, model, Kl, term = levels(level)
        ref = tr.linearise(src, model, Kl, row["A"], R0, trunc, delta, term)
        assert row["valid"] == ref["valid"], (what, "valid", row["valid"], ref["valid"])
        assert row["inliers"] == ref["inliers"], (what, "inliers", row["inliers"], ref["inliers"])
        pin = 0
        if hybrid:
            pin = ref["photometric_inliers"]
            assert row["photometric_inliers"] == pin, (what, "photometric inliers", row["photometric_inliers"], pin)
            bar_i = 2.0 * (pin + 2) * tr.EPS
            assert abs(row["sq_intensity_error"] - ref["sq_intensity_error"]) <= bar_i * ref["sq_intensity_error"], (
                what, "e_I", row["sq_intensity_error"], ref["sq_intensity_error"])
        bar = 2.0 * (ref["inliers"] + pin + 2) * tr.EPS
        dH = np.abs(row["H"] - ref["H"])
        assert (dH <= bar * ref["H_abs"]).all(), (what, "H", float((dH / np.maximum(ref["H_abs"], 1e-300)).max()), bar)
        dg = np.abs(row["g"] - ref["g"])
        assert (dg <= bar * ref["g_abs"]).all(), (what, "g", float((dg / np.maximum(ref["g_abs"], 1e-300)).max()), bar)
        bar_e = 2.0 * (ref["inliers"] + 2) * tr.EPS
        assert abs(row["sq_error"] - ref["sq_error"]) <= bar_e * ref["sq_error"], (what, "e", row["sq_error"], ref["sq_error"])

        xi_ref, deg_ref = tr.solve(row["H"], row["g"], row["inliers"])
        if row["inliers"] >= tr.MIN_INLIERS and tr.pivot_near_threshold(row["H"]):
            near.append(what)
        else:
            assert (row["status"] == 2) == deg_ref, (what, "degenerate decision", row["status"], tr.pivots(row["H"]))
        if row["status"] == 2:
            assert not row["xi"].any(), what
            A_next = row["A"]
        else:
            if not deg_ref:
                scale = np.abs(xi_ref).max()
                rel = float(np.abs(row["xi"] - xi_ref).max() / scale) if scale > 0 else float(np.abs(row["xi"]).max())
                xi_rel = max(xi_rel, rel)
                assert rel <= tr.XI_REL, (what, "xi", row["xi"], xi_ref)
            assert (row["status"] == 1) == tr.converged(row["xi"]), (what, row["status"], row["xi"])
            A_next = tr.exp_twist(row["xi"]) @ row["A"]

    # outputs
    last = rows[-1]
    assert last["level"] == 0
    inl, val = last["inliers"], last["valid"]
    assert out.success == (last["status"] != 2 and inl >= tr.MIN_INLIERS), (out.success, last["status"], inl)
    assert np.array_equal(out.information, last["H"])
    assert out.inliers == inl and out.valid == val
    assert out.fitness == (inl / val if val else 0.0), (out.fitness, inl, val)
    assert out.inlier_rmse == (float(np.sqrt(last["sq_error"] / inl)) if inl else 0.0), (out.inlier_rmse, last["sq_error"], inl)
    if hybrid:
        pin = last["photometric_inliers"]
        assert out.photometric_inliers == pin, (out.photometric_inliers, pin)
        assert out.intensity_rmse == (float(np.sqrt(last["sq_intensity_error"] / pin)) if pin else 0.0), (
            out.intensity_rmse, last["sq_intensity_error"], pin)
    if last["status"] == 2 and out.iterations[0] == 1:
        assert np.array_equal(out.transformation, T_init), (out.transformation, T_init)
    else:
        assert np.abs(out.transformation - A_next).max() <= tr.A_REL * max(1.0, np.abs(A_next).max()), (out.transformation, A_next)
    return {"rows": len(rows), "near_pivot": near, "xi_rel": xi_rel}


def relative_pose(T_cw_target, T_cw_source):
    """The ground truth of a pair with world poses: T_target_source = T_cw(target) inverse(T_cw(source))."""
    return np.asarray(T_cw_target, np.float64) @ np.linalg.inv(np.asarray(T_cw_source, np.float64))


def motion(T):
    """-> (translation length in m, rotation angle in deg) of a rigid transform."""
    T = np.asarray(T, np.float64)
    c = np.clip((np.trace(T[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(T[:3, 3])), float(np.degrees(np.arccos(c)))


def pose_error(T_a, T_b):
    """-> (m, deg) of T_a inverse(T_b): how far two T_target_source are apart (tr.pose_error's measure)."""
    return tr.pose_error(T_a, T_b)
