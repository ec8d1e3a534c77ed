"""Geometric verification of feature matches for appearance loop closure: back-projection of keypoints through a depth image and
a three-point RANSAC for the rigid motion between two matched point sets.  Host code by decision: the inputs are tens of points
(the detection and the matching are the GPU calls, _Volume.detect_features / match_features)."""
import numpy as np


def _fxfycxcy(intrinsic):
    if hasattr(intrinsic, "as_array"):
        intrinsic = intrinsic.as_array()
    k = np.asarray(intrinsic, np.float64)
    if k.shape == (3, 3):
        return k[0, 0], k[1, 1], k[0, 2], k[1, 2]
    if k.shape == (4,):
        return tuple(k)
    raise ValueError(f"backproject: intrinsic must be a PinholeCameraIntrinsic, 3x3 or (fx, fy, cx, cy), got shape {k.shape}")


def backproject(xy, depth, intrinsic, depth_scale=1.0):
    """xy [N,2] pixel positions (level 0), depth [H,W] (metres times depth_scale) -> (points float64 [N,3] in the camera frame,
    valid bool [N]).  Each point takes the depth of the nearest pixel (round half up); valid where that pixel lies in the image and
    its depth is finite and positive.  Invalid points are zero."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    d = np.asarray(depth)
    if d.ndim != 2:
        raise ValueError(f"backproject: depth must be [H,W], got {d.shape}")
    fx, fy, cx, cy = _fxfycxcy(intrinsic)
    u, v = np.floor(xy[:, 0] + 0.5).astype(np.int64), np.floor(xy[:, 1] + 0.5).astype(np.int64)
    inside = (u >= 0) & (u < d.shape[1]) & (v >= 0) & (v < d.shape[0])
    z = np.zeros(len(xy), np.float64)
    z[inside] = d[v[inside], u[inside]].astype(np.float64) / float(depth_scale)
    valid = inside & np.isfinite(z) & (z > 0)
    z = np.where(valid, z, 0.0)
    pts = np.stack([(xy[:, 0] - cx) / fx * z, (xy[:, 1] - cy) / fy * z, z], axis=1)
    return pts, valid


def kabsch(P, Q):
    """The rigid T (4x4) minimising sum |T P_i - Q_i|^2."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    cp, cq = P.mean(axis=0), Q.mean(axis=0)
    U, _, Vt = np.linalg.svd((Q - cq).T @ (P - cp))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    T = np.eye(4)
    T[:3, :3] = U @ D @ Vt
    T[:3, 3] = cq - T[:3, :3] @ cp
    return T


def rigid_from_matches(P, Q, threshold, iterations=256, seed=0):
    """Three-point RANSAC for T with T P_i ~ Q_i (P, Q [N,3], metres): `iterations` samples of three distinct matches drawn with
    numpy's default_rng(seed), Kabsch on each, inliers |T P_i - Q_i| <= threshold; the sample with the most inliers (the first one of
    a tie) is refitted on its inliers, and the inliers of the refit are returned.  Deterministic.  -> (T 4x4 float64, inliers bool
    [N]); (None, all False) with fewer than three matches or when no sample has three inliers."""
    P, Q = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(Q, np.float64).reshape(-1, 3)
    n = len(P)
    if len(Q) != n:
        raise ValueError(f"rigid_from_matches: P and Q must have the same length, got {n} and {len(Q)}")
    none = np.zeros(n, bool)
    if n < 3:
        return None, none
    rng = np.random.default_rng(seed)
    best, best_count = None, 2
    for _ in range(int(iterations)):
        pick = rng.choice(n, 3, replace=False)
        T = kabsch(P[pick], Q[pick])
        inl = np.linalg.norm(P @ T[:3, :3].T + T[:3, 3] - Q, axis=1) <= threshold
        if inl.sum() > best_count:
            best, best_count = inl, int(inl.sum())
    if best is None:
        return None, none
    T = kabsch(P[best], Q[best])
    inl = np.linalg.norm(P @ T[:3, :3].T + T[:3, 3] - Q, axis=1) <= threshold
    if inl.sum() < 3:
        return None, none
    return T, inl
