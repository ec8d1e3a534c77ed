"""Bundle adjustment over keyframes: tracks from pairwise matches, their first points, and the reference's two-phase schedule around
_Volume.bundle_adjust (hv_bundle_adjust, contract in include/hipvol.h).  Host bookkeeping only; the adjustment runs on the GPU."""
import numpy as np


def build_tracks(pair_matches, min_length=2):
    """Union-find over (keyframe, keypoint) joined by accepted matches: -> a list of tracks, each an int64 array [L,2] of (keyframe,
    keypoint) sorted by keyframe.  pair_matches: an iterable of (keyframe a, keyframe b, matches [K,2] of (keypoint in a, keypoint in
    b)).  A track that would hold two keypoints of one keyframe is dropped whole (the matches contradict each other); tracks shorter
    than min_length are dropped.  The order is fixed: by each track's smallest member."""
    if int(min_length) < 2:
        raise ValueError(f"build_tracks: min_length must be at least 2, got {min_length}")
    up = {}

    def root(a):
        up.setdefault(a, a)
        while up[a] != a:
            up[a] = up[up[a]]
            a = up[a]
        return a

    for a, b, matches in pair_matches:
        for i, j in np.asarray(matches, np.int64).reshape(-1, 2).tolist():
            ra, rb = root((int(a), i)), root((int(b), j))
            if ra != rb:
                up[max(ra, rb)] = min(ra, rb)
    groups = {}
    for member in sorted(up):
        groups.setdefault(root(member), []).append(member)
    tracks = []
    for members in sorted(groups.values()):
        frames = [m[0] for m in members]
        if len(members) >= int(min_length) and len(set(frames)) == len(frames):
            tracks.append(np.array(members, np.int64))
    return tracks


def observations_of(tracks):
    """-> (index [O,2] int32 of (keyframe, track), keypoint [O] int64): one observation per member of every track, track by track."""
    if not tracks:
        return np.zeros((0, 2), np.int32), np.zeros(0, np.int64)
    frame = np.concatenate([t[:, 0] for t in tracks])
    point = np.concatenate([np.full(len(t), j) for j, t in enumerate(tracks)])
    return np.stack([frame, point], -1).astype(np.int32), np.concatenate([t[:, 1] for t in tracks])


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def initial_points(tracks, features, depths, extrinsics, intrinsic, bf, depth_scale=1.0):
    """The start of an adjustment from tracks: -> (points [M,3], index [O,2] int32, measurements [O,3], inv_sigma2 [O], keep
    [len(tracks)] bool).  features[k]: keyframe k's Features (keypoints with the level in column 2, xy at level 0); depths[k]: its
    depth image; extrinsics [N,4,4] T_cw.  A track's point is its first member with a valid depth, back-projected with
    features.backproject and carried to the world through the keyframe's pose; tracks without one are dropped (keep = False) and the
    points are numbered in the order of the kept tracks.  Every member with a valid depth z is an RGB-D observation, u_r = u - bf / z as
    the reference forms it; the others are monocular (u_r = nan).  inv_sigma2 = 4^-level for the factor-2 pyramid."""
    from .features import backproject

    if not hasattr(intrinsic, "as_array") and hasattr(intrinsic, "fx"):
        intrinsic = (intrinsic.fx, intrinsic.fy, intrinsic.cx, intrinsic.cy)
    frames = sorted({int(k) for t in tracks for k in t[:, 0]})
    cam = {k: backproject(_host(features[k].xy), _host(depths[k]), intrinsic, depth_scale) for k in frames}
    xy = {k: _host(features[k].xy).astype(np.float64) for k in frames}
    level = {k: _host(features[k].keypoints)[:, 2].astype(np.float64) for k in frames}
    extrinsics = np.asarray(extrinsics, np.float64).reshape(-1, 4, 4)
    pts, idx, meas, s2, keep = [], [], [], [], np.zeros(len(tracks), bool)
    for n, t in enumerate(tracks):
        valid = [bool(cam[k][1][i]) for k, i in t.tolist()]
        if not any(valid):
            continue
        keep[n] = True
        k, i = t[valid.index(True)].tolist()
        T = extrinsics[k]
        pts.append(T[:3, :3].T @ (cam[k][0][i] - T[:3, 3]))
        for (k, i), ok in zip(t.tolist(), valid):
            u, v = xy[k][i]
            idx.append((k, len(pts) - 1)), meas.append((u, v, u - bf / cam[k][0][i, 2] if ok else np.nan)), s2.append(4.0 ** -level[k][i])
    return (np.array(pts, np.float64).reshape(-1, 3), np.array(idx, np.int32).reshape(-1, 2), np.array(meas, np.float64).reshape(-1, 3),
            np.array(s2, np.float64), keep)


def bundle_adjust_two_phase(volume, cameras, points, observations, measurements, intrinsic, bf, inv_sigma2=1.0, camera_fixed=None,
                            fixed_points=False, rounds=10, **params):
    """The reference's schedule (optimizer_g2o.bundle_adjustment): rounds // 2 outer iterations with the Huber kernel; the observations
    that end as outliers or behind their camera are switched off; the remaining iterations run without the kernel.  -> (the second
    BundleResult, active [O] bool as the second phase saw it, mean chi2 over those observations - what the reference returns).  With
    rounds < 2 there is one phase, with the kernel."""
    first = volume.bundle_adjust(cameras, points, observations, measurements, intrinsic, bf=bf, inv_sigma2=inv_sigma2, camera_fixed=camera_fixed,
                                 fixed_points=fixed_points, huber=True, max_iterations=max(1, int(rounds) // 2), **params)
    active = first.inlier
    result = first
    if int(rounds) - int(rounds) // 2 >= 1 and int(rounds) >= 2 and bool(active.any()):
        result = volume.bundle_adjust(first.cameras, first.points, observations, measurements, intrinsic, bf=bf, inv_sigma2=inv_sigma2, active=active,
                                      camera_fixed=camera_fixed, fixed_points=fixed_points, huber=False,
                                      max_iterations=int(rounds) - int(rounds) // 2, **params)
    n = int(active.sum())
    mean = float((result.chi2 * active).sum()) / n if n else 0.0
    return result, active, mean
