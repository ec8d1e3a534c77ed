"""Planted images and descriptor sets for the tests of detect_features / match_features - test infrastructure, no GPU - and the
constants of the appearance loop test with where they come from."""
import numpy as np

# (H, W, channels): 33x33 has exactly one candidate pixel; 33x97 one candidate row; 64x64 four full cells; 65x66 has a level 1 of
# 32x33, which yields nothing; 66x66 a level 1 of 33x33 with exactly one candidate; 97x131x3 partial cells on both sides, colour
SHAPES = [(33, 33, 1), (33, 97, 1), (64, 64, 1), (65, 66, 1), (66, 66, 1), (97, 131, 3)]


def blocks(H, W, channels=1, seed=0):
    """Random rectangles of random grey with a little noise: corners at the junctions, ties among the scores."""
    rng = np.random.default_rng(seed)

    def plane():
        low = rng.integers(0, 256, (H // 5 + 1, W // 7 + 1))
        return (np.kron(low, np.ones((5, 7), np.int64))[:H, :W] // 4 * 4 + rng.integers(0, 4, (H, W))).clip(0, 255).astype(np.uint8)

    return plane() if channels == 1 else np.ascontiguousarray(np.stack([plane() for _ in range(channels)], axis=2))


def shaped(H, W, channels, seed=0):
    """blocks() with a bright 2x2 block at rows / columns 32, 33 where it fits: one bright pixel at (16,16) of level 1."""
    img = blocks(H, W, channels, seed)
    if H >= 66 and W >= 66:
        img[29:37, 29:37] = 40
        img[32:34, 32:34] = 250
    if H == 33:
        img[13:20, 13:20] = 40
        img[16, 16] = 250
    return img


def dot(H=40, W=48, y=17, x=20, background=100, value=200):
    img = np.full((H, W), background, np.uint8)
    img[y, x] = value
    return img


def periodic(H=96, W=96, period=8, phase=4):
    """Bright dots every `period` pixels: 16 lone-dot corners of one score in a 32x32 cell that lies inside the candidate region."""
    img = np.full((H, W), 60, np.uint8)
    img[phase::period, phase::period] = 220
    return img


def adjacent_pair(H=48, W=48, y=20, x=22):
    """Two horizontally adjacent bright pixels: two corners of one score, of which rule F5 keeps the first."""
    img = np.full((H, W), 80, np.uint8)
    img[y, x] = img[y, x + 1] = 230
    return img


TIE_CENTRE = (32, 32)  # (y, x)


def orientation_tie(H=64, W=64):
    """A lone bright pixel at TIE_CENTRE on a flat field with two more pixels in its disc, +200 at dx = 10 and +20 at dy = 10:
    m10 = 2000 = 10 m01, so bins 0 and 1 tie (1024 m10 = 1004 m10 + 200 m01) and rule F8 takes bin 0."""
    y, x = TIE_CENTRE
    img = np.full((H, W), 30, np.uint8)
    img[y, x] = 250
    img[y, x + 10] = 230
    img[y + 10, x] = 50
    return img


def descriptor_sets(nq, nt, seed=0):
    """Random train descriptors; each query a train descriptor with 0..47 bits flipped, every fifth one random."""
    rng = np.random.default_rng(seed)
    train = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    query = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    for i in range(nq):
        if i % 5 == 4:
            continue
        bits = np.unpackbits(train[rng.integers(0, nt)])
        bits[rng.choice(256, int(rng.integers(0, 48)), replace=False)] ^= 1
        query[i] = np.packbits(bits)
    return query, train


# ---- the appearance loop test (tests/test_gpu_appearance_loops.py) -------------------------------------------------------------
LOOP_FRAMES = (0, 6, 12, 18, 570, 580, 590)  # frames of SyntheticRGBD("tiny_160x120_2cm"), noisy depth, a 600-frame orbit
LOOP_FEATURES = dict(levels=3, threshold=20, per_cell=8)
LOOP_PARAMS = dict(min_gap=3, min_inliers=8, inlier_threshold=0.05, max_candidates=3)
LOOP_ODOMETRY = dict(depth_max=5.0)  # what the graph hands to rgbd_odometry (hybrid, everything else at its default)
# The tolerance of an added edge's transformation against the ground truth: MEASURED, not chosen.  The same chain run with the numpy
# restatements on the CPU - restated_loops(odometry=True) below: tests/orb_reference.py, pyslam_amd/features.py and
# tests/odometry_reference.py; `python -m tests.orb_cases` prints it, profiles/orb_features/README.md keeps the output - gave the
# errors per edge listed there.  The worst of them are the two constants; the test allows LOOP_TOLERANCE_FACTOR times that, and the
# factor covers nothing but a future change of the noise seed.
LOOP_WORST_TRANSLATION_M = 0.0023  # frames (570, 0)
LOOP_WORST_ROTATION_DEG = 0.045    # frames (570, 0)
LOOP_TOLERANCE_FACTOR = 2.0


def loop_frames():
    """-> (K (fx, fy, cx, cy), [(depth, rgb, T_cw)] of LOOP_FRAMES, the camera namespace KeyframeGraphRgbd takes)"""
    import types

    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD("tiny_160x120_2cm")
    cam = types.SimpleNamespace(fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, width=s.width, height=s.height)
    return s.intrinsics, [s[i] for i in LOOP_FRAMES], cam


def restated_loops(K, frames, odometry=False, **match_params):
    """KeyframeGraphRgbd.close_loops_by_appearance on the numpy restatements: -> [dict(j, i, matches, inliers, T_ransac, accepted, and
    with odometry: success, transformation, translation_error_m, rotation_error_deg against the ground truth)] for every verified
    pair, in the order the method verifies them."""
    from pyslam_amd import features as F
    from tests import odometry_reference as orf
    from tests import orb_reference as R

    feats = []
    for depth, rgb, _ in frames:
        kp, desc = R.detect(rgb, **LOOP_FEATURES)
        feats.append((R.level0_xy(kp), desc))
    sizes = [len(f[1]) for f in feats]
    out = []
    for j in range(len(frames)):
        last = j - LOOP_PARAMS["min_gap"]
        if last < 0 or sizes[j] == 0:
            continue
        offsets = np.concatenate([[0], np.cumsum(sizes[:last + 1])]).astype(np.int32)
        if offsets[-1] == 0:
            continue
        index, _, _, counts = R.match(feats[j][1], np.concatenate([f[1] for f in feats[:last + 1]]), offsets,
                                      match_params.get("max_distance", 64), match_params.get("ratio_percent", 80), match_params.get("cross_check", 1))
        for i in [int(i) for i in np.argsort(-counts, kind="stable")[:LOOP_PARAMS["max_candidates"]] if counts[i] >= 3]:
            hit = index[i] >= 0
            P, okp = F.backproject(feats[j][0][hit], frames[j][0], K)
            Q, okq = F.backproject(feats[i][0][index[i][hit] - offsets[i]], frames[i][0], K)
            T, inliers = F.rigid_from_matches(P[okp & okq], Q[okp & okq], LOOP_PARAMS["inlier_threshold"])
            row = dict(j=j, i=i, matches=int(hit.sum()), inliers=int(inliers.sum()), T_ransac=T,
                       accepted=T is not None and int(inliers.sum()) >= LOOP_PARAMS["min_inliers"])
            if odometry and row["accepted"]:
                res = orf.odometry(frames[j][0], frames[i][0], np.asarray(K, np.float64), T_init=T, source_rgb=frames[j][1], target_rgb=frames[i][1],
                                   **LOOP_ODOMETRY)
                err = orf.pose_error(res["transformation"], orf.relative_pose(frames[i][2], frames[j][2]))
                row.update(success=bool(res["success"]), transformation=res["transformation"], translation_error_m=float(err[0]),
                           rotation_error_deg=float(err[1]))
            out.append(row)
    return out


if __name__ == "__main__":
    K, frames, _ = loop_frames()
    for row in restated_loops(K, frames, odometry=True):
        tail = "" if "success" not in row else "  odometry %s, off the truth by %.4f m, %.3f deg" % (
            "ok" if row["success"] else "FAILED", row["translation_error_m"], row["rotation_error_deg"])
        print("frames (%3d, %3d): %2d matches, %2d inliers, %s%s" % (LOOP_FRAMES[row["j"]], LOOP_FRAMES[row["i"]], row["matches"], row["inliers"],
                                                                     "accepted" if row["accepted"] else "rejected", tail))
