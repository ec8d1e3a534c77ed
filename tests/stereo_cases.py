"""Inputs shared by the CPU and GPU tests of the stereo matcher (tests/stereo_reference.py is the restatement they are held to)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_sgm_tiny.npz")
GOLDEN_PARAMS = dict(num_disparities=32)  # every other parameter at its default
BASELINE = 0.11                            # metres, the synthetic pair's
TRUTH_POSES = (0, 150, 300)

# (H, W, D): the shapes at which the kernels change form
SHAPES = (
    (37, 83, 16), (37, 83, 48), (37, 83, 64),  # part of a wave; not a power of two; exactly one wave
    (19, 70, 128), (19, 70, 256),              # several values per lane
    (24, 40, 64),                              # W < D: most of the cost volume is the constant 64
    (1, 50, 16), (50, 1, 16),                  # one row, one column
    (7, 9, 16),                                # the image equals the census window
)


def planted_shift(H=24, W=96, k=11, seed=0):
    """right[:, x] = left[:, x + k], both cut from one random uint8 image.  -> (left, right) [H,W]"""
    base = np.random.default_rng(seed).integers(0, 256, (H, W + k), dtype=np.uint8)
    return np.ascontiguousarray(base[:, :W]), np.ascontiguousarray(base[:, k:])


def textured_pair(H, W, channels, seed):
    """A pair with structure at every scale the matcher looks at: smooth random texture, the right image the left one moved by a
    disparity that grows along x (2 .. about W / 5 px), plus a little noise of its own.  uint8 [H,W] or [H,W,3]."""
    rng = np.random.default_rng(seed)
    c = 1 if channels == 1 else 3
    wide = W + W // 4 + 8
    tex = rng.integers(0, 256, (H, wide, c)).astype(np.float64)
    for axis in (0, 1):  # a 3-tap blur: neighbouring pixels correlate, the census bits are not pure noise
        tex = (np.roll(tex, 1, axis) + 2 * tex + np.roll(tex, -1, axis)) / 4
    x = np.arange(W)
    shift = 2 + (x * (W // 5)) // max(W - 1, 1)
    left = tex[:, :W]
    right = np.zeros_like(left)
    for xr in range(W):  # right pixel xr shows what the left image shows at xr + shift
        right[:, xr] = tex[:, min(xr + int(shift[xr]), wide - 1)]
    right = right + rng.normal(0, 2.0, right.shape)
    to_u8 = lambda a: np.ascontiguousarray(np.clip(np.rint(a), 0, 255).astype(np.uint8))
    left, right = to_u8(left), to_u8(right)
    return (left[..., 0], right[..., 0]) if channels == 1 else (left, right)


def smooth_texture(rng, H, W, channels=1):
    """Random uint8 [H,W,channels] after a 3-tap blur along both axes: the texture of textured_pair."""
    tex = rng.integers(0, 256, (H, W, channels)).astype(np.float64)
    for axis in (0, 1):
        tex = (np.roll(tex, 1, axis) + 2 * tex + np.roll(tex, -1, axis)) / 4
    return np.clip(np.rint(tex), 0, 255).astype(np.uint8)


def staircase(W, shifts, rows=4, channels=1, seed=1):
    """Smooth texture, the right image cut in bands of `rows` rows, band b moved by shifts[b]: right[band, x] = left[band, x + k],
    so that a left pixel of band b has the disparity shifts[b].  -> (left, right) uint8 [rows len(shifts), W] or [.., W, 3]"""
    tex = smooth_texture(np.random.default_rng(seed), rows * len(shifts), W + max(shifts), channels)
    left = tex[:, :W]
    right = np.empty_like(left)
    for b, k in enumerate(shifts):
        right[b * rows:(b + 1) * rows] = tex[b * rows:(b + 1) * rows, k:k + W]
    if channels == 1:
        left, right = left[..., 0], right[..., 0]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def shifted_noise(H, W, k, seed):
    """planted_shift with a little noise of its own in the right image, so that costs tie and nearly tie.  -> (left, right) [H,W]"""
    rng = np.random.default_rng(seed)
    left, right = planted_shift(H, W, k, seed)
    noisy = right.astype(np.int32) + rng.integers(-6, 7, right.shape)
    return left, np.clip(noisy, 0, 255).astype(np.uint8)


def left_of_image_pair(H=8, W=28, k=3, columns=3, seed=0):
    """right = left moved by k, then the first columns of left replaced by 255 - right: the census of a left pixel at x < k looks
    least unlike a right pixel that lies outside the image's left edge.  -> (left, right) [H,W]"""
    left, right = planted_shift(H, W, k, seed)
    left = left.copy()
    left[:, :columns] = 255 - right[:, :columns]
    return left, right


# the shifts of the staircases: on both sides of every border between two rows of 16 lanes of the path kernel's wave (16, 32, 48
# for D = 64; twice and four times that for D = 128 and 256, where a lane holds 2 and 4 disparities), and the ends of the range
_STAIR_64 = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)
_STAIR_128 = (2, 30, 32, 34, 62, 64, 66, 94, 96, 98, 124, 127)
_STAIR_256 = (3, 60, 64, 68, 124, 128, 132, 188, 192, 196, 252, 255)
BF_24 = float(np.array([0x4166B3A7], np.uint32).view(np.float32)[0])  # 14.41886...: a float32 whose mantissa uses all 24 bits
_SGM = dict(p1=10, p2=120, uniqueness_ratio=15, max_diff=1, paths=8, bf=BF_24, min_depth=0.0, max_depth=np.inf)
# cases whose events need their own number of paths; every other case is also run with the other one on the GPU
OWN_PATHS = ("wide_2x257_D256_p1023", "equality_u0", "equality_u20", "equality_u50", "left_of_image_maxdiff1", "left_of_image_maxdiff-1",
             "maxdiff3_9x40", "depth_cuts_9x40")


def _planted():
    cases = []

    def add(name, pair, **params):
        cases.append((name, pair[0], pair[1], {**_SGM, **params}))

    add("stair_D64", staircase(140, _STAIR_64), num_disparities=64)
    add("stair_D128", staircase(220, _STAIR_128), num_disparities=128)
    add("stair_D256", staircase(330, _STAIR_256), num_disparities=256)
    add("stair_D64_rgb", staircase(140, _STAIR_64, channels=3), num_disparities=64)
    # wide rows: one, two (the second of one pixel) and three tiles of 256 of the winner kernel; a band of one row per shift
    for W in (256, 257, 513):
        add(f"wide_3x{W}_D16", staircase(W, (3, 9, 15), rows=1, seed=W), num_disparities=16)
        add(f"wide_3x{W}_D256", staircase(W, (40, 130, 250), rows=1, seed=W), num_disparities=256)
    add("wide_2x257_D256_p1023", staircase(257, (70, 200), rows=1, seed=2), num_disparities=256, p1=1023, p2=1023)  # the largest keys
    # path starts: n = H, W and H + W - 1 starts per direction, four to a workgroup; W = 6, 41, 43, 40 and H + W - 1 = 46, 46, 47,
    # 48, 49 take every residue mod 4
    for H, W in ((41, 6), (6, 41), (5, 43), (9, 40), (7, 43)):
        add(f"starts_{H}x{W}", textured_pair(H, W, 1, seed=H * 100 + W), num_disparities=16)
    # rule 6 at equality: the seeds that tools/search_stereo_cases.py settled on
    for u, seed in ((0, 995), (20, 166), (50, 55)):
        add(f"equality_u{u}", shifted_noise(6, 24, 5, seed), num_disparities=16, uniqueness_ratio=u)
    # a unique winner that points left of the image, with the left-right check and without it
    for max_diff in (1, -1):
        add(f"left_of_image_maxdiff{max_diff}", left_of_image_pair(), num_disparities=16, paths=4, p1=100, p2=1023, uniqueness_ratio=0,
            max_diff=max_diff)
    add("maxdiff3_9x40", textured_pair(9, 40, 1, seed=24), num_disparities=16, max_diff=3)
    # depth cuts that some pixel's depth equals: the pair has pixels with d16 = 115 (the near cut) and d16 = 33 (the far cut), and
    # rule 10 is one float32 multiplication and one division
    near, far = (float(np.float32(BF_24) * np.float32(16.0) / np.float32(d16)) for d16 in (115, 33))
    add("depth_cuts_9x40", textured_pair(9, 40, 1, seed=940), num_disparities=16, min_depth=near, max_depth=far)
    return cases


PLANTED = _planted()  # [(name, left, right, params)]


def planted(name):
    """-> (left, right, params) of the named case"""
    return next(c[1:] for c in PLANTED if c[0] == name)


def synthetic_pair(i, config="tiny_160x120_2cm", baseline=BASELINE):
    """-> (rgb_left, rgb_right, depth_left, T_cw, stream) of pose i"""
    from pyslam_amd.synthetic import SyntheticRGBD

    s = SyntheticRGBD(config, noise=False, invalid_frac=0.0)
    return s.stereo(i, baseline) + (s,)


def truth_figures(disparity16, depth_left, fx, baseline):
    """The three figures of the ground-truth check: the share of valid pixels; among valid pixels that the right view also sees
    (x - true disparity >= 0), the share off by more than 1 px, and the median absolute error in px."""
    d = np.asarray(disparity16).astype(np.float64) / 16.0
    valid = np.asarray(disparity16) >= 0
    true = fx * baseline / np.asarray(depth_left, np.float64)
    x = np.arange(d.shape[1])[None, :]
    seen = valid & (x - true >= 0)
    err = np.abs(d - true)[seen]
    return float(valid.mean()), float((err > 1.0).mean()), float(np.median(err))


def load_golden():
    z = np.load(GOLDEN)
    return z["left"], z["right"], z["disparity"]
