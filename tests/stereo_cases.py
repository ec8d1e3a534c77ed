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
