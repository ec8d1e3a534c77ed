"""Writes tests/golden/stereo_sgm_tiny.npz: the synthetic 160x120 stereo pair of pose 0 (baseline 0.11 m) as grey uint8 images
(rule 1 applied: a third of the bytes) and the int16 disparity the numpy restatement (tests/stereo_reference.py) gives for it at
D = 32, defaults otherwise.  The file pins the restatement: run this
again only when the rules themselves change.  Also prints the ground-truth figures of profiles/stereo_sgm/README.md."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import stereo_cases as sc  # noqa: E402
import stereo_reference as sr  # noqa: E402


def main():
    for i in sc.TRUTH_POSES:
        left, right, depth, _, s = sc.synthetic_pair(i)
        disp, _ = sr.stereo_sgm(left, right, **sc.GOLDEN_PARAMS)
        valid, off, med = sc.truth_figures(disp, depth, s.fx, sc.BASELINE)
        true = s.fx * sc.BASELINE / depth
        print(f"pose {i}: true disparity {true.min():.1f}-{true.max():.1f} px, valid {valid:.4f}, off by > 1 px {off:.4f}, "
              f"median error {med:.3f} px")
        if i == 0 and "--check" not in sys.argv:
            os.makedirs(os.path.dirname(sc.GOLDEN), exist_ok=True)
            grey = [sr.grey(a).astype(np.uint8) for a in (left, right)]
            assert np.array_equal(sr.stereo_sgm(*grey, **sc.GOLDEN_PARAMS)[0], disp)
            np.savez_compressed(sc.GOLDEN, left=grey[0], right=grey[1], disparity=disp)
            print("wrote", sc.GOLDEN, os.path.getsize(sc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
