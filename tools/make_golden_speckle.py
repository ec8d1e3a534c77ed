#!/usr/bin/env python3
"""PIN for the speckle filter (include/hipvol.h, rules S1 - S6): run wherever `import cv2` works and commit the output.

Writes tests/golden/speckle_opencv.npz: cv2.filterSpeckles(image, new_val, max_speckle_size, max_diff) on every planted int16 case
of tests/speckle_cases.py, one array per case name.  tests/test_speckle_reference_cpu.py consumes the file when it exists (the numpy
restatement against OpenCV; the GPU is held to the restatement).  OpenCV is not installed in this image: until this script has run
somewhere, parity with cv2.filterSpeckles is by rule."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    try:
        import cv2
    except ImportError:
        print("cv2 is not importable here: nothing written (the speckle filter stays unpinned)")
        return 1
    from tests import speckle_cases as pc

    out = {"cv2_version": cv2.__version__}
    for name, image, params in pc.PLANTED:
        if image.dtype != np.int16:
            continue  # (cv2.filterSpeckles takes 8-bit and 16-bit images only)
        work = image.copy()
        cv2.filterSpeckles(work, params["new_val"], params["max_speckle_size"], params["max_diff"])
        out[name] = work
    path = os.path.join(ROOT, "tests", "golden", "speckle_opencv.npz")
    np.savez_compressed(path, **out)
    print("wrote", path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
