"""Host time per call of the Python binding alone: four methods of ScalableTSDFVolume against the recording stand-in for the library
(tests/recording_lib.py), so nothing but Python runs and no GPU is needed.  Five repeats of 2000 calls, the median call of each
repeat in microseconds, one JSON line.  --against DIR also loads the pyslam_amd of another checkout (as the package pyslam_other) and
runs the repeats of the two alternately in this one process: the way profiles/binding_refactor/README.md compares this commit with
its parent, because the speed of a shared CPU changes from one process to the next by more than the difference."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    trees = {"this": ROOT}
    if args.against:
        trees["other"] = os.path.abspath(args.against)
        spec = importlib.util.spec_from_file_location("pyslam_other", os.path.join(trees["other"], "pyslam_amd", "__init__.py"),
                                                      submodule_search_locations=[os.path.join(trees["other"], "pyslam_amd")])
        sys.modules["pyslam_other"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules["pyslam_other"])
    modules = {"this": importlib.import_module("pyslam_amd.volumetric")}
    if args.against:
        modules["other"] = importlib.import_module("pyslam_other.volumetric")
    out = {"trees": trees, "unit": "us per call (median of each repeat)", "calls": args.calls}
    cases = {side: make_cases(V) for side, V in modules.items()}
    for name in next(iter(cases.values())):
        out[name] = {side: [] for side in cases}
        for _ in range(args.repeats):
            for side in cases:
                out[name][side].append(median_call(cases[side][name], args.calls))
    print(json.dumps(out))


def median_call(call, calls):
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return round(statistics.median(times) * 1e6, 3)


def make_cases(V):
    from tests.recording_lib import RecordingLib, volume

    class Lib(RecordingLib):  # (nothing reads the record here: keep it from growing)
        calls = property(lambda self: [], lambda self, value: None)

    vol = volume(V.ScalableTSDFVolume, voxel_length=0.02, sdf_trunc=0.08, res=16)
    vol._lib = Lib()
    K = V.PinholeCameraIntrinsic(640, 480, 525.0, 525.0, 319.5, 239.5)
    image = V.RGBDImage(np.zeros((480, 640, 3), np.uint8), np.ones((480, 640), np.float32), 1.0, 4.0)
    points = np.zeros((1000, 3), np.float32)
    T = np.eye(4)
    return {"integrate_480x640": lambda: vol.integrate(image, K, T), "sample_points_1000": lambda: vol.sample_points(points),
            "dirty_keys": vol.dirty_keys, "surface_components_empty": vol.surface_components}


if __name__ == "__main__":
    main()
