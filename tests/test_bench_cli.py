"""bench.py's command line: a plain run prints the headline alone, everything else it measures sits behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config")
FULL_ONLY_KEYS = ("roofline", "cpu_baseline", "speedup_vs_cpu", "online_mode", "replay_mode", "batch32", "extraction", "host_mode", "host_fed",
                  "tum1_640x480_5mm", "configs", "voxel_grid", "semantic", "semantic_scannet_2mm")


def test_help_lists_full_and_the_driver_options():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, check=True).stdout
    for opt in ("--full", "--gpus", "--steps", "--warmup", "--dump-outputs"):
        assert opt in out, opt


def test_load_frames_returns_the_same_frames_rendered_and_cached():
    """A cache miss hands back the frames it has just rendered, a hit the cached copy: the same arrays either way."""
    import bench

    cache = bench.frame_cache_path("tiny_160x120_2cm_3_2")
    if os.path.exists(cache):
        os.remove(cache)
    try:
        _, d0, c0, T0 = bench.load_frames("tiny_160x120_2cm", 2, start=3)
        assert os.path.exists(cache)
        _, d1, c1, T1 = bench.load_frames("tiny_160x120_2cm", 2, start=3)
        for a, b in ((d0, d1), (c0, c1), (T0, T1)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    finally:
        if os.path.exists(cache):
            os.remove(cache)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(tmp_path):
    """Two steps of the driver's command: one JSON line with the headline keys and none of the legs --full adds; --dump-outputs writes
    its five arrays."""
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, check=True, timeout=300, cwd=str(tmp_path)).stdout
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    z = json.loads(lines[0])
    for k in HEADLINE_KEYS:
        assert k in z, k
    assert z["unit"] == "frames/s" and z["higher_is_better"] is True and z["dtype"] == "f32" and z["steps"] == 2 and z["warmup"] == 1
    assert z["value"] > 0 and z["ms_per_step"] > 0
    assert abs(z["value"] - 2 * 64 / (2 * z["ms_per_step"] * 1e-3)) <= 0.01 * z["value"]  # value = frames of the timed steps / their time
    assert z["config"]["full"] is False
    for k in FULL_ONLY_KEYS:
        assert z.get(k) is None, k
    assert sorted(os.listdir(tmp_path / "dump")) == ["sample_color_sum.npy", "sample_keys.npy", "sample_tsdf_x_weight.npy", "sample_weight.npy",
                                                     "unit_keys.npy"]
