"""CPU: the register budget of the batch path's touch + pack launch, read from the compiler's kernel metadata.

k_tsdf_prep_touch_batch runs beside the 128-register column sweep: two of its waves must fit where one sweep wave retired, i.e. at
most 64 vector registers, and the frame-grouped pack role (hv_pack_px4_frames: every load of a group in flight before the first
wait) only pays when nothing of it is spilled.  hv_tsdf.hip is compiled to assembly with the build's own flags (device side only,
no GPU needed), as tests/test_sweep_registers_cpu.py does for the sweep.
"""
import os
import re
import subprocess

import pytest

from pyslam_amd import build

KERNEL = "_Z23k_tsdf_prep_touch_batch"


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{field: value} of the .amdhsa.kernels entry of k_tsdf_prep_touch_batch."""
    out = str(tmp_path_factory.mktemp("pack_asm") / "hv_tsdf.s")
    cmd = [build._hipcc()] + build._flags() + ["--cuda-device-only", "-S", os.path.join(build.CSRC, "hv_tsdf.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    text = open(out).read()
    entries = text[text.index("amdhsa.kernels:"):].split("  - .")
    (entry,) = [e for e in entries if re.search(r"\.name:\s+" + re.escape(KERNEL), e)]
    found = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", entry)}
    assert len(found) == 3
    return found


def test_two_touch_pack_waves_fit_one_sweep_slot(metadata):
    assert metadata["vgpr_count"] <= 64


def test_touch_pack_launch_spills_nothing(metadata):
    assert metadata["vgpr_spill_count"] == 0
    assert metadata["private_segment_fixed_size"] == 0
