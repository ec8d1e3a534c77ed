"""CPU: the register budget of the production sweep, read from the compiler's kernel metadata.

k_tsdf_sweep_column runs four waves per SIMD, i.e. at most 128 vector registers, and its frame loop only pays at that budget when
nothing of it is spilled.  hv_tsdf.hip is compiled to assembly with the build's own flags (device side only, no GPU needed) and the
metadata of both instantiations is held against the figures profiles/sweep_epilogue/README.md records for this source state.
"""
import os
import re
import subprocess

import pytest

from pyslam_amd import build
from tests.conftest import ROOT

RECORD = os.path.join(ROOT, "profiles", "sweep_epilogue", "README.md")
KERNELS = {1: "_Z19k_tsdf_sweep_columnILi1EEv", 2: "_Z19k_tsdf_sweep_columnILi2EEv"}


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{ZS: {field: value}} of the .amdhsa.kernels entries of k_tsdf_sweep_column<ZS>."""
    out = str(tmp_path_factory.mktemp("sweep_asm") / "hv_tsdf.s")
    cmd = [build._hipcc()] + build._flags() + ["--cuda-device-only", "-S", os.path.join(build.CSRC, "hv_tsdf.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    text = open(out).read()
    entries = text[text.index("amdhsa.kernels:"):].split("  - .")
    found = {}
    for zs, prefix in KERNELS.items():
        (entry,) = [e for e in entries if re.search(r"\.name:\s+" + re.escape(prefix), e)]
        found[zs] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", entry)}
        assert len(found[zs]) == 3
    return found


def recorded():
    """{ZS: (vgprs, spilled, scratch bytes)} from the record's table rows `| k_tsdf_sweep_column<ZS>, head | v | s | b |`."""
    rows = re.findall(r"^\|\s*`k_tsdf_sweep_column<(\d)>`, head\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", open(RECORD).read(), re.M)
    return {int(zs): (int(v), int(s), int(b)) for zs, v, s, b in rows}


@pytest.mark.parametrize("zs", [1, 2])
def test_column_sweep_stays_inside_four_waves_per_simd(metadata, zs):
    assert metadata[zs]["vgpr_count"] <= 128


@pytest.mark.parametrize("zs", [1, 2])
def test_column_sweep_spills_no_more_than_recorded(metadata, zs):
    rec = recorded()
    assert set(rec) == {1, 2}
    _, spilled, scratch = rec[zs]
    assert metadata[zs]["vgpr_spill_count"] <= spilled
    assert metadata[zs]["private_segment_fixed_size"] <= scratch
