"""CPU: the numpy restatement of the VOXEL_GRID queries, carving and removal (tests/grid_query_reference.py) against the oracles on
every case of tests/grid_query_cases.py; every decision class occurs in some case; every wrong reading of a rule (VARIANTS) is told
from the right one by some case.  Bit for bit, no tolerance."""
import functools

import numpy as np
import pytest

import oracle
from tests import grid_query_cases as qc
from tests import grid_query_reference as qr


def fronts(c):
    port = qc.OracleFront(oracle.PortGrid(c["voxel"], c["bs"]))
    ref = [qc.OracleFront(oracle.RefGrid(c["voxel"], c["bs"]))] if oracle.ref_available() else []
    return port, ref


@pytest.mark.parametrize("name", qc.CASE_NAMES)
def test_restatement_equals_the_oracles(name):
    c = qc.case(name)
    port, ref = fronts(c)
    assert qc.run_case(c, port, ref) == len(c["steps"])
    assert port.grid.num_blocks() <= 400 and port.grid.num_blocks() * c["bs"] ** 3 <= 200_000  # grids stay small


@functools.lru_cache(maxsize=None)
def survey():
    """Every case once on the port oracle -> (classes seen: {class: [case names]}, variants told apart: {variant: [case names]})."""
    classes = {k: [] for k in qr.CLASSES}
    told = {v: [] for v in qr.VARIANTS}
    for c in qc.all_cases():
        voxel, bs = c["voxel"], c["bs"]

        def on_step(i, step, before, want):
            for k, m in qr.classify(before, step, voxel, bs).items():
                if m.any() and c["name"] not in classes[k]:
                    classes[k].append(c["name"])
            if want is None:
                return
            for v in qr.VARIANTS:
                if c["name"] in told[v]:
                    continue
                wrong = qr.apply_step(before, step, voxel, bs, variant=v)
                if want[0] == "rows":
                    a, b = qc.sorted_rows(want[2], want[3]), qc.sorted_rows(wrong[2], wrong[3])
                    same = a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
                        np.array_equal(qc.bits(a)[~np.isnan(a)], qc.bits(b)[~np.isnan(b)])
                else:
                    same = np.array_equal(want[1][2], wrong[1][2])
                if not same:
                    told[v].append(c["name"])

        qc.run_case(c, qc.OracleFront(oracle.PortGrid(voxel, bs)), on_step=on_step)
    return classes, told


@pytest.mark.parametrize("cls", qr.CLASSES)
def test_every_class_occurs(cls):
    assert survey()[0][cls], f"no case puts a voxel on '{cls}'"


@pytest.mark.parametrize("variant", qr.VARIANTS)
def test_cases_tell_the_variant_from_the_rule(variant):
    assert survey()[1][variant], f"no case tells '{variant}' from the reference's rule"


def test_hair_boxes_exist_at_every_voxel_size():
    """The CPU search of box_hair_case finds coordinates whose float32 key is above their float64 key, below and above 0, at every size."""
    for voxel, _ in qc.SIZES:
        found = qc.key_disagreements(voxel)
        assert any(x < 0 for x, _, _ in found) and any(x > 0 for x, _, _ in found), voxel
        assert all(k32 == k64 + 1 for _, k32, k64 in found)


def test_face_points_split_as_float64_predicts():
    """Of the 18 prev / at / next points of BOX_A's faces, the oracle returns exactly those with lo <= float64(p) <= hi: 9."""
    for voxel, bs in ((0.05, 5), (0.015, 8), (0.005, 16)):
        pts = qc.face_points(qc.BOX_A, voxel)
        g = oracle.PortGrid(voxel, bs)
        g.integrate(pts)
        got = qc.sort_rows(g.get_voxels_in_bb(qc.BOX_A, 1)[0])[0]
        p = pts.astype(np.float64)
        want = pts[((p >= qc.BOX_A[:3]) & (p <= qc.BOX_A[3:])).all(axis=1)]
        assert len(want) == 9
        assert np.array_equal(got, qc.sort_rows(want)[0])
        assert len(g.get_voxels(0)[0]) == g.num_blocks() * bs ** 3


@pytest.mark.parametrize("name", [n for n in qc.CASE_NAMES if n.startswith("carve_identity") and "1000000000" not in n])
def test_sheet_two_tells_a_rounded_pixel_from_a_truncated_one(name):
    """The voxels at u = prev32(k + 1), v = prev32(r + 1), last column and row included: the rule reads pixel (r, k) and keeps every one;
    rounding reads (r + 1, k + 1) and carves every one but the corner voxel, whose rounded pixel is clamped back onto (H - 1, W - 1)."""
    c = qc.case(name)
    g = oracle.PortGrid(c["voxel"], c["bs"])
    for pts, cols in c["batches"]:
        g.integrate(pts, cols)
    before = g.dump()
    sheet2 = qc.voxels_holding(before, c["sheet2"])
    n = len(np.unique(c["sheet2"], axis=0))
    assert sheet2.sum() == n == 88
    step = c["steps"][1]
    kept = qr.apply_step(before, step, c["voxel"], c["bs"])[1][2] > 0
    rounded = qr.apply_step(before, step, c["voxel"], c["bs"], variant="round_pixel")[1][2] > 0
    assert kept[sheet2].all()
    assert (~rounded[sheet2]).sum() == n - 1
    g.carve(*[step[1][k] for k in ("intr", "W", "H", "T_cw", "dmax", "dmin")], step[2], np.float32(step[3]))
    assert (g.dump()[2][sheet2] == 1).all()
