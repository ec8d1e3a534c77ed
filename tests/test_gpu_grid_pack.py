"""GPU: pack / unpack / save / load of VoxelBlockGrid and the four semantic block grids (include/hipvol.h "Packed grids").

Every comparison is an equality of bits: dumps, label lists, log-probabilities, confidences and confidence counters (recomputed by
tests/grid_pack_reference.py in float32 with the formulas of hv_semantic.h: exp / log in double, rounded once), packed bytes.
States are planted through integrate with the exact arithmetic of tests/semantic_planted.py: voxel 1/16, dyadic positions."""
import numpy as np
import pytest

import oracle
from oracle.semantic import PortSemGrid2, RefSemGrid2
from pyslam_amd._lib import HipVolError
from tests import bin_cases as bc
from tests import grid_pack_reference as R
from tests import semantic_planted as sp
from tests.test_gpu_semantic_ops import assert_state_equal
from tests.test_gpu_semantic_planted import GpuGrid
from tests.test_gpu_voxel_grid import assert_same_grid, make_oracle

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2, 11, 12)
KIND_OF_MODE = {1: 0, 2: 1, 11: 2, 12: 3}


def grid_class(mode):
    from pyslam_amd import volumetric as v
    from pyslam_amd import volumetric_semantic as vs

    return {0: v.VoxelBlockGrid, 1: vs.VoxelBlockSemanticGrid, 2: vs.VoxelBlockSemanticProbabilisticGrid, 11: vs.VoxelBlockSemanticGrid2,
            12: vs.VoxelBlockSemanticProbabilisticGrid2}[mode]


def make(mode, bs, max_blocks=64, max_points=1 << 12, voxel=sp.VOXEL):
    return grid_class(mode)(voxel, bs, max_blocks=max_blocks, max_points=max_points)


def centre(key, k, bs):
    """The centre of local voxel k of block `key` (voxel 1/16: exact)."""
    l = np.array([k % bs, (k // bs) % bs, k // (bs * bs)])
    return (np.asarray(key) * bs + l + 0.5) / 16.0


def feed(g, mode, pts, cls=3, obj=2):
    pts = np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 3))
    n = len(pts)
    col = np.stack([np.full(n, 0.25), np.full(n, 0.5), (np.arange(n) % 4) * 0.25], 1).astype(np.float32)
    if mode == 0:
        g.integrate(pts.astype(np.float32), col)
    else:
        g.integrate(pts, col, np.broadcast_to(np.asarray(cls, np.int32), (n,)).copy(), np.broadcast_to(np.asarray(obj, np.int32), (n,)).copy(), None)


def sorted_voxels(g, mode):
    v = g.get_voxels(1) if mode == 0 else g.get_voxels(1, -1.0)
    order = np.lexsort(tuple(np.asarray(v.points, np.float64).T[::-1]))
    rows = [np.asarray(v.points)[order], np.asarray(v.colors)[order]]
    if mode != 0:
        rows += [np.asarray(v.class_ids)[order], np.asarray(v.object_ids)[order], np.asarray(v.confidences)[order]]
    return rows


def state(g, mode):
    """Everything the round trip has to keep, as a list of arrays."""
    out = list(g.dump()) + [np.array([g.size(), g.num_blocks()])] + sorted_voxels(g, mode)
    if mode != 0:
        out += list(g.dump2(max_labels=254)) + list(g.dump_marginals())
    return out


def assert_same_state(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), i


def assert_reference_decodes(buf, g, mode):
    """unpack_reference(buf) against the grid's own dumps."""
    ref = R.unpack_reference(bytes(buf))
    if mode == 0:
        keys, _, counts, sums = g.dump()
        assert np.array_equal(ref["keys"], keys) and np.array_equal(ref["counts"], counts)
        assert ref["sums"].tobytes() == np.ascontiguousarray(sums).tobytes()
        return ref
    keys, ints, pos, col, conf, nlab, labels, logp = g.dump2(max_labels=254)
    oc, cc = g.dump_marginals()
    assert np.array_equal(ref["keys"], keys)
    assert ref["pos"].tobytes() == pos.tobytes() and ref["col"].tobytes() == col.tobytes()
    if mode in (2, 12):
        assert np.array_equal(ref["nlab"], nlab) and np.array_equal(ref["labels"], labels) and ref["logp"].tobytes() == logp.tobytes()
    assert np.array_equal(ref["ints"], ints), np.argwhere(ref["ints"] != ints)[:4]
    for name, a, b in (("conf", ref["conf"], conf), ("obj_conf", ref["obj_conf"], oc), ("cls_conf", ref["cls_conf"], cc)):
        assert a.dtype == b.dtype == np.float32
        assert a.tobytes() == b.tobytes(), (name, np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:4])
    return ref


# ---- 1. round trip ------------------------------------------------------------------------------------------------------------------
def plant_round_trip(mode, bs):
    """Voxels at local indices 0, 63, 64, 65 and nvox - 1 (where they exist) of blocks (-2, 0, 1) and (1, 2, 0), two points each with
    a label change on the odd ones; block (3, -1, -2) takes one point and is emptied again (kept, mask 0)."""
    nvox = bs ** 3
    g = make(mode, bs)
    ks = sorted({k for k in (0, 63, 64, 65, nvox - 1) if k < nvox})
    pts = np.array([centre(key, k, bs) for key in ((-2, 0, 1), (1, 2, 0)) for k in ks])
    odd = np.arange(len(pts)) % 2
    feed(g, mode, pts, cls=3 + odd, obj=2 + np.arange(len(pts)) % 3)
    feed(g, mode, pts, cls=3 + odd, obj=2 + np.arange(len(pts)) % 3 + odd)
    feed(g, mode, [centre((3, -1, -2), nvox // 2, bs)])
    g.remove_low_count_voxels(2)
    return g, 2 * len(ks)


@pytest.mark.parametrize("bs", [1, 3, 4, 5, 8, 16])
@pytest.mark.parametrize("mode", MODES)
def test_round_trip(mode, bs):
    src, planted = plant_round_trip(mode, bs)
    assert src.num_blocks() == 3
    want = state(src, mode)
    counts = want[2] if mode == 0 else want[1][..., 0]  # dump(): per block and voxel, keys ascending
    per_block = (counts > 0).sum(axis=1).tolist()
    stored = sum(per_block)
    assert stored == src.size() and 0 in per_block  # (one block is allocated and empty)
    assert per_block == [planted // 2, planted // 2, 0]  # (-2, 0, 1), (1, 2, 0), the emptied (3, -1, -2)
    buf = src.pack()
    info = src.packed_info(buf)
    assert (info["mode"], info["block_size"], info["blocks"], info["voxels"], info["bytes"]) == (mode, bs, 3, stored, buf.size)
    ref = assert_reference_decodes(buf, src, mode)
    assert ref["stored"].sum(axis=1).tolist() == per_block
    dst = make(mode, bs)
    st = dst.unpack(buf)
    assert (st.blocks, st.voxels, st.extra_pairs, st.bytes) == (3, stored, 0, buf.size)
    assert_same_state(state(dst, mode), want)
    assert dst.pack().tobytes() == buf.tobytes()
    src.reserve_blocks(512)  # (another pool, the same map)
    assert src.pack().tobytes() == buf.tobytes()
    assert_same_state(state(src, mode), want)


def test_an_empty_grid_packs_to_a_valid_buffer_and_unpacks():
    for mode in MODES:
        g = make(mode, 8)
        buf = g.pack()
        info = g.packed_info(buf)
        assert (info["blocks"], info["voxels"], info["extra_pairs"]) == (0, 0, 0) and R.check_reference(bytes(buf))["blocks"] == 0
        st = make(mode, 8).unpack(buf)
        assert st.blocks == 0 and st.bytes == buf.size


# ---- 2. label maps at the boundaries ------------------------------------------------------------------------------------------------
MAP_SIZES = (1, 6, 7, 16, 17, 26, 63)


def grow_maps(g, mode, sizes, sites, first=0):
    """Single-point integrates with distinct labels until site i holds sizes[i] pairs.  Mode 2 adds one (object, class) pair per distinct
    label; mode 12 holds one object and one class entry after the first observation and adds one object entry per further object (the
    class stays 5), so an n-entry list takes n - 1 observations - and its smallest list has 2 entries, which stands in for 1 there."""
    need = [s if mode == 2 else max(s - 1, 1) for s in sizes]
    for step in range(max(need)):
        on = [i for i, n in enumerate(need) if n > step]
        feed(g, mode, [sites[i] for i in on], cls=(step % 7 if mode == 2 else 5), obj=100 + first + step)


@pytest.mark.parametrize("mode", [2, 12])
def test_label_maps_at_the_boundaries(mode):
    bs = 8
    src = make(mode, bs)
    victim = centre((0, 0, 0), 77, bs)
    grow_maps(src, mode, [17], [victim], first=500)
    assert src.prob_nodes_used() == 2
    src.remove_low_confidence_voxels(0.5)  # the only voxel so far (confidence 1 / 17 or less): reset, keeps its two nodes
    assert src.size() == 0 and src.prob_nodes_used() == 2
    sites = [centre((-1, 0, 0) if i % 2 else (0, 0, 0), 9 * i + 1, bs) for i in range(len(MAP_SIZES))]
    grow_maps(src, mode, MAP_SIZES, sites)
    sizes = sorted(max(s, 2) if mode == 12 else s for s in MAP_SIZES)
    nlab = src.dump2(max_labels=254)[5]
    assert sorted(nlab[nlab > 0].tolist()) == sizes and src.label_overflows() == 0
    nodes = sum(-(-max(s - 6, 0) // 10) for s in sizes)
    assert src.prob_nodes_used() == nodes + 2
    buf = src.pack()
    info = src.packed_info(buf)
    assert info["voxels"] == len(sizes) and info["extra_pairs"] == sum(max(s - 6, 0) for s in sizes) and info["chain_nodes"] == nodes
    assert_reference_decodes(buf, src, mode)
    dst = make(mode, bs)
    assert dst.unpack(buf).extra_pairs == info["extra_pairs"]
    assert dst.prob_nodes_used() == nodes  # the reset voxel's chain was capacity, not content
    assert_same_state(state(dst, mode), state(src, mode))
    assert dst.pack().tobytes() == buf.tobytes()
    for g in (src, dst):  # one more observation of an existing pair, one of a new pair
        feed(g, mode, sites, cls=(0 if mode == 2 else 5), obj=100)
        feed(g, mode, sites, cls=(1 if mode == 2 else 5), obj=900)
    assert_same_state(state(dst, mode), state(src, mode))
    assert dst.label_overflows() == 0


# ---- 3. continuation against the oracles -------------------------------------------------------------------------------------------
ORACLES = [PortSemGrid2] + ([RefSemGrid2] if oracle.ref_available() else [])
CONTINUATIONS = {
    "label-half": (lambda: sp.label_case(8), "half"),
    "label-between-calls": (lambda: sp.label_case(8), "assoc"),
    "depth-filter-carve": (lambda: sp.depth_filter_case(4, "carve"), "assoc"),
    "carve": (lambda: sp.carve_case(5, "depth"), "half"),
    "overflow-labels": (sp.overflow_label_case, "assoc"),
}


def cut_of(case, where):
    if where == "half":
        return len(case.steps) // 2
    return next(i for i, s in enumerate(case.steps) if s[0] == "assoc") + 1


def part_of(case, steps, next_id):
    part = sp.Case(case.name, case.bs, case.T, case.depth_max, case.depth_min, next_id)
    part.steps = steps
    return part


@pytest.mark.parametrize("name", sorted(CONTINUATIONS))
@pytest.mark.parametrize("kind", sp.KINDS)
def test_continuation_equals_the_uninterrupted_oracles(kind, name, tmp_path):
    build, where = CONTINUATIONS[name]
    case = build()
    cut = cut_of(case, where)
    assert 0 < cut < len(case.steps)
    first = GpuGrid(kind, case.bs)
    records, canon = sp.drive(first, part_of(case, case.steps[:cut], case.next_id), raw_depth=True)
    second = GpuGrid(kind, case.bs)
    if kind % 2:  # through a file
        first.g.save(tmp_path / "map.hvg")
        second.g = type(first.g).load(tmp_path / "map.hvg", max_blocks=256, max_points=1 << 13)
    else:
        second.g.unpack(first.g.pack(device=True))
    more, canon = sp.drive(second, part_of(case, case.steps[cut:], first.peek_next_object_id()), raw_depth=True, to_canon=canon)
    records += more
    assert not canon and second.g.dropped_points() == 0 and second.g.label_overflows() == 0
    for mk in ORACLES:
        ref = mk(kind, sp.VOXEL, case.bs)
        ref_records, ref_canon = sp.drive(ref, build())
        assert [(r["map"], r["next_id"]) for r in records] == [(r["map"], r["next_id"]) for r in ref_records]
        assert_state_equal(second, ref, kind, ref_canon)


def test_voxel_grid_continuation_equals_the_oracle():
    calls = bc.vg_two_small()
    first, cpu = make(0, 8, max_blocks=256, max_points=1 << 14, voxel=bc.VOXEL), make_oracle(bc.VOXEL)
    first.integrate(*calls[0].grid_args())
    second = make(0, 8, max_blocks=256, max_points=1 << 14, voxel=bc.VOXEL)
    second.unpack(first.pack())
    second.integrate(*calls[1].grid_args())
    for c in calls:
        cpu.integrate(*c.grid_args())
    assert_same_grid(second, cpu)
    assert second.size() == cpu.size()


# ---- 4. many blocks and capacity ---------------------------------------------------------------------------------------------------
def many_blocks(mode, n=2500):
    g = make(mode, 8, max_blocks=8192, max_points=1 << 12)
    i = np.arange(n)
    keys = np.stack([i % 50 - 25, i // 50 - 25, (i % 7) - 3], 1)
    feed(g, mode, (keys * 8 + 0.5) / 16.0, cls=1 + i % 4, obj=1 + i % 9)
    assert g.num_blocks() == n
    return g


@pytest.mark.parametrize("mode", [0, 2])
def test_many_blocks_grow_the_target_or_are_refused_whole(mode, monkeypatch):
    src = many_blocks(mode)
    buf, want = src.pack(), state(src, mode)
    assert src.packed_info(buf)["blocks"] == 2500
    dst = make(mode, 8)
    dst.unpack(buf)
    assert dst.max_blocks() >= 2500
    assert_same_state(state(dst, mode), want)
    monkeypatch.setenv("HV_AUTO_GROW", "0")
    small = make(mode, 8)
    with pytest.raises(HipVolError, match="block pool exhausted"):
        small.unpack(buf)
    assert small.num_blocks() == 0 and small.size() == 0
    small.reserve_blocks(4096)
    small.unpack(buf)
    monkeypatch.delenv("HV_AUTO_GROW")
    assert_same_state(state(small, mode), want)


@pytest.mark.parametrize("mode", [2, 12])
def test_chains_beyond_the_node_pool_are_refused_whole(mode, monkeypatch):
    src = make(mode, 8)
    sites = [centre((0, 0, 0), 3, 8), centre((1, 0, 0), 5, 8)]
    grow_maps(src, mode, [17, 7], sites)
    buf = src.pack()
    assert src.packed_info(buf)["chain_nodes"] == 3
    monkeypatch.setenv("HV_PROB_NODE_CAP", "2")
    small = make(mode, 8)
    monkeypatch.delenv("HV_PROB_NODE_CAP")
    with pytest.raises(HipVolError, match="need 3 overflow nodes"):
        small.unpack(buf)
    assert small.num_blocks() == 0 and small.prob_nodes_used() == 0
    big = make(mode, 8)
    big.unpack(buf)
    assert_same_state(state(big, mode), state(src, mode))


# ---- 5. pack only reads ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_pack_only_reads(kind):
    import torch

    case = sp.label_case(8).upto(1)
    gpu = GpuGrid(kind, 8)
    mode = {0: 1, 1: 2}[kind]
    for step in case.steps[:-1]:
        gpu.integrate(step[1], step[2], step[3], step[4], None)
    feed(gpu.g, mode, [[2.0 ** 30, 0.0, 0.0]])  # a point without a voxel
    a = case.steps[-1][1]
    gpu.set_next_object_id(case.next_id)
    frustum = gpu.frustum(np.array(sp.INTR, np.float32), sp.W, sp.H, case.T, case.depth_max, case.depth_min)
    lazy = gpu.g.assign_object_ids_to_instance_ids(frustum, a["cls_img"], a["inst_img"], None, a["depth_threshold"], False, a["min_vote_ratio"],
                                                   a["min_votes"])
    assert lazy._d is None
    probes = np.concatenate([case.steps[0][1][:40], [[9.0, 9.0, 9.0]]])

    def observed():
        look = gpu.g.lookup_points(probes, stats=True)
        return state(gpu.g, mode) + [np.asarray(x) for x in (look.status, look.count, look.position, look.class_id, look.object_id, look.confidence)] + [
            np.array(look.stats.as_tuple()), np.array([gpu.g.dropped_points(), gpu.g.label_overflows()])]

    before = observed()
    host = gpu.g.pack()
    dev = gpu.g.pack(device=True)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.uint8
    assert dev.cpu().numpy().tobytes() == host.tobytes()
    assert_same_state(observed(), before)
    assert lazy._d is None and lazy.on_device_of(gpu.g)
    twin = GpuGrid(kind, 8)
    for step in case.steps[:-1]:
        twin.integrate(step[1], step[2], step[3], step[4], None)
    twin.set_next_object_id(case.next_id)
    want = dict(twin.g.assign_object_ids_to_instance_ids(frustum, a["cls_img"], a["inst_img"], None, a["depth_threshold"], False, a["min_vote_ratio"],
                                                         a["min_votes"]))
    assert dict(lazy) == want and want


# ---- 6. refusals leave the volume as it was ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 12])
def test_refusals_leave_the_target_empty_and_usable(mode):
    import torch

    bs = 3 if mode == 1 else 8
    src = make(mode, bs)
    sites = [centre(key, k, bs) for key, k in (((-2, 0, 1), bs ** 3 - 1), ((-2, 0, 1), 0), ((1, 2, 0), 1), ((3, -1, -2), 2))]
    if mode in (2, 12):
        grow_maps(src, mode, [7, 17, 2, 2], sites)
    else:
        feed(src, mode, sites)
    good = src.pack()
    want = state(src, mode)
    dst = make(mode, bs)

    def refused(buf, words, target=None, blocks=0):
        target = dst if target is None else target
        with pytest.raises(HipVolError) as e:
            target.unpack(buf)
        assert words in str(e.value), str(e.value)
        assert target.num_blocks() == blocks and target.size() == blocks

    for name, (bad, rule) in R.corrupt_buffers(good.tobytes()).items():
        refused(bad, R.RULE_WORDS[rule])
        refused(torch.frombuffer(bytearray(bad), dtype=torch.uint8).cuda(), R.RULE_WORDS[rule])
    other = {0: 1, 1: 11, 2: 12, 12: 2}[mode]
    refused(good, "the packed grid has mode", make(other, bs))
    refused(good, "the packed grid has mode", make(mode, bs + 1))
    refused(good, "bitwise equal", make(mode, bs, voxel=float(np.nextafter(np.float32(sp.VOXEL), np.float32(1)))))
    # ... and a voxel_size that differs in the LAST bit of the float64 the header holds (the constructors narrow a grid's own voxel
    # size to float32, so the bit is flipped in the header, at byte 16): only a comparison of all 64 bits can tell
    last_bit = bytearray(good.tobytes())
    last_bit[16:24] = np.float64(np.nextafter(sp.VOXEL, 1.0)).tobytes()
    assert np.float32(np.frombuffer(bytes(last_bit[16:24]), np.float64)[0]) == np.float32(sp.VOXEL)
    R.check_reference(bytes(last_bit))
    refused(bytes(last_bit), "bitwise equal")
    sharded = make(mode, bs)
    sharded.set_owner(0, 2)
    refused(good, "owner-sharded", sharded)
    full = make(mode, bs)
    feed(full, mode, sites[:1])
    held = state(full, mode)
    refused(good, "EMPTY grid", full, blocks=1)
    assert_same_state(state(full, mode), held)
    if mode in (2, 12):
        h = R.header_reference(good.tobytes())
        rec = h["offsets"][3]
        meta = int(np.frombuffer(good.tobytes(), "<u4", 1, rec + 4)[0])
        assert meta & 0xFF == 17  # record 0: block (-2, 0, 1), voxel 0
        for patched, words in ((meta - 1, "meta names 16 label pairs"), ((meta & 0xFF) | (18 << 8), "cached best index")):
            bad = bytearray(good.tobytes())
            bad[rec + 4:rec + 8] = np.uint32(patched).tobytes()
            R.check_reference(bytes(bad))  # (the metadata is consistent: only the record pass can tell)
            refused(bytes(bad), words)
    dst.unpack(good)
    assert_same_state(state(dst, mode), want)


# ---- 7. next object id ---------------------------------------------------------------------------------------------------------------
def test_next_object_id_is_raised_never_lowered_and_new_ids_lie_above_the_map(tmp_path):
    from pyslam_amd.volumetric_semantic import get_next_object_id_peek, set_next_object_id

    case = sp.label_case(8)
    first = GpuGrid(0, 8)
    cut = cut_of(case, "assoc")
    sp.run_case(first, part_of(case, case.steps[:cut], 40))
    at_pack = get_next_object_id_peek()
    assert at_pack >= 40
    first.g.save(tmp_path / "map.hvg")
    assert first.g.packed_info(tmp_path / "map.hvg")["next_object_id"] == at_pack
    buf = first.g.pack()
    set_next_object_id(at_pack + 100)
    GpuGrid(0, 8).g.unpack(buf)
    assert get_next_object_id_peek() == at_pack + 100
    set_next_object_id(3)
    second = GpuGrid(0, 8)
    second.g = type(first.g).load(tmp_path / "map.hvg")
    assert get_next_object_id_peek() == at_pack
    held = second.g.get_voxels(1, -1.0).object_ids
    cls_img, inst_img = sp.images(4, 77)  # only the class-4 voxels vote, and they carry no object id yet: instance 77 needs a new one
    m = second.assign_object_ids_to_instance_ids(np.array(sp.INTR, np.float32), sp.W, sp.H, case.T, case.depth_max, case.depth_min, cls_img, inst_img,
                                                 None, 0.25, False, 0.0, 1)
    assert m == {77: at_pack} and at_pack > held.max() and get_next_object_id_peek() == at_pack + 1


# ---- 8. operands and files ------------------------------------------------------------------------------------------------------------
def test_operands_files_and_load(tmp_path):
    import torch

    mode, bs = 2, 8
    src = make(mode, bs)
    src.set_depth_threshold(3.5)
    src.set_depth_decay_rate(0.125)
    sites = [centre((0, 0, 0), 3, bs), centre((-1, 2, 0), 5, bs)]
    grow_maps(src, mode, [17, 3], sites)
    buf, want = src.pack(), state(src, mode)
    for operand in (buf, buf.tobytes(), memoryview(buf.tobytes()), torch.from_numpy(buf.copy()), torch.from_numpy(buf.copy()).cuda(), src.pack(device=True)):
        dst = make(mode, bs)
        dst.unpack(operand)
        assert_same_state(state(dst, mode), want)
    path = tmp_path / "map.hvg"
    st = src.save(path)
    assert path.read_bytes() == buf.tobytes() and st.bytes == buf.size and [p.name for p in tmp_path.iterdir()] == ["map.hvg"]
    assert src.packed_info(path) == src.packed_info(buf) == src.packed_info(buf.tobytes())
    loaded = type(src).load(path)
    assert_same_state(state(loaded, mode), want)
    assert loaded.max_blocks() == 1024 and loaded.block_size == bs and loaded.voxel_size == src.voxel_size
    assert type(src).load(path, max_blocks=77).max_blocks() == 77
    # the header's depth settings were applied: the same deep observation folds to the same bits on both
    for g in (src, loaded):
        g.integrate(np.array([sites[0]]), np.array([[0.5, 0.5, 0.5]], np.float32), np.array([0], np.int32), np.array([100], np.int32),
                    np.array([6.0], np.float32))
    assert_same_state(state(loaded, mode), state(src, mode))
    plain = make(mode, bs)  # unpack leaves the target's own settings alone: the default threshold 5.0 and rate 0.07 fold differently
    plain.unpack(buf)
    plain.integrate(np.array([sites[0]]), np.array([[0.5, 0.5, 0.5]], np.float32), np.array([0], np.int32), np.array([100], np.int32),
                    np.array([6.0], np.float32))
    assert plain.dump2(max_labels=254)[7].tobytes() != src.dump2(max_labels=254)[7].tobytes()
    with pytest.raises(ValueError, match="cannot be loaded as"):
        grid_class(12).load(path)
