"""GPU: the semantic association (vote scan, voting rules, deferred assignments), carving and the segment operations / queries on the
planted cases of tests/semantic_planted.py - cases tests/test_semantic_planted_cpu.py has proven on three restatements that share
no code.  Expectations: tests/assoc_rules_reference.py for the rules alone, oracle.semantic.PortSemGrid2 always and RefSemGrid2 (the
compiled reference) where it is built for everything that touches a grid.  Tolerances are assert_state_equal's: bit-exact for the
voting payloads, 2e-6 on confidences for the log-probability ones.  Nothing here drives a table, list or queue past its capacity
on the device; the one capacity condition is the host's refusal of 4097 pairs."""
import functools

import numpy as np
import pytest

import oracle
from oracle.semantic import PortSemGrid2, RefSemGrid2, ref_get_class_segments
from tests import semantic_planted as sp
from tests.assoc_rules_reference import SEEN, decide, pack_pairs, unpack_pairs
from tests.test_gpu_semantic_ops import EXACT, assert_state_equal

pytestmark = pytest.mark.gpu

ORACLES = [PortSemGrid2] + ([RefSemGrid2] if oracle.ref_available() else [])


class GpuGrid:
    """A pyslam_amd semantic grid behind the oracles' interface (oracle.semantic._Sem2Base)."""

    def __init__(self, kind, bs, max_blocks=256, max_points=1 << 13):
        from pyslam_amd import volumetric_semantic as vs

        cls = (vs.VoxelBlockSemanticGrid, vs.VoxelBlockSemanticProbabilisticGrid, vs.VoxelBlockSemanticGrid2, vs.VoxelBlockSemanticProbabilisticGrid2)[kind]
        self.g = cls(sp.VOXEL, bs, max_blocks=max_blocks, max_points=max_points)
        self.kind, self.block_size = kind, bs

    def frustum(self, intr, width, height, T, dmax, dmin):
        from pyslam_amd.volumetric import CameraFrustrum

        return CameraFrustrum(*(float(x) for x in intr), width, height, T, depth_max=dmax, depth_min=dmin)

    def integrate(self, *a):
        self.g.integrate(*a)

    def set_next_object_id(self, v):
        from pyslam_amd.volumetric_semantic import set_next_object_id

        set_next_object_id(v)

    def peek_next_object_id(self):
        from pyslam_amd.volumetric_semantic import get_next_object_id_peek

        return get_next_object_id_peek()

    def assign_object_ids_to_instance_ids(self, intr, width, height, T, dmax, dmin, cls_img, inst_img, depth, thr, carve, ratio, votes):
        return dict(self.g.assign_object_ids_to_instance_ids(self.frustum(intr, width, height, T, dmax, dmin), cls_img, inst_img, depth, thr, carve,
                                                             ratio, votes))

    def carve(self, intr, width, height, T, dmax, dmin, depth, thr):
        self.g.carve(self.frustum(intr, width, height, T, dmax, dmin), depth, thr)

    def dump(self):
        return self.g.dump2()[:5]

    def dump2(self, *a, **kw):
        return self.g.dump2(*a, **kw)

    def num_blocks(self):
        return self.g.num_blocks()


def check_case_on_gpu(make, kind):
    """The case on the GPU grid and on every oracle, cut after each of its association calls in turn: maps, next ids, the first
    call's votes and the whole voxel state (carving and deferred assignments included) after every call."""
    n = make().n_assoc()
    for upto in range(1, n + 1) if n else [0]:
        case = make().upto(upto)
        gpu = GpuGrid(kind, case.bs)
        records, to_canon = sp.drive(gpu, case, raw_depth=True)
        assert not to_canon  # new ids in ascending instance order: the rules reference's, nothing to permute
        assert gpu.g.dropped_points() == 0 and gpu.g.label_overflows() == 0
        for mk in ORACLES:
            ref = mk(kind, sp.VOXEL, case.bs)
            ref_records, ref_canon = sp.drive(ref, make().upto(upto))
            assert [(r["map"], r["next_id"]) for r in records] == [(r["map"], r["next_id"]) for r in ref_records]
            assert [r["votes"]["pairs"] for r in records[:1]] == [r["votes"]["pairs"] for r in ref_records[:1]]
            assert_state_equal(gpu, ref, kind, ref_canon)
    return gpu, records


# ---- a. the rules alone -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def staged():
    """One vote of blank images on an empty grid opens the staged interface; every test then sets its own pairs."""
    gpu = GpuGrid(0, 8, max_blocks=64, max_points=1 << 12)
    cls_img, inst_img = sp.images(-1, -1)
    assert gpu.g.assoc_vote(gpu.frustum(sp.INTR, sp.W, sp.H, sp.IDENTITY, 4.0, 0.25), cls_img, inst_img)
    keys, counts = gpu.g.assoc_pairs()
    assert len(keys) == 0 and len(counts) == 0
    return gpu


def decide_on_gpu(gpu, pairs, ratio, min_votes, next_id):
    from pyslam_amd.volumetric_semantic import get_next_object_id_peek, set_next_object_id

    set_next_object_id(next_id)
    gpu.g.assoc_set_pairs(*pack_pairs(pairs))
    m = dict(gpu.g.assoc_decide(ratio, min_votes))
    return m, get_next_object_id_peek()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 63, 64, 65, 1000, 4095, 4096])
def test_rules_on_seeded_pair_lists(staged, n):
    """Pair counts around the powers of two of the padded sort and at its capacity; duplicates, ties, instance 0, markers; next id 6
    inside the object ids (a new id before, equal to and after existing ones)."""
    for seed, ratio, min_votes in ((n, 0.5, 3), (n + 7, sp.THIRD, 1), (n + 13, 2.0 / 3.0, 2)):
        pairs = sp.random_pairs(n, seed)
        assert decide_on_gpu(staged, pairs, ratio, min_votes, 6) == decide(pairs, ratio, min_votes, 6), (n, seed)


SCENES = sp.rule_scenes()


@pytest.mark.parametrize("name,pairs,ratio,min_votes,next_id", SCENES, ids=[s[0] for s in SCENES])
def test_rules_on_the_exact_ratio_min_votes_and_next_id_cases(staged, name, pairs, ratio, min_votes, next_id):
    """The rule scenes of the CPU test as pair lists: as given, reversed, with the image's markers (what the vote stage hands out
    for the scene), and with every pair a second time (two GPUs' lists: the votes double, the ratios stay)."""
    with_markers = pairs + [(i, SEEN, 1) for i, _, _ in pairs]
    for lst in (pairs, pairs[::-1], with_markers, with_markers + pairs):
        assert decide_on_gpu(staged, lst, ratio, min_votes, next_id) == decide(lst, ratio, min_votes, next_id), (name, lst)


def test_more_pairs_than_the_rules_kernel_sorts_are_refused_by_the_host(staged):
    from pyslam_amd._lib import HipVolError
    from pyslam_amd.volumetric_semantic import get_next_object_id_peek, set_next_object_id

    set_next_object_id(50)
    with pytest.raises(HipVolError, match="more than 4096 pairs"):
        staged.g.assoc_set_pairs(*pack_pairs(sp.random_pairs(4097, 1)))
    assert get_next_object_id_peek() == 50
    assert decide_on_gpu(staged, [(4, 2, 1)], 0.5, 1, 50) == ({4: 2}, 50)  # the stage is still usable


# ---- b. the full association on every builder ---------------------------------------------------------------------------------------
KINDS = list(sp.KINDS)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bs", [4, 5, 8, 16])
def test_frustum_edge_case(kind, bs):
    gpu, records = check_case_on_gpu(functools.partial(sp.frustum_edge_case, bs), kind)
    assert records[0]["votes"]["visited"] == 6


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bs", [4, 5, 8, 16])
def test_label_case(kind, bs):
    gpu, records = check_case_on_gpu(functools.partial(sp.label_case, bs), kind)
    assert records[0]["map"] == {0: 0, 6: 5, 8: -1}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant", sp.DEPTH_VARIANTS)
@pytest.mark.parametrize("bs", [5, 8])
def test_depth_filter_case(kind, bs, variant):
    gpu, records = check_case_on_gpu(functools.partial(sp.depth_filter_case, bs, variant), kind)
    assert records[0]["votes"]["carved"] == (2 if variant == "carve" else 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bs", [5, 8])
def test_dense_pending_case(kind, bs):
    gpu, records = check_case_on_gpu(functools.partial(sp.dense_pending_case, bs), kind)
    assert records[1]["votes"]["pending"] >= 600 and sorted(records[1]["map"].values()) == [4, 5, 6, 7]


@pytest.mark.parametrize("kind", KINDS)
def test_many_pairs_case(kind):
    gpu, records = check_case_on_gpu(sp.many_pairs_case, kind)
    assert len(records[0]["map"]) == 100


@pytest.mark.parametrize("kind", [1, 3])
def test_overflow_label_case(kind):
    gpu, records = check_case_on_gpu(sp.overflow_label_case, kind)
    if kind == 1:
        assert sorted(gpu.dump2(max_labels=16)[5].ravel())[-3:] == [7, 13, 13]
    assert [r["map"] for r in records] == [{5: 2}, {5: 2}]


# ---- c. carve ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bs", [5, 8])
@pytest.mark.parametrize("which", ["depth", "edge"])
def test_carve_on_the_planted_edges(kind, bs, which):
    make = functools.partial(sp.carve_case, bs, which)
    gpu, _ = check_case_on_gpu(make, kind)
    n_before = sum(len(np.unique(np.floor(s[1] * 16.0), axis=0)) for s in make().steps[:1])
    assert gpu.g.size() == n_before - (2 if which == "depth" else 6)  # depth > 1.25 + 0.25 twice; the six voxels in view


# ---- d. segment operations and queries -----------------------------------------------------------------------------------------------
RESET = np.array([0, -1, -1, 0], np.int32)


def after_python_reset(dump, which):
    """A dump after v.reset() of the voxels `which` (VoxelSemanticData::reset: zero sums and counts, ids -1)."""
    keys, ints, pos, col, conf = (a.copy() for a in dump)
    ints[which], pos[which], col[which], conf[which] = RESET, 0.0, 0.0, 0.0
    return keys, ints, pos, col, conf


def assert_dump_equal(gpu, exp, kind):
    class Fixed:
        def dump(self):
            return exp

    assert_state_equal(gpu, Fixed(), kind)


def ids_multiset(cls, obj):
    return sorted(zip(np.asarray(cls).tolist(), np.asarray(obj).tolist()))


@pytest.mark.parametrize("kind", KINDS)
def test_segment_operations_and_queries_on_planted_counts_and_confidences(kind):
    case = sp.segment_ops_case()
    gpu = GpuGrid(kind, case.bs)
    refs = [mk(kind, sp.VOXEL, case.bs) for mk in ORACLES]
    sp.drive(gpu, case)
    for r in refs:
        sp.drive(r, case)
    tol = 0.0 if kind in EXACT else 2e-6

    def same():
        for r in refs:
            assert_state_equal(gpu, r, kind)
            cg, og = gpu.g.get_ids()
            assert ids_multiset(cg, og) == ids_multiset(*r.get_ids())
            assert gpu.g.size() == len(cg)

    def both(op, *a):
        getattr(gpu.g, op)(*a)
        for r in refs:
            getattr(r, op)(*a)
        same()

    def away_from(threshold):
        """A confidence threshold compares exactly only where confidences are exact: for the log-probability payloads every planted
        confidence must be further than 1e-4 from it (the kernels' 2e-6 could otherwise flip a voxel), or the threshold moves."""
        conf = refs[0].dump()[4]
        t = threshold
        while kind not in EXACT and np.abs(conf - np.float32(t)).min() < 1e-4:
            t += 0.003
        return t

    same()
    # queries first: strict '>' on the count, '>=' on the confidence
    for min_count, min_conf in ((1, 0.0), (2, away_from(0.5)), (3, away_from(1.0)), (0, away_from(0.5))):
        segs = gpu.g.get_object_segments(min_count, min_conf)
        for r in refs:
            exp = r.get_object_segments(min_count, min_conf)
            assert [(int(o.object_id), len(o.points)) for o in segs.object_vector] == [(o["object_id"], len(o["points"])) for o in exp]
            # (the voxels without an object id are of several classes: which one their segment reports is the container's order)
            assert [int(o.class_id) for o in segs.object_vector if o.object_id >= 0] == [o["class_id"] for o in exp if o["object_id"] >= 0]
            for a, b in zip(segs.object_vector, exp):
                np.testing.assert_array_equal(a.points[np.lexsort(a.points.T[::-1])], b["points"][np.lexsort(b["points"].T[::-1])])
                assert abs(a.confidence_min - b["conf_min"]) <= tol and abs(a.confidence_max - b["conf_max"]) <= tol
        if kind in EXACT and min_count == 2 and min_conf == 0.5:
            by_id = {int(o.object_id): len(o.points) for o in segs.object_vector}
            # object 11: the rows of 3 and 4 points at confidence 1 and the row of 4 points of which one said 12 - confidence exactly
            # 2 / 4 - but not the rows of 1 and 2 points (count > 2 is strict); object 12 has 2 points per voxel; object 14: one row
            assert by_id[11] == 9 and by_id.get(12, 0) == 0 and by_id[14] == 3
        got = gpu.g.get_class_segments(min_count, min_conf)
        if RefSemGrid2 in ORACLES:
            ids, conf = ref_get_class_segments(refs[-1], min_count, min_conf)
            assert [(c.class_id, len(c.points)) for c in got] == [tuple(x) for x in ids.tolist()]
            np.testing.assert_allclose(np.array([[c.confidence_min, c.confidence_max] for c in got]).reshape(-1, 2), conf, rtol=0, atol=tol)
    both("merge_segments", 11, 11)
    both("remove_segment", 999)
    both("merge_segments", 12, 13)
    # remove_low_count_voxels / remove_low_confidence_voxels (voxel_block_grid.hpp:624-676; the oracles do not bind them): the oracle's
    # dump with the voxels below the threshold reset - count == n stays, n - 1 goes; confidence == threshold stays
    before = refs[0].dump()
    assert (before[1][..., 0] == 3).any() and (before[1][..., 0] == 2).any()
    gpu.g.remove_low_count_voxels(3)
    state = after_python_reset(before, before[1][..., 0] < 3)
    assert_dump_equal(gpu, state, kind)
    assert gpu.g.size() == int((state[1][..., 0] > 0).sum())
    t = away_from(0.5)
    if kind in EXACT:
        assert ((state[4] == 0.5) & (state[1][..., 0] > 0)).any() and ((state[4] > 0.5) & (state[1][..., 0] > 0)).any()
    gpu.g.remove_low_confidence_voxels(t)
    state = after_python_reset(state, state[4] < np.float32(t))
    assert_dump_equal(gpu, state, kind)
    assert gpu.g.size() == int((state[1][..., 0] > 0).sum()) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_merge_into_the_voxels_without_an_object_id_reaches_empty_voxels(kind):
    """merge_segments(7, -1): every voxel whose object id is -1 - empty ones included (voxel_block_semantic_grid.hpp: no count test) -
    becomes object 7; what follows sees them: an association call (the probabilistic voxels of class -1 now have no cached best
    pair and a log-probability of -inf), remove_segment of an absent id, remove_low_confidence_segments."""
    case = sp.segment_ops_case()
    gpu = GpuGrid(kind, case.bs)
    refs = [mk(kind, sp.VOXEL, case.bs) for mk in ORACLES]
    for g in [gpu] + refs:
        sp.drive(g, case)
    gpu.g.merge_segments(7, -1)
    for r in refs:
        r.merge_segments(7, -1)
        assert_state_equal(gpu, r, kind)
    if kind in EXACT:  # (an empty log-probability voxel has no class: its forced label is dropped again and it reads -1)
        ints = gpu.dump()[1]
        assert ((ints[..., 1] == 7) & (ints[..., 0] == 0)).sum() > (ints[..., 0] > 0).sum()  # the empty cells of every block
    call = [s[1] for s in case.steps if s[0] == "assoc"][0]
    again = sp.Case("again", case.bs, case.T, next_id=40).assoc(call["cls_img"], call["inst_img"])
    maps = [sp.drive(g, again)[0][0]["map"] for g in [gpu] + refs]
    assert all(m == maps[0] for m in maps)
    for op, arg in (("remove_segment", 999), ("remove_low_confidence_segments", 1)):
        getattr(gpu.g, op)(arg)
        for r in refs:
            getattr(r, op)(arg)
            assert_state_equal(gpu, r, kind)
            assert ids_multiset(*gpu.g.get_ids()) == ids_multiset(*r.get_ids())


def sorted_rows(points, colors, cls, obj, conf):
    order = np.lexsort(np.asarray(points).T[::-1])
    return [np.asarray(a)[order] for a in (points, colors, cls, obj, conf)]


@pytest.mark.parametrize("bs", [8, 12])
@pytest.mark.parametrize("kind", KINDS)
def test_a_full_block_flushes_the_row_windows_in_the_middle_of_a_scan(kind, bs):
    """get_voxels and get_object_segments on sp.dense_rows_case: one wave gets a whole block's rows, and its window of 512 flushes from
    inside a push once more than 448 wait - on the block's last push at block size 8 (512 rows, 504 keys), three times with rows of
    the same block still to come at block size 12 (1728 rows, 1716 keys; partial pushes where a count above 1 is asked for); five
    voxels go to another wave.  Row sets against the oracles and the planted numbers: positions, colours and ids exact, confidences
    to the file's tolerance.  get_voxels once more with output capacities below the row count - inside the first flush and between
    later ones: the count is still the whole count, the rows written are distinct rows of the full set (which ones is the order
    of the waves).  get_object_segments sizes its own output from a counting pass: there is no capacity to set."""
    import ctypes

    from pyslam_amd import _lib as L

    case = sp.dense_rows_case(bs)
    obj, rep = case.planted
    gpu = GpuGrid(kind, case.bs)
    refs = [mk(kind, sp.VOXEL, case.bs) for mk in ORACLES]
    for g in [gpu] + refs:
        sp.drive(g, case)
    tol = 0.0 if kind in EXACT else 2e-6
    total = bs ** 3 + 5
    assert gpu.g.size() == total == len(obj)
    for min_count in (1, 2):  # get_voxels keeps count >= min_count
        got = gpu.g.get_voxels(min_count, 0.0)
        rows = sorted_rows(got.points, got.colors, got.class_ids, got.object_ids, got.confidences)
        assert len(rows[0]) == int((rep >= min_count).sum())
        np.testing.assert_array_equal(np.sort(rows[3]), np.sort(obj[rep >= min_count]))
        for r in refs:
            exp = sorted_rows(*r.get_voxels(min_count, 0.0))
            for a, b in zip(rows[:4], exp[:4]):
                np.testing.assert_array_equal(a, b)
            np.testing.assert_allclose(rows[4], exp[4], rtol=0, atol=tol)
    for min_count in (0, 1):  # get_object_segments keeps count > min_count
        segs = gpu.g.get_object_segments(min_count, 0.0)
        planted = [(o, int(((obj == o) & (rep > min_count)).sum())) for o in (10, 11, 12)]
        assert [(int(o.object_id), len(o.points)) for o in segs.object_vector] == planted
        for r in refs:
            exp = r.get_object_segments(min_count, 0.0)
            assert [(int(o.object_id), int(o.class_id), len(o.points)) for o in segs.object_vector] == [(o["object_id"], o["class_id"], len(o["points"])) for o in exp]
            for a, b in zip(segs.object_vector, exp):
                for x, y in ((a.points, b["points"]), (a.colors, b["colors"])):
                    np.testing.assert_array_equal(x[np.lexsort(a.points.T[::-1])], y[np.lexsort(b["points"].T[::-1])])
                assert abs(a.confidence_min - b["conf_min"]) <= tol and abs(a.confidence_max - b["conf_max"]) <= tol
    got = gpu.g.get_voxels(1, 0.0)
    rows = sorted_rows(got.points, got.colors, got.class_ids, got.object_ids, got.confidences)
    full = {tuple(np.concatenate([rows[0][i], rows[1][i], [rows[2][i], rows[3][i], rows[4][i]]]).tolist()) for i in range(total)}
    assert len(full) == total
    for cap in (100, 460) + ((1100,) if bs == 12 else ()):
        out = [np.zeros((cap, 3), np.float64), np.zeros((cap, 3), np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float32)]
        n = ctypes.c_int64()
        L.check(gpu.g._lib.hv_get_voxels_semantic(gpu.g._h, 1, 0.0, *(L.ptr(a) for a in out), cap, ctypes.byref(n)))
        assert n.value == total
        some = {tuple(np.concatenate([out[0][i], out[1][i], [out[2][i], out[3][i], out[4][i]]]).tolist()) for i in range(cap)}
        assert len(some) == cap and some <= full


# ---- e. the vote kernel against the staged interface --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["many_pairs", "dense_pending"])
def test_vote_stage_hands_out_the_counted_pairs(kind, which):
    """assoc_pairs() after assoc_vote as a multiset of (instance, object, votes) against count_votes on the oracle's dump - for
    dense_pending the second call's stripes: 4 instances x (PENDING + SEEN)."""
    case = sp.many_pairs_case() if which == "many_pairs" else sp.dense_pending_case(8)
    gpu, port = GpuGrid(kind, case.bs), PortSemGrid2(kind, sp.VOXEL, case.bs)
    for g in (gpu, port):
        g.set_next_object_id(case.next_id)
        for s in case.steps:
            if s[0] == "integrate":
                g.integrate(s[1], s[2], s[3], s[4], None)
    a = [s[1] for s in case.steps if s[0] == "assoc"][1]
    expected = sp.count_votes(case, port.dump(), a)["pairs"]
    assert gpu.g.assoc_vote(gpu.frustum(sp.INTR, sp.W, sp.H, case.T, case.depth_max, case.depth_min), a["cls_img"], a["inst_img"], None, 0.25, False)
    got = unpack_pairs(*gpu.g.assoc_pairs())
    # a marker carries no votes: the vote stage counts the instance's pixels with a valid class into it, count_votes writes 1
    valid = a["inst_img"][(a["inst_img"] >= 0) & (a["cls_img"] >= 0)]
    assert {i: n for i, o, n in got if o == SEEN} == {int(i): int(n) for i, n in zip(*np.unique(valid, return_counts=True))}
    assert sorted((i, o, 1 if o == SEEN else n) for i, o, n in got) == expected
    assert len(expected) == (400 if which == "many_pairs" else 8)
    m = dict(gpu.g.assoc_decide(a["min_vote_ratio"], a["min_votes"]))
    assert m == decide(expected, a["min_vote_ratio"], a["min_votes"], case.next_id)[0]
