"""CPU: the planted semantic cases of tests/semantic_planted.py proven before any GPU test uses them.  Every association call is
predicted by tests/assoc_rules_reference.py (rules) on the votes tests/semantic_planted.count_votes (visit predicate) counts on the
grid's dump, and must come out of oracle.semantic.PortSemGrid2 (the C restatement) and - where it is built - RefSemGrid2 (the
compiled reference) alike: three restatements that share no code.  The branch-reach assertions make sure each builder really
drives the path it is meant for (they are conditions on the inputs, counted on the oracle side, not measurements)."""
import numpy as np
import pytest

import oracle
from oracle.semantic import PortSemGrid2, RefSemGrid2
from tests import semantic_planted as sp
from tests.assoc_rules_reference import PENDING, SEEN, decide, pack_pairs, unpack_pairs

need_ref = pytest.mark.skipif(not oracle.ref_available(), reason="compiled reference not available")
GRIDS = [pytest.param(PortSemGrid2, id="port"), pytest.param(RefSemGrid2, id="ref", marks=need_ref)]

CASES = ([(f"frustum_edge-{bs}", lambda bs=bs: sp.frustum_edge_case(bs)) for bs in (4, 5, 8, 16)]
         + [(f"label-{bs}", lambda bs=bs: sp.label_case(bs)) for bs in (4, 5, 8, 16)]
         + [(f"depth_filter-{bs}-{v}", lambda bs=bs, v=v: sp.depth_filter_case(bs, v)) for bs in (5, 8) for v in sp.DEPTH_VARIANTS]
         + [(f"dense_pending-{bs}", lambda bs=bs: sp.dense_pending_case(bs)) for bs in (5, 8)]
         + [("many_pairs", sp.many_pairs_case), ("overflow_label", sp.overflow_label_case)]
         + [(f"carve-{w}-{bs}", lambda bs=bs, w=w: sp.carve_case(bs, w)) for bs in (5, 8) for w in ("depth", "edge")])


def kinds_of(name):
    return (1, 3) if name == "overflow_label" else sp.KINDS


def test_rules_reference_on_hand_worked_votes():
    """The restated rules on votes small enough to do by hand (voxel_semantic_data_association.h:284-353)."""
    assert decide([(4, 2, 1), (4, 3, 1)], 0.5, 1, 20) == ({4: 2}, 20)                      # tie: the smaller id, ratio 1/2 is not < 1/2
    assert decide([(4, 2, 1), (4, 3, 1)], 0.5000001, 1, 20) == ({4: -1}, 20)
    assert decide([(4, 2, 2), (4, 3, 1)], 0.5, 4, 20) == ({4: -1}, 20)                     # 3 votes < min_votes 4
    assert decide([(4, 2, 2), (4, 2, 1), (4, 3, 2)], 0.6, 1, 20) == ({4: 2}, 20)           # equal pairs add up: 3 of 5
    assert decide([(4, PENDING, 2), (4, 5, 2), (4, 9, 2)], 0.25, 1, 3) == ({4: 3}, 4)      # new id 3 sorts first and wins the tie
    assert decide([(4, PENDING, 2), (4, 5, 2), (4, 9, 2)], 0.25, 1, 5) == ({4: 5}, 6)      # new id 5 IS object 5: 4 votes
    assert decide([(4, PENDING, 2), (4, 5, 2), (4, 9, 2)], 0.25, 1, 12) == ({4: 5}, 13)
    assert decide([(7, PENDING, 1), (3, PENDING, 1)], 0.5, 1, 8) == ({3: 8, 7: 9}, 10)      # ascending instance order
    assert decide([(3, SEEN, 1), (0, SEEN, 1), (0, 6, 5)], 0.5, 1, 8) == ({3: -1, 0: 0}, 8)
    assert decide([], 0.5, 1, 8) == ({}, 8)
    pairs = sp.random_pairs(500, 3)
    assert unpack_pairs(*pack_pairs(pairs)) == sorted(pairs)
    assert len(set((i, o) for i, o, _ in pairs)) < len(pairs) and any(i == 0 for i, _, _ in pairs)  # duplicates, instance 0


def test_every_case_fits_the_limits():
    for name, make in CASES:
        c = make()
        assert 1 <= c.n_blocks() <= 64, (name, c.n_blocks())
        assert max(len(s[1]) for s in c.steps if s[0] == "integrate") <= 4096, name


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_planted_case_is_what_the_rules_reference_predicts(grid, name, make):
    """drive(): map, next id and permutation discipline of every call; then the branch each builder is for."""
    for kind in kinds_of(name):
        case = make()
        g = grid(kind, sp.VOXEL, case.bs)
        records, _ = sp.drive(g, case)
        assert g.num_blocks() == case.n_blocks()
        votes = [r["votes"] for r in records]
        if name.startswith("dense_pending"):
            assert votes[0]["pending"] >= 600 and votes[1]["pending"] == votes[0]["pending"] and votes[2]["pending"] == 0
            assert records[0]["map"] == {4: -1} and sorted(records[1]["map"].values()) == [4, 5, 6, 7] and records[2]["map"] == records[1]["map"]
        elif name == "many_pairs":
            real = [p for p in votes[0]["pairs"] if p[1] != SEEN]
            assert len(real) == 300 > 64 and len(votes[0]["pairs"]) == 400 and votes[0]["pairs"] == case.pairs
            assert all(o >= 0 for o in records[0]["map"].values()) and records[1]["map"] == records[0]["map"]
        elif name.startswith("frustum_edge"):
            pr = votes[0]["projection"]
            for plane in sp.PLANES:
                assert pr["rejected"][plane].sum() == 1, plane  # exactly the voxel planted beyond that plane
            assert votes[0]["visited"] == sum(case.expected_inside) == 6
            keys, ints, pos, _, _ = g.dump()
            inside_pos = {tuple(p) for p in (pos[pr["block"], pr["cell"]] / ints[pr["block"], pr["cell"], 0][:, None])[pr["inside"]]}
            assert inside_pos == {tuple(p) for p, ok in zip(sp.to_world(case.points, case.T), case.expected_inside) if ok}
            on_63 = [(int(u), int(v)) for u, v, i in zip(pr["u"], pr["v"], pr["inside"]) if i]
            assert any(u == 63 for u, _ in on_63) and any(v == 47 for _, v in on_63) and any(u == 0 for u, _ in on_63) and any(v == 0 for _, v in on_63)
            assert keys.min() < 0 <= keys.max()
        elif name.startswith("depth_filter"):
            variant = name.split("-")[2]
            n_ok = dict(filter=5, carve=4, no_depth=10, wrong_shape=10)[variant]  # per row of ten voxels
            assert votes[0]["pending"] == n_ok and votes[0]["carved"] == (2 if variant == "carve" else 0)
            assert dict((o, n) for _, o, n in votes[0]["pairs"] if o != SEEN) == {PENDING: n_ok, 2: n_ok}
            assert records[0]["map"] == {5: 2}  # a tie between object 2 and the new id 7 at ratio exactly 1/2
        elif name.startswith("label"):
            assert votes[0]["pairs"] == sorted([(0, 0, 24), (0, SEEN, 1), (6, PENDING, 32), (6, 2, 16), (6, 9, 16), (6, SEEN, 1), (8, SEEN, 1)])
            assert records[0]["map"] == {0: 0, 6: 5, 8: -1}
            assert votes[1]["pairs"] == sorted([(0, 0, 24), (0, SEEN, 1), (6, 2, 16), (6, 5, 32), (6, 9, 16), (6, SEEN, 1), (8, SEEN, 1)])
        elif name == "overflow_label":
            assert [r["map"] for r in records] == [{5: 2}, {5: 2}] and votes[0]["pairs"] == sorted([(5, 2, 3), (5, SEEN, 1)])
            if kind == 1 and grid is PortSemGrid2:
                most, hist = g.label_histogram()
                assert most == 13 and hist[13] == 2 and hist[7] == 1


@need_ref
@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_port_and_compiled_reference_agree_on_the_planted_case(name, make):
    """Same canonical maps, same next ids, same votes and - object ids made canonical - the same voxel records after the last step."""
    for kind in kinds_of(name):
        case = make()
        a, b = PortSemGrid2(kind, sp.VOXEL, case.bs), RefSemGrid2(kind, sp.VOXEL, case.bs)
        ra, ca = sp.drive(a, case)
        rb, cb = sp.drive(b, case)
        assert [(r["map"], r["next_id"]) for r in ra] == [(r["map"], r["next_id"]) for r in rb]
        for x, y in zip(sp.canonical_dump(a.dump(), ca), sp.canonical_dump(b.dump(), cb)):
            np.testing.assert_array_equal(x, y)


SCENES = sp.rule_scenes()


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name,pairs,ratio,min_votes,next_id", SCENES, ids=[s[0] for s in SCENES])
def test_rule_scene_casts_its_pairs_and_decides_like_the_rules_reference(grid, name, pairs, ratio, min_votes, next_id):
    for kind in sp.KINDS:
        case = sp.scene_from_pairs(name, pairs, ratio, min_votes, next_id)
        g = grid(kind, sp.VOXEL, case.bs)
        (rec,), to_canon = sp.drive(g, case)
        assert rec["votes"]["pairs"] == case.pairs and not to_canon  # one instance at most needs an id: nothing to permute
        assert (rec["map"], rec["next_id"]) == decide(pairs + [(i, SEEN, 1) for i, _, _ in pairs], ratio, min_votes, next_id)


def test_rule_scenes_decide_what_they_were_built_for():
    got = {name: decide(pairs, ratio, mv, nid)[0] for name, pairs, ratio, mv, nid in SCENES}
    assert got["ratio_half_at_0.5"] == {4: 2} and got["ratio_half_at_third"] == {4: 2} and got["ratio_half_at_two_thirds"] == {4: -1}
    assert got["ratio_third_at_third"] == {4: 2} and got["ratio_third_at_0.5"] == {4: -1}
    assert got["ratio_two_thirds_at_two_thirds"] == {4: 2} and got["ratio_two_thirds_at_0.5"] == {4: 2}
    assert got["total_equals_min_votes"] == {4: 2} and got["total_below_min_votes"] == {4: -1}
    assert got["tie_later_object_smaller_id"] == {4: 3, 6: 0} and got["tie_three_way_with_instance_0"] == {0: 1, 4: 7}
    assert [got[f"new_id_{k}"][4] for k in ("below", "equal", "between", "above")] == [3, 5, 5, 5]
    assert got["new_id_equal_to_the_larger"] == {4: 9} and got["seen_only_and_instance_0"] == {3: -1, 0: 0, 4: 2}
