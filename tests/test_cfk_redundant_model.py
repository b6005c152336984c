"""Properties of the RedundantBefore model (cfk_redundant_model.py) that the GPU tests of acc_cfk_redundant_before rest
on (no GPU): idempotence, a bound below everything, missing[] closed over the key's entries after a prune, and the
hand-worked case of CommandsForKey.withRedundantBefore (local/CommandsForKey.java:1654-1684); and what the case builders
of cfk_redundant_cases.py must give (sizes past a scan tile, keys that leave, ids equal to a bound, the hand-worked
order edges), so a parameter set that stops giving it fails here."""
import numpy as np
import pytest

import cfk_cases as CC
import cfk_redundant_cases as RCS
import cfk_redundant_model as M
import oracle

SEEDS = (5, 7)     # as test_cfk_redundant_gpu.py


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


@pytest.fixture(scope="module")
def mid_state():
    upd = CC.cfk_case(SEEDS[0], n_txn=300, n_keys=12, p_accinv=0)
    part, _ = CC.split_updates(upd, len(upd["msb"]) * 2 // 5)
    return oracle.cfk_apply(CC.empty_snapshot(), part)


def test_handmade():
    upd, ranges, before, after = M.handmade()
    state = oracle.cfk_apply(CC.empty_snapshot(), upd)
    assert M.describe(state) == before
    m = M.BoundMap(1)
    counts = {}
    pruned = M.with_redundant_before(state, M.BoundMap(1).get, m.add(ranges).get, counts)
    assert M.describe(pruned) == after
    # entries: A, B of 200; A..D of 300; all five of 400. missing ids: one each of D and E on 200; D's two with D and E's
    # two on 300; the four of 400
    assert counts == dict(keys_advanced=4, entries_dropped=11, missing_dropped=10)


def test_a_second_identical_call_changes_nothing(mid_state):
    ranges = M.chain_bounds("three", 1, 300)
    m0, m1 = M.BoundMap(1), M.BoundMap(1).add(ranges)
    once = M.with_redundant_before(mid_state, m0.get, m1.get)
    assert len(once["status"]) < len(mid_state["status"])
    counts = {}
    twice = M.with_redundant_before(once, m1.get, m1.copy().add(ranges).get, counts)
    assert same(once, twice)
    assert counts == dict(keys_advanced=0, entries_dropped=0, missing_dropped=0)


def test_a_bound_below_every_txn_id_changes_nothing(mid_state):
    m = M.BoundMap(1).add(M.ranges_of([(M.KEY_LO, M.KEY_HI, M.ts(1))]))
    counts = {}
    out = M.with_redundant_before(mid_state, M.BoundMap(1).get, m.get, counts)
    assert same(out, mid_state)
    assert counts == dict(keys_advanced=len(mid_state["key"]), entries_dropped=0, missing_dropped=0)


@pytest.mark.parametrize("variant", ["single", "three"])
@pytest.mark.parametrize("seed", SEEDS)
def test_after_a_prune_every_missing_id_is_an_entry_of_its_key(seed, variant):
    upd = CC.cfk_case(seed, n_txn=300, n_keys=12, p_accinv=0)
    prunes = [s for s in M.chained_case(upd, variant, oracle.cfk_apply) if s["op"] == "prune"]
    assert len(prunes) == M.N_BATCHES - 1
    for s in prunes:
        st = s["state"]
        assert len(st["mmsb"]) > 0
        for k in range(len(st["key"])):
            e0, e1 = int(st["ent_off"][k]), int(st["ent_off"][k + 1])
            ids = {M.order((st["emsb"][e], st["elsb"][e], st["enode"][e])) for e in range(e0, e1)}
            for j in range(int(st["miss_off"][e0]), int(st["miss_off"][e1])):
                assert M.order((st["mmsb"][j], st["mlsb"][j], st["mnode"][j])) in ids


def test_the_map_is_the_pointwise_max():
    m = M.BoundMap(1).add(M.ranges_of([(10, 20, M.ts(8)), (20, 30, M.ts(4))]))
    m.add(M.ranges_of([(15, 25, M.ts(6))]))
    assert [m.get(k) for k in (10, 11, 15, 16, 20, 21, 25, 26, 30, 31)] == [
        M.NONE, M.ts(8), M.ts(8), M.ts(8), M.ts(8), M.ts(6), M.ts(6), M.ts(4), M.ts(4), M.NONE]
    assert m.intervals() == [(11, 20, M.order(M.ts(8))), (21, 25, M.order(M.ts(6))), (26, 30, M.order(M.ts(4)))]
    half_open = M.BoundMap(0).add(M.ranges_of([(10, 20, M.ts(8))]))
    assert half_open.get(10) == M.ts(8) and half_open.get(20) == M.NONE


def test_trim_deps_keeps_a_dep_equal_to_the_bound():
    upd, _, _, _ = M.handmade()
    t12 = M.ts(12)
    out, removed = M.trim_deps(upd, lambda key: t12 if key == 200 else M.NONE)
    # on key 200: D's [A] -> [], E's [A, C] -> [C]; the other keys keep theirs
    assert removed == 2
    do = out["dep_off"].astype(int)
    pairs = {(int(out["lsb"][u]) >> 16, int(out["key"][j])): [int(x) >> 16 for x in out["dlsb"][do[j]:do[j + 1]]]
             for u in range(len(out["msb"])) for j in range(int(out["key_off"][u]), int(out["key_off"][u + 1]))}
    assert pairs[(16, 200)] == [] and pairs[(20, 200)] == [12]
    assert pairs[(16, 100)] == [4] and pairs[(20, 300)] == [4, 12]


# ---------------------------------------------------------------- the case builders of cfk_redundant_cases.py

def test_call_map_agrees_with_bound_map():
    """CallMap (bisection per call) against BoundMap (every update walked): lookups at every range edge and beside it,
    and the intervals, over two overlapping calls of the scale chain's shape and a call with a tie"""
    edge = list(range(0, 6001, 10))
    call = lambda b: M.ranges_of([(edge[r], edge[r + 1], M.ts(4 * (100 * b + r % 7) + 4, node=1 + r % 3))  # noqa: E731
                                  for r in range(600) if r % 2 == b % 2 or r % 5 == 0])
    slow, fast = M.BoundMap(1), RCS.CallMap(1)
    for ranges in (call(0), call(1), M.ranges_of([(95, 205, M.ts(4 * 103 + 4, flags=(1 << 1) | RCS.FLAG, node=1))])):
        slow.add(ranges)
        fast.add(ranges)
        keys = sorted({e + d for e in edge[:80] + edge[-40:] for d in (-1, 0, 1, 2)})
        assert [fast.get(k) for k in keys] == [slow.get(k) for k in keys]
        assert fast.copy().intervals() == slow.intervals()
    assert len(fast.intervals()) > RCS.MC_BLK


@pytest.mark.parametrize("dist", ["uniform", "zipf"])
def test_scale_chain_meets_its_conditions(dist):
    RCS.scale_conditions(RCS.scale_chain(dist), dist)


def test_replica_case_meets_its_conditions():
    RCS.replica_conditions(RCS.replica_case())


def test_order_edges_by_hand():
    """the hand-written states and counts of cfk_redundant_cases.order_edges are what the model and the C restatement
    give; the ids are ordered as the comments there say"""
    I = RCS.EDGE_IDS
    names = ["P", "N", "Q", "E1", "E2", "T", "U"]
    assert [M.order(I[a]) < M.order(I[b]) for a, b in zip(names, names[1:])] == [True] * 6
    assert I["N"][:2] == I["Q"][:2] and (I["N"][2], I["Q"][2]) == (-1, 2)
    assert I["E1"][1:] == I["E2"][1:] and I["E1"][0] != I["E2"][0]
    assert RCS.E1F != I["E1"] and M.order(RCS.E1F) == M.order(I["E1"]) and M.order(RCS.QF) == M.order(I["Q"])
    steps = RCS.order_edges_model()
    assert [len(st["key"]) for _, _, st, _ in steps] == [3] * 5
    assert [len(st["status"]) for _, _, st, _ in steps] == [18, 12, 12, 9, 12]


def test_small_script_runs_on_the_model():
    m, state = M.BoundMap(1), CC.empty_snapshot()
    dropped = trimmed = 0
    for op, arg in RCS.small_script():
        step, state = (RCS.apply_step if op == "apply" else RCS.prune_step)(state, m, arg)
        CC.snap_as_batch(state)
        dropped += step["counts"]["entries_dropped"] if op == "prune" else 0
        trimmed += step["trimmed"] if op == "apply" else 0
    assert dropped > 0 and trimmed > 0 and len(state["key"]) > 0
