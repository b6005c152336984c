"""Properties of the RedundantBefore model (cfk_redundant_model.py) that the GPU tests of acc_cfk_redundant_before rest
on (no GPU): idempotence, a bound below everything, missing[] closed over the key's entries after a prune, and the
hand-worked case of CommandsForKey.withRedundantBefore (local/CommandsForKey.java:1654-1684)."""
import numpy as np
import pytest

import cfk_cases as CC
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
