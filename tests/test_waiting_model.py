"""The WaitingOn model (waiting_model) pinned with hand-worked literals, and the generators (waiting_cases) checked for
coverage, so that no GPU case of test_waiting_gpu passes vacuously. Runs on the CPU."""
import numpy as np
import pytest

import waiting_cases as WC
import waiting_model as WM
from waiting_cases import READ, WRITE, EXCLUSIVE_SYNC_POINT, late, rcmd_upd, tid, waiters_of


def states(view, r):
    return list(view["dep_state"][view["dep_off"][r]:view["dep_off"][r + 1]])


def eal(view, r):
    return (int(view["eal_msb"][r]), int(view["eal_lsb"][r]), int(view["eal_node"][r]))


@pytest.mark.parametrize("range_waiter,want", [(True, [2, 1, 1, 2, 0, 2, 1]), (False, [0, 1, 1, 0, 0, 0, 1])])
def test_each_step(range_waiter, want):
    """slots E, D0, D0b, D2, D3, D4, D5 of W: E cleared by D4's propagation alone (2 in a range-domain W, 0 in a
    key-domain one), step 0 twice, step 2, step 3, step 4, step 5"""
    steps, ids = WC.literal_steps(range_waiter)
    res, store, _ = WC.run_model(steps)
    assert res[1]["out"]["waiting"].tolist() == [0]                      # R finished as it registered
    assert states(res[1]["view"], 0) == [2]
    v = res[3]["view"]
    r = 1                                                                # W (hlc 500) sorts after D4 (hlc 150)
    assert (int(v["msb"][r]), int(v["flags"][r])) == (500, 2 if range_waiter else 0)
    assert states(v, r) == want
    assert res[3]["out"]["waiting"].tolist() == [3 + 2]
    assert (int(v["n_wait_dep"][r]), int(v["n_wait_key"][r]), int(v["next_waiting_on"][r])) == (3, 2, 6)
    assert res[3]["stats"] == dict(register_evaluated=7, propagated=1)
    assert store.trace == {0: 2, 1: 0, 2: 2, 3: 1, 4: 1, 5: 1}           # (step 2 also fired for R's dep)
    assert store.prop_beyond_own == 1
    assert eal(v, r) == WM.ZERO


def test_awaits_only_deps():
    """an ExclusiveSyncPoint never takes step 3 and raises executeAtLeast to the max executeAt above its TxnId"""
    A, B, C_, D = (tid(100 + 10 * i, READ, 1) for i in range(4))
    W = tid(500, EXCLUSIVE_SYNC_POINT, 1)
    steps = [("rcmd", rcmd_upd([(A, 5, late(A)), (B, 5, (50_900, B[1], B[2])), (C_, 10, C_), (D, 10, (60_000, D[1], D[2]))])),
             ("register", waiters_of([dict(txn=W, x=W, keys=[], deps=[A, B, C_, D])]))]
    res, store, _ = WC.run_model(steps)
    v = res[1]["view"]
    assert states(v, 0) == [1, 1, 2, 2]                                  # late Stable deps still wait (no step 3)
    assert store.trace[3] == 0 and store.trace[1] == 2                   # D is Invalidated: its executeAt is not known
    assert eal(v, 0) == (50_900, B[1], B[2])
    assert int(v["flags"][0]) == 3


def descending_case(w_kind, w_dom):
    E, D = tid(100, READ, 1), tid(200, READ, 1)
    W = tid(500, w_kind, w_dom)
    return [("rcmd", rcmd_upd([(E, 10, E), (D, 5, D)])),
            ("register", waiters_of([dict(txn=D, x=D, keys=[], deps=[E])])),
            ("rcmd", rcmd_upd([(E, 5, late(E)), (D, 8, D)])),
            ("register", waiters_of([dict(txn=W, x=W, keys=[], deps=[E, D])]))]


def test_descending_walk():
    """E < D, D Applied with R_D.dep_state[E] == 2, E executing after W: D is visited first and its propagation leaves E
    at 2; E's own branch (step 3), which an ascending walk would take first, would leave 0"""
    steps = descending_case(READ, 1)
    res, store, _ = WC.run_model(steps)
    assert states(res[3]["view"], 1) == [2, 2]
    assert store.trace[3] == 0
    w = store.recs[WM.order(tid(500, READ, 1))]
    assert WM.branch(w, tid(100, READ, 1), {WM.order(tid(100, READ, 1)): (5, late(tid(100, READ, 1)))})[0] == 3


def test_propagation_into_key_domain():
    res, _, _ = WC.run_model(descending_case(WRITE, 0))
    assert states(res[3]["view"], 1) == [0, 0]


@pytest.mark.parametrize("n", [63, 64, 65])
def test_word_boundary(n):
    """every waiting slot below n_dep is visited once: with 65 txnIds slot 64 is cleared too (the reference's ranged
    reverseForEach would index word 0 twice and never reach it: the documented divergence)"""
    pool = [tid(100 + i, READ, 1) for i in range(n)]
    W = tid(5000, READ, 1)
    res, store, _ = WC.run_model([("rcmd", rcmd_upd([(p, 10, p) for p in pool])),
                                  ("register", waiters_of([dict(txn=W, x=W, keys=[3], deps=pool)]))])
    assert states(res[1]["view"], 0) == [2] * n
    assert store.trace[2] == n
    assert res[1]["out"]["waiting"].tolist() == [1]
    (waiting, applied), = store.bitsets()
    assert len(waiting) == (n + 1 + 63) // 64 and len(applied) == (n + 63) // 64
    assert sum(bin(w & (2 ** 64 - 1)).count("1") for w in applied) == n
    assert waiting[n >> 6] & (2 ** 64 - 1) == 1 << (n & 63) and sum(1 for w in waiting if w) == 1   # the key: bit n_dep + 0


def test_bitset_packing():
    """txn i is bit i, key k is bit n_dep + k; Java longs are signed; a key-domain record has no appliedOrInvalidated"""
    from accord_amd.deps import waiting_bitsets
    pool = [tid(100 + i, READ, 1) for i in range(64)]
    Wr, Wk = tid(5000, READ, 1), tid(5001, WRITE, 0)
    steps = [("rcmd", rcmd_upd([(pool[0], 10, pool[0])])),
             ("register", waiters_of([dict(txn=Wr, x=Wr, keys=[1, 2], key_wait=[0, 1], deps=pool),
                                      dict(txn=Wk, x=Wk, keys=[5], deps=pool[:2])]))]
    res, store, _ = WC.run_model(steps)
    want = [([-2, 2], [1]), ([2 | 4], None)]      # Wr: deps 1..63 wait = 0xFFFF...FE = -2, key 1 of 2 = bit 65; Wk: dep 1, key 0
    assert store.bitsets() == want
    assert waiting_bitsets(res[1]["view"]) == want


def test_release_pairs():
    """a key release alone makes a record ready; a pair with no record, an unknown key or a clear bit is ignored; until
    raises executeAtLeast of an awaits-only-deps record only when strictly above"""
    W = tid(5000, EXCLUSIVE_SYNC_POINT, 1)
    U1, U2 = (9000, 2, 1), (9500, 2, 1)
    steps = [("register", waiters_of([dict(txn=W, x=W, keys=[4, 8], deps=[])])),
             ("notify", WC.ts_cols([]), WC.releases_of([(W, 4, 1, U2), (W, 4, 1, U1), (W, 5, 1, WM.ZERO),
                                                        (tid(1, READ, 1), 4, 1, WM.ZERO), (W, 8, 0, WM.ZERO)])),
             ("notify", None, WC.releases_of([(W, 8, 1, WM.ZERO)]))]
    res, store, _ = WC.run_model(steps)
    assert res[1]["stats"] == dict(notify_slots=0, propagated=0, key_released=1, key_ignored=3, ready=0)
    assert res[1]["out"]["n_changed"] == 1 and eal(res[1]["view"], 0) == U2
    assert res[2]["out"]["ready_rec"].tolist() == [0] and res[2]["out"]["ready_eal"] == [U2]
    assert store.ready_by == dict(key=1, dep=0, both=0)


def test_applied_dep_still_waiting():
    """the step-4 invariant: IllegalState, store unchanged"""
    D, X, W = tid(100, READ, 1), tid(50, READ, 1), tid(5000, READ, 1)
    steps = [("rcmd", rcmd_upd([(D, 5, D), (X, 5, X)])),
             ("register", waiters_of([dict(txn=D, x=D, keys=[], deps=[X])])),
             ("rcmd", rcmd_upd([(D, 8, D)])),
             ("register", waiters_of([dict(txn=W, x=W, keys=[], deps=[D])]))]
    res, store, _ = WC.run_model(steps)
    assert res[3]["error"] == "state" and len(store.recs) == 1
    for k, a in res[1]["view"].items():
        np.testing.assert_array_equal(a, res[3]["view"][k], err_msg=k)


@pytest.mark.parametrize("seed", WC.SEEDS)
def test_chain_coverage(seed):
    steps = WC.chain(seed)
    res, store, _ = WC.chain_model(seed)
    assert [s[0] for s in steps] == ["rcmd", "register", "rcmd", "register", "rcmd", "notify", "notify", "erase", "rcmd", "notify"]
    assert all(r["error"] is None for r in res)
    assert all(store.trace[s] > 0 for s in range(6)), store.trace
    assert store.prop_beyond_own > 0
    assert all(store.ready_by[k] > 0 for k in ("key", "dep", "both")), store.ready_by
    v = res[3]["view"]
    nd = np.diff(v["dep_off"].astype(np.int64))
    assert 280 <= len(nd) <= 320 and nd.max() >= 129 and nd.min() == 0
    assert set(WC.EDGE_DEPS) <= set(nd.tolist())
    assert sum(r["stats"].get("propagated", 0) for r in res) > 0
    assert res[5]["stats"]["key_ignored"] > 0 and res[5]["stats"]["key_released"] > 0
    assert 0 < res[5]["stats"]["notify_slots"] < res[6]["stats"]["notify_slots"]     # changed, then NULL
    last = res[-1]["view"]
    assert len(last["msb"]) > 0 and not last["n_wait_dep"].any() and not last["n_wait_key"].any()
    assert len(res[-1]["out"]["ready_rec"]) > 0


def test_edge_case_shapes():
    for total in (8191, 8192, 8193):
        steps, pool, ws = WC.edge_case(WC.EDGE_DEPS, total)
        assert steps[1][1]["dep_off"][-1] == total
    steps, pool, ws = WC.edge_case(WC.EDGE_DEPS)
    res, _, _ = WC.run_model(steps)
    assert res[1]["stats"]["register_evaluated"] == sum(WC.EDGE_DEPS)
    assert res[1]["out"]["waiting"].tolist() == [n + 1 for n in WC.EDGE_DEPS]
