"""GPU parity for acc_waiting_* (WaitingStore over a real RangeCmdStore; ReplicaStore.execution_step).

Expected values come from the literal Python model (waiting_model, replayed by waiting_cases.run_model). Every
comparison is exact: the whole view, the outputs and the stats after every step."""
import numpy as np
import pytest

import waiting_cases as WC
import waiting_model as WM
from accord_amd import _lib as L
from waiting_cases import READ, WRITE, rcmd_upd, tid, ts_cols, waiters_of

pytestmark = pytest.mark.gpu

TIERS = (0, L.ACC_WT_TIER_LANE, L.ACC_WT_TIER_WAVE)
E_ARG, E_STATE, E_CAP = -1, -2, -5


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


class Stores:
    def __init__(self, ctx):
        from accord_amd.deps import RangeCmdStore, WaitingStore
        self.ctx = ctx
        self.rcmd = RangeCmdStore(ctx)
        self.w = WaitingStore(ctx, self.rcmd)

    def close(self):
        self.w.close()
        self.rcmd.close()


def triples(g, p):
    return [(int(a), int(b), int(c)) for a, b, c in zip(g[p + "msb"], g[p + "lsb"], g[p + "node"])]


def assert_view(got, want, msg):
    assert sorted(got) == sorted(want), msg
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{msg}: {k}")


def step_device(s, st, tier=0, device=False):
    if st[0] == "rcmd":
        s.rcmd.update(st[1])
        return None
    if st[0] == "register":
        return s.w.register(st[1], tier=tier, device=device)
    if st[0] == "notify":
        return s.w.notify(st[1], st[2], tier=tier, device=device)
    s.w.erase(st[1], device=device)
    return None


def assert_step(ctx, s, st, got, want, msg):
    """one step's outputs, stats and the whole view against the model's"""
    stats = ctx.stats()
    view = s.w.view()
    assert_view(view, want["view"], msg)
    from accord_amd.deps import waiting_bitsets
    assert s.w.bitsets(view) == waiting_bitsets(want["view"]), msg
    if st[0] == "register":
        np.testing.assert_array_equal(got["waiting"], want["out"]["waiting"], err_msg=msg)
        assert triples(got, "eal_") == [tuple(e) for e in want["out"]["eal"]], msg
        assert (stats["wt.register_evaluated"], stats["wt.propagated"]) == (
            want["stats"]["register_evaluated"], want["stats"]["propagated"]), msg
    elif st[0] == "notify":
        o = want["out"]
        np.testing.assert_array_equal(got["ready_rec"], o["ready_rec"], err_msg=msg)
        assert triples(got, "ready_") == [tuple(t) for t in o["ready_txn"]], msg
        assert triples(got, "ready_eal_") == [tuple(t) for t in o["ready_eal"]], msg
        assert got["n_changed"] == o["n_changed"], msg
        assert {k: stats["wt." + k] for k in want["stats"]} == want["stats"], msg
    elif st[0] == "erase":
        assert stats["wt.erased"] == want["stats"]["erased"], msg
    if st[0] != "rcmd":
        v = want["view"]
        assert (stats["wt.records"], stats["wt.slots"]) == (len(v["msb"]), len(v["key"]) + len(v["dmsb"])), msg


def replay(ctx, steps, res, tier=0, device=False, msg=""):
    s = Stores(ctx)
    try:
        for i, (st, want) in enumerate(zip(steps, res)):
            assert want["error"] is None
            got = step_device(s, st, tier, device)
            if st[0] != "rcmd":
                assert_step(ctx, s, st, got, want, f"{msg} step {i} {st[0]} tier {tier}")
    finally:
        s.close()


# ---------------------------------------------------------------- 1. the literals, through every tier

def literal_cases():
    import test_waiting_model as TM
    W = tid(5000, WC.EXCLUSIVE_SYNC_POINT, 1)
    A, B = tid(100, READ, 1), tid(110, READ, 1)
    return dict(
        range_waiter=WC.literal_steps(True)[0], key_waiter=WC.literal_steps(False)[0],
        descending=TM.descending_case(READ, 1), into_key_domain=TM.descending_case(WRITE, 0),
        awaits_only_deps=[("rcmd", rcmd_upd([(A, 5, WC.late(A)), (B, 10, (60_000, B[1], B[2]))])),
                          ("register", waiters_of([dict(txn=W, x=W, keys=[4, 8], deps=[A, B])])),
                          ("notify", ts_cols([]), WC.releases_of([(W, 4, 1, (90_000, 2, 1)), (W, 4, 1, (80_000, 2, 1)),
                                                                  (W, 5, 1, WM.ZERO), (tid(1, READ, 1), 4, 1, WM.ZERO)])),
                          ("rcmd", rcmd_upd([(A, 8, WC.late(A))])),
                          ("notify", ts_cols([A]), WC.releases_of([(W, 8, 1, WM.ZERO)]))])


@pytest.mark.parametrize("tier", TIERS)
def test_literals(ctx, tier):
    for name, steps in literal_cases().items():
        res, _, _ = WC.run_model(steps)
        replay(ctx, steps, res, tier, msg=name)


# ---------------------------------------------------------------- 2. the seeded chains

@pytest.mark.parametrize("seed,tier", [(s, 0) for s in WC.SEEDS] + [(WC.SEEDS[0], t) for t in TIERS[1:]])
def test_chain(ctx, seed, tier):
    res, _, _ = WC.chain_model(seed)
    replay(ctx, WC.chain(seed), res, tier, msg=f"seed {seed}")


# ---------------------------------------------------------------- 3. edge shapes

@pytest.mark.parametrize("total", [None, 8191, 8192, 8193])
def test_edge_shapes(ctx, total):
    """dep counts around WT_LANE_MAX and the 64-bit word; total slots around one u32 scan tile (256 x 32); changed of
    size 0, 1, every dep and NULL; the last step clears every record"""
    base, pool, ws = WC.edge_case(WC.EDGE_DEPS, total)
    every = [(w["txn"], k, 1, WM.ZERO) for w in ws for k in w["keys"]]
    steps = list(base) + [("notify", ts_cols([]), None), ("notify", ts_cols(pool[:1]), None),
                          ("notify", ts_cols(pool[1:]), None), ("notify", None, WC.releases_of(every))]
    res, store, _ = WC.run_model(steps)
    assert [r["stats"]["notify_slots"] for r in res[3:]] == [0, len(ws) - 1, sum(max(len(w["deps"]) - 1, 0) for w in ws), 0]
    assert not res[-1]["view"]["n_wait_dep"].any() and not res[-1]["view"]["n_wait_key"].any()
    for tier in TIERS if total is None else (0,):
        replay(ctx, steps, res, tier, msg=f"edge {total}")


def test_empty_store(ctx):
    s = Stores(ctx)
    try:
        want = WM.Store().view()
        assert_view(s.w.view(), want, "empty")
        g = s.w.notify(None, WC.releases_of([(tid(1, READ, 1), 4, 1, WM.ZERO)]))
        assert len(g["ready_rec"]) == 0 and g["n_changed"] == 0 and ctx.stats()["wt.key_ignored"] == 1
        g = s.w.notify(ts_cols([tid(1, READ, 1)]), None)
        assert len(g["ready_rec"]) == 0
        s.w.erase(ts_cols([tid(1, READ, 1)]))
        assert ctx.stats()["wt.erased"] == 0
        g = s.w.register(waiters_of([]))
        assert len(g["waiting"]) == 0
        assert_view(s.w.view(), want, "empty after no-ops")
    finally:
        s.close()


# ---------------------------------------------------------------- 4. errors leave the store unchanged

_ONE = np.zeros(2, np.uint64)   # a non-NULL pointer for an empty column


def raw_register(s, w, mem=0, tier=0, **over):
    """acc_waiting_register with the counts and tier as given (the wrapper derives them)"""
    import ctypes as C
    a = {k: np.ascontiguousarray(w[k]) for k in w}
    p = lambda k: a[k].ctypes.data if len(a[k]) else _ONE.ctypes.data  # noqa: E731
    ri = L.WaitingRegisterIn(mem, len(a["msb"]), over.get("n_keys", len(a["key"])), over.get("n_deps", len(a["dmsb"])),
                             L.TsCols(p("msb"), p("lsb"), p("node")), L.TsCols(p("xmsb"), p("xlsb"), p("xnode")), p("key_off"),
                             p("key"), p("key_wait"), p("dep_off"), L.TsCols(p("dmsb"), p("dlsb"), p("dnode")), p("dep_wait"), tier)
    o = L.WaitingRegisterOut()
    return s.ctx._lib.acc_waiting_register(s.ctx.handle, s.w._h, s.rcmd._h, C.byref(ri), C.byref(o))


def code_of(fn):
    from accord_amd.deps import IllegalArgumentException, IllegalStateException
    try:
        fn()
    except IllegalArgumentException:
        return E_ARG
    except IllegalStateException:
        return E_STATE
    return 0


def test_errors(ctx):
    """every error of the header, then a view equal to the one before them all"""
    import ctypes as C
    steps, ids = WC.literal_steps(True)
    s = Stores(ctx)
    try:
        for st in steps:
            step_device(s, st)
        before = s.w.view()
        P = [tid(100 + 10 * i, READ, 1) for i in range(4)]
        N = tid(7000, READ, 1)
        good = dict(txn=N, x=N, keys=[3, 5], deps=P[:3])

        def reg(mutate=None, mem=0, tier=0, **over):
            w = waiters_of([dict(good), dict(good, txn=tid(7001, READ, 1))])
            if mutate:
                k, i, v = mutate
                w[k] = w[k].copy()
                w[k][i] = v
            return raw_register(s, w, mem, tier, **over)

        got = dict(
            mem=reg(mem=2), tier=reg(tier=3),
            key_off_start=reg(("key_off", 0, 1)), key_off_decreasing=reg(("key_off", 1, 5)), key_off_end=reg(n_keys=3),
            dep_off_start=reg(("dep_off", 0, 1)), dep_off_decreasing=reg(("dep_off", 1, 7)), dep_off_end=reg(n_deps=5),
            keys_unsorted=reg(("key", 1, 3)), deps_unsorted=reg(("dmsb", 1, 100)), key_domain_dep=reg(("dlsb", 0, 0)),
            kind=reg(("lsb", 0, (6 << 1) | 1)), key_wait=reg(("key_wait", 0, 2)), dep_wait=reg(("dep_wait", 0, 2)),
            twice=reg(("msb", 1, 7000)), registered=reg(("msb", 0, 500)))
        want = {k: E_ARG for k in got}
        got.update(cap_keys=reg(n_keys=0xFFFFFFFF), cap_deps=reg(n_deps=0xFFFFFFFF))   # refused before anything is read
        want.update(cap_keys=E_CAP, cap_deps=E_CAP)
        # ACC_E_STATE: a waiter the range-command store holds Applied; an Applied dep whose own record still waits
        s.rcmd.update(rcmd_upd([(N, 8, N), (ids["W"], 8, ids["W"])]))
        got["applied_waiter"] = reg()
        s.rcmd.update(rcmd_upd([(N, 5, N)]))
        got["invariant"] = reg(("dmsb", 2, 500))                          # W (hlc 500) is Applied there and still waits here
        want.update(applied_waiter=E_STATE, invariant=E_STATE)
        s.rcmd.update(rcmd_upd([(ids["W"], 5, ids["W"])]))
        got["changed_unsorted"] = code_of(lambda: s.w.notify(ts_cols([P[1], P[0]]), None))
        got["changed_twice"] = code_of(lambda: s.w.notify(ts_cols([P[1], P[1]]), None))
        got["rel_flags"] = code_of(lambda: s.w.notify(ts_cols([]), WC.releases_of([(ids["W"], 7, 2, WM.ZERO)])))
        ni = L.WaitingNotifyIn(0, 0, L.TsCols(None, None, None), 0, 3, L.TsCols(None, None, None), None, None, L.TsCols(None, None, None))
        no = L.WaitingNotifyOut()
        got["notify_tier"] = ctx._lib.acc_waiting_notify(ctx.handle, s.w._h, s.rcmd._h, C.byref(ni), C.byref(no))
        ni.tier, ni.mem = 0, 7
        got["notify_mem"] = ctx._lib.acc_waiting_notify(ctx.handle, s.w._h, s.rcmd._h, C.byref(ni), C.byref(no))
        got["erase_unsorted"] = code_of(lambda: s.w.erase(ts_cols([P[1], P[0]])))
        want.update(changed_unsorted=E_ARG, changed_twice=E_ARG, rel_flags=E_ARG, notify_tier=E_ARG, notify_mem=E_ARG,
                    erase_unsorted=E_ARG)
        assert got == want
        assert_view(s.w.view(), before, "after every error")
        assert raw_register(s, waiters_of([good])) == 0                   # and the store still works
        assert len(s.w.view()["msb"]) == len(before["msb"]) + 1
    finally:
        s.close()


def test_notify_invariant(ctx):
    """an Applied dep whose own record still waits, met by notify: ACC_E_STATE, nothing changes; once the record has
    stopped waiting the same call goes through"""
    D, X, W = tid(100, READ, 1), tid(50, READ, 1), tid(5000, READ, 1)
    steps = [("rcmd", rcmd_upd([(D, 5, D), (X, 5, X)])),
             ("register", waiters_of([dict(txn=D, x=D, keys=[], deps=[X]), dict(txn=W, x=W, keys=[], deps=[D, X])])),
             ("rcmd", rcmd_upd([(D, 8, D)]))]
    res, store, rcmd = WC.run_model(steps)
    s = Stores(ctx)
    try:
        for st in steps:
            step_device(s, st)
        for tier in TIERS:
            assert code_of(lambda: s.w.notify(ts_cols([D]), None, tier=tier)) == E_STATE
            assert_view(s.w.view(), res[2]["view"], f"after the failed notify, tier {tier}")
        more = [("rcmd", rcmd_upd([(X, 10, X)])), ("notify", ts_cols([X]), None), ("notify", ts_cols([D]), None)]
        res2, _, _ = WC.run_model(more, store, rcmd)
        assert [r["out"]["ready_rec"].tolist() for r in res2[1:]] == [[0], [1]]   # D's record, then W through D
        for st, want in zip(more, res2):
            got = step_device(s, st)
            if st[0] != "rcmd":
                assert_step(ctx, s, st, got, want, "after the record stopped waiting")
    finally:
        s.close()


# ---------------------------------------------------------------- 5. erase

def test_erase(ctx):
    base, pool, ws = WC.edge_case(WC.EDGE_DEPS)
    ids = [w["txn"] for w in ws]
    absent = [tid(4000, READ, 1), tid(9000, READ, 1)]
    steps = list(base[:2]) + [("erase", ts_cols(sorted(ids[2:5] + absent, key=WM.order))), ("erase", ts_cols(absent)),
                              ("erase", ts_cols([])), ("notify", ts_cols(pool[:20]), None),
                              ("erase", ts_cols(sorted(ids, key=WM.order))), ("register", base[1][1]), ("erase", ts_cols(ids[:1]))]
    res, _, _ = WC.run_model(steps)
    assert [r["stats"].get("erased") for r in res if r["name"] == "erase"] == [3, 0, 0, len(ids) - 3, 1]
    assert len(res[6]["view"]["msb"]) == 0
    replay(ctx, steps, res, msg="erase")


# ---------------------------------------------------------------- 6. device inputs

def test_device_inputs(ctx):
    seed = WC.SEEDS[0]
    res, _, _ = WC.chain_model(seed)
    replay(ctx, WC.chain(seed), res, device=True, msg="device inputs")


# ---------------------------------------------------------------- 7. the replica's execution loop

def pairs_of(rel):
    return sorted((t, k, f, u) for t, k, f, u in ((tuple(int(v) for v in t), k, f, tuple(int(v) for v in u))
                                                  for t, k, f, u in WC.release_list(rel)))


@pytest.mark.parametrize("seed", (3, 5))
def test_replica_chain(ctx, seed):
    """preaccept_batch, register_unmanaged, register_waiting and execution_step per batch on one ReplicaStore: the
    release pairs and the ready lists must equal cfk_notify_model and cfk_unmanaged_model composed with waiting_model"""
    import cfk_notify_model as NM
    import cfk_unmanaged_cases as UC
    import cfk_unmanaged_model as UM
    import oracle
    from accord_amd.deps import ReplicaStore
    case = UC.family(seed)
    usteps = UC.run_model(case, oracle.cfk_apply)
    wt, reg, state0 = case["waiters"], usteps[0][4], usteps[0][2]
    RC = [tid(10 + i, READ, 1) for i in range(3)]      # range commands every range-domain waiter depends on
    model, rcmd = WM.Store(), {}
    rs = ReplicaStore(ctx)
    try:
        rp = rcmd_upd([(c, 5, c) for c in RC])
        rs.preaccept_batch(case["base"], scan=False, range_part=rp)
        WM.rcmd_apply(rcmd, rp)
        got = rs.register_unmanaged(wt)
        np.testing.assert_array_equal(got["outcome"], reg["outcome"])
        # the waiters: the unmanaged ones with the bits registerUnmanaged left set, and every CommandsForKey member
        ws, until = [], []
        for i in range(len(wt["msb"])):
            t = (int(wt["msb"][i]), int(wt["lsb"][i]), int(wt["node"][i]))
            k0, k1 = int(wt["key_off"][i]), int(wt["key_off"][i + 1])
            ws.append(dict(txn=t, x=(int(wt["xmsb"][i]), int(wt["xlsb"][i]), int(wt["xnode"][i])),
                           keys=[int(k) for k in wt["key"][k0:k1]], key_wait=[int(o != UM.READY) for o in reg["outcome"][k0:k1]],
                           deps=RC if t[1] & 1 else []))
            until += [(t, int(wt["key"][j]), 0, tuple(reg["until"][j])) for j in range(k0, k1) if reg["outcome"][j] == UM.PENDING_APPLY]
        members = {}
        for k, code in enumerate(state0["key"]):
            for e in range(int(state0["ent_off"][k]), int(state0["ent_off"][k + 1])):
                t = (int(state0["emsb"][e]), int(state0["elsb"][e]), int(state0["enode"][e]))
                if int(state0["status"][e]) != UM.TK and not t[1] & 1:
                    members.setdefault(t, ((int(state0["xmsb"][e]), int(state0["xlsb"][e]), int(state0["xnode"][e])), []))[1].append(int(code))
        ws += [dict(txn=t, x=x, keys=keys, deps=[]) for t, (x, keys) in members.items()]
        W = waiters_of(ws)
        got, want = rs.register_waiting(W), model.register(W, rcmd)
        np.testing.assert_array_equal(got["waiting"], want["waiting"])
        assert until, "a PENDING_APPLY pair hands an until to the caller"
        rel = WC.releases_of(until)
        got, want = rs.notify_waiting(ts_cols([]), rel), model.notify([], WC.release_list(rel), rcmd)
        assert triples(got, "ready_") == [tuple(t) for t in want["ready_txn"]]
        assert_view(rs.waiting.view(), model.view(), "after the registration")
        n_ready = 0
        for b, upd in enumerate(case["later"]):
            state, events = usteps[1 + 2 * b][2], usteps[2 + 2 * b][4]
            rp = rcmd_upd([(c, 8, c) for c in RC]) if b == 1 else None
            rs.preaccept_batch(upd, scan=False, range_part=rp)
            if rp is not None:
                WM.rcmd_apply(rcmd, rp)
            changed = RC if b == 1 else []
            nm = NM.model(state)
            pairs = []
            for r in range(len(nm["key"])):
                for j in range(int(nm["ev_off"][r]), int(nm["ev_off"][r + 1])):
                    if nm["ev_kind"][j] == NM.RELEASE:
                        e = int(nm["ev_entry"][j])
                        pairs.append(((int(state["emsb"][e]), int(state["elsb"][e]), int(state["enode"][e])), int(nm["key"][r]), 1, WM.ZERO))
            pairs += [(t, key, int(kind == UM.EV_RELEASE), u if fl & 1 else WM.ZERO) for kind, fl, key, t, u in events
                      if kind == UM.EV_RELEASE or fl & 1]
            got = rs.execution_step(None, ts_cols(changed))
            assert pairs_of(got["releases"]) == sorted(pairs), f"batch {b}"
            want = model.notify(changed, pairs, rcmd)
            np.testing.assert_array_equal(got["ready_rec"], want["ready_rec"], err_msg=f"batch {b}")
            assert triples(got, "ready_") == [tuple(t) for t in want["ready_txn"]], f"batch {b}"
            assert triples(got, "ready_eal_") == [tuple(t) for t in want["ready_eal"]], f"batch {b}"
            assert got["n_changed"] == want["n_changed"], f"batch {b}"
            assert_view(rs.waiting.view(), model.view(), f"batch {b}")
            n_ready += len(want["ready_rec"])
        assert n_ready > 0 and model.ready_by["key"] > 0 and model.ready_by["both"] + model.ready_by["dep"] > 0, model.ready_by
    finally:
        rs.close()
