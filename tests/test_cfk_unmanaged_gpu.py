"""GPU parity for acc_cfk_register_unmanaged / acc_cfk_notify_unmanaged / acc_cfk_unmanaged_view (CfkStore and
ReplicaStore register_unmanaged, notify_unmanaged, unmanaged).

Expected values come from the literal Python model (cfk_unmanaged_model: pairwise sequential registration into sorted
per-key arrays) over the state the C restatement of the update gives (oracle.cfk_apply; after a prune
cfk_redundant_model.with_redundant_before). Every comparison is exact: outcome / until per pair, state() and the views
after the insertion, the table per key after sorting both by Unmanaged.compareTo, the events as a sorted multiset."""
import functools

import numpy as np
import pytest

import cfk_cases as CC
import cfk_notify_cases as NC
import cfk_notify_model as NM
import cfk_redundant_model as M
import cfk_unmanaged_cases as UC
import cfk_unmanaged_model as UM
import oracle
import test_cfk_query_gpu as QG
import test_cfk_redundant_gpu as RG
from accord_amd import _lib as L

pytestmark = pytest.mark.gpu

TIERS = (0, L.ACC_UNM_TIER_LANE, L.ACC_UNM_TIER_WAVE)
E_ARG, E_STATE = -1, -2


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


def new_store(ctx, upd=None):
    from accord_amd.deps import CfkStore
    s = CfkStore(ctx)
    if upd is not None:
        s.apply_deps(upd)
    return s


def raw_until(g):
    return [(int(a), int(b), int(c)) for a, b, c in zip(g["until_msb"], g["until_lsb"], g["until_node"])]


def assert_register(ctx, s, got, want, st, msg):
    """one register call against the model store st after the same registration"""
    np.testing.assert_array_equal(got["outcome"], want["outcome"], err_msg=msg)
    assert raw_until(got) == [tuple(u) for u in want["until"]], msg
    assert got["n_inserted"] == want["n_inserted"], msg
    assert UM.comparable(UM.device_records(s.unmanaged())) == UM.comparable(st.records()), msg
    stats = ctx.stats()
    oc = want["outcome"]
    assert (stats["cfk.unmanaged_pairs"], stats["cfk.unmanaged_ready"], stats["cfk.unmanaged_pending_commit"],
            stats["cfk.unmanaged_pending_apply"], stats["cfk.unmanaged_tk_inserted"]) == (
        len(oc), int((oc == UM.READY).sum()), int((oc == UM.PENDING_COMMIT).sum()), int((oc == UM.PENDING_APPLY).sum()),
        want["n_inserted"]), msg
    assert stats["cfk.unmanaged_records"] == sum(len(v) for v in st.records().values()), msg


def register_all_tiers(ctx, base_upd, waiters, msg, bounds=None):
    """the same registration on a fresh store per tier; returns the model store"""
    state = oracle.cfk_apply(CC.empty_snapshot(), base_upd) if base_upd is not None else CC.empty_snapshot()
    if bounds is not None:
        state = M.with_redundant_before(state, lambda k: M.NONE, bounds.get)
    st = UM.Store(state, bounds)
    want = st.register(waiters)
    for tier in TIERS:
        s = new_store(ctx, base_upd)
        try:
            if bounds is not None:
                for a, b, t in bounds.updates:
                    s.redundant_before(M.ranges_of([(a - 1, b, t)]))
            got = s.register_unmanaged(waiters, tier=tier)
            assert_register(ctx, s, got, want, st, f"{msg}, tier {tier}")
            if want["n_inserted"] or len(state["key"]):
                RG.assert_store(ctx, s, st.state(), f"{msg}, tier {tier}")
        finally:
            s.close()
    return st, want


# ---------------------------------------------------------------- 1. the chain

@functools.lru_cache(maxsize=None)
def chain(seed):
    case = UC.family(seed)
    return case, UC.run_model(case, oracle.cfk_apply)


@pytest.mark.parametrize("seed", UC.SEEDS)
def test_chain(ctx, seed):
    """register, apply_deps committing, notify_unmanaged, apply_deps applying, notify_unmanaged, redundant_before,
    notify_unmanaged: the table, the state and the events at every step; a second notify_unmanaged emits nothing"""
    case, steps = chain(seed)
    s = new_store(ctx, case["base"])
    try:
        for i, (name, payload, state, records, res) in enumerate(steps):
            msg = f"seed {seed} step {i} {name}"
            if name == "register":
                got = s.register_unmanaged(payload)
                np.testing.assert_array_equal(got["outcome"], res["outcome"], err_msg=msg)
                assert raw_until(got) == [tuple(u) for u in res["until"]], msg
                assert got["n_inserted"] == res["n_inserted"], msg
            elif name == "apply_deps":
                s.apply_deps(payload)
            elif name == "redundant_before":
                s.redundant_before(payload)
            else:
                before = sum(len(v) for v in steps[i - 1][3].values())
                ev = s.notify_unmanaged()
                assert UM.device_events(ev) == res, msg
                assert ev["n_rec"] == sum(len(v) for v in records.values()), msg
                stats = ctx.stats()
                assert stats["cfk.unmanaged_released"] == before - ev["n_rec"], msg
                assert stats["cfk.unmanaged_reevaluated"] == sum(f for _, f, _, _, _ in res), msg
                again = s.notify_unmanaged()
                assert len(again["ev_kind"]) == 0 and again["n_rec"] == ev["n_rec"], msg
            assert UM.comparable(UM.device_records(s.unmanaged())) == records, msg
            RG.assert_store(ctx, s, state, msg)
    finally:
        s.close()


def test_chain_with_key_lists(ctx):
    """key_code=None against explicit lists: the keys in two halves, plus keys without records or a CommandsForKey"""
    case, steps = chain(UC.SEEDS[0])
    s = new_store(ctx, case["base"])
    try:
        s.register_unmanaged(case["waiters"])
        s.apply_deps(case["later"][0])
        want = steps[2][4]
        keys = sorted({k for _, _, k, _, _ in want} | {3, 107, 5000})
        got = []
        for part in (keys[::2], keys[1::2], [], [3]):
            got += UM.device_events(s.notify_unmanaged(np.array(part, np.uint64)))
        assert sorted(got) == want
        assert UM.comparable(UM.device_records(s.unmanaged())) == steps[2][3]
        assert len(s.notify_unmanaged()["ev_kind"]) == 0
    finally:
        s.close()


def test_replica_store(ctx):
    from accord_amd.deps import ReplicaStore
    case, steps = chain(UC.SEEDS[1])
    r = ReplicaStore(ctx)
    try:
        r.cfk.apply_deps(case["base"])
        got = r.register_unmanaged(case["waiters"])
        np.testing.assert_array_equal(got["outcome"], steps[0][4]["outcome"])
        r.cfk.apply_deps(case["later"][0])
        assert UM.device_events(r.notify_unmanaged()) == steps[2][4]
        r.cfk.apply_deps(case["later"][1])
        keys = np.unique(np.asarray(case["waiters"]["key"], np.uint64))
        assert UM.device_events(r.notify_unmanaged(keys)) == steps[4][4]
        assert UM.comparable(UM.device_records(r.cfk.unmanaged())) == steps[4][3]
    finally:
        r.cfk.close()


# ---------------------------------------------------------------- 2. tiers and tiles

DEP_COUNTS = (0, 1, UC.UM_LANE_MAX, UC.UM_LANE_MAX + 1, 63, 64, 65, 1000)


def test_dep_list_lengths_under_every_tier(ctx):
    base, waiters = UC.wide_case(DEP_COUNTS)
    st, want = register_all_tiers(ctx, base, waiters, "wide")
    assert len(set(want["outcome"])) >= 2 and want["n_inserted"] > 100


@pytest.mark.parametrize("n", (NC.SCAN_TILE - 1, NC.SCAN_TILE, NC.SCAN_TILE + 1))
def test_pair_and_missing_counts_at_the_scan_tile(ctx, n):
    """one waiter over n keys of an empty store, one missing dep each: n pairs, n missing pairs, n new keys, n records"""
    tid = UC.ts(4003, UC.EXCLUSIVE_SYNC_POINT, 1, 1)
    waiters = UC.waiters_of([(tid, None, [(1000 + 3 * k, [UC.ts(5 + 4 * (k % 50))]) for k in range(n)])])
    st, want = register_all_tiers(ctx, None, waiters, f"tile {n}")
    assert want["n_inserted"] == n and (want["outcome"] == UM.PENDING_COMMIT).all()


def test_sync_point_over_every_key(ctx):
    """one ExclusiveSyncPoint over every key of a store of 20K keys, deps = each key's entries; then the entries apply"""
    n = 20000
    s_, a_ = NC._Stream(), NC._Stream()
    per_key = []
    for k in range(n):
        code = 10 + 2 * k
        t0, t1 = UC.ts(8 * k + 4), UC.ts(8 * k + 8)
        s_.add(t0, t0, UC.APPLIED if k % 3 else UC.STABLE, [(code, [])])
        s_.add(t1, t1, UC.COMMITTED if k % 2 else UC.PRE, [(code, [t0])])
        a_.add(t0, t0, UC.APPLIED, [(code, [])])
        a_.add(t1, t1, UC.APPLIED, [(code, [t0])])
        per_key.append((code, [t0, t1]))
    base, later = s_.done(), a_.done()
    tid = UC.ts(8 * n + 7, UC.EXCLUSIVE_SYNC_POINT, 1, 1)
    waiters = UC.waiters_of([(tid, None, per_key)])
    state = oracle.cfk_apply(CC.empty_snapshot(), base)
    st = UM.Store(state)
    want = st.register(waiters)
    s = new_store(ctx, base)
    try:
        got = s.register_unmanaged(waiters)
        assert_register(ctx, s, got, want, st, "sync point")
        assert got["n_inserted"] == 0 and set(want["outcome"]) == {UM.PENDING_COMMIT, UM.PENDING_APPLY}
        s.apply_deps(later)
        st.load(oracle.cfk_apply(state, later))
        assert UM.device_events(s.notify_unmanaged()) == sorted(st.notify())
        assert s.unmanaged()["key"].size == 0 and not st.records()
    finally:
        s.close()


def test_same_missing_dep_from_many_waiters(ctx):
    dep, dep2 = UC.ts(401), UC.ts(405)
    items = [(UC.ts(4 * i + 1003, UC.SYNC_POINT, 1 + i % 3, 1), None, [(100, [dep]), (200 + (i % 5), [dep, dep2])]) for i in range(300)]
    base = NC.stream_of([(4, 1, UC.APPLIED, None, 100, [])])
    st, want = register_all_tiers(ctx, base, UC.waiters_of(items), "shared missing")
    assert want["n_inserted"] == 1 + 2 * 5


def test_every_dep_below_the_bound_and_one_equal_to_it(ctx):
    A, B, C, D = (UC.ts(h) for h in (4, 8, 12, 16))
    base = NC.stream_of([(4, 1, UC.APPLIED, None, 500, []), (8, 1, UC.PRE, None, 500, []), (12, 1, UC.PRE, None, 500, []),
                         (16, 1, UC.COMMITTED, None, 500, [])])
    bounds = M.BoundMap(1).add(M.ranges_of([(499, 500, C)]))
    w = UC.waiters_of([(UC.ts(23, UC.SYNC_POINT, 1, 1), None, [(500, [A, B])]),          # all below the bound: READY
                       (UC.ts(27, UC.SYNC_POINT, 1, 1), None, [(500, [A, B, C])]),       # C equals the bound and stays
                       (UC.ts(31, UC.SYNC_POINT, 1, 1), None, [(500, [UC.ts(5), D])])])  # an absent dep below it is not inserted
    st, want = register_all_tiers(ctx, base, w, "bound", bounds)
    assert list(want["outcome"]) == [UM.READY, UM.PENDING_COMMIT, UM.PENDING_APPLY] and want["n_inserted"] == 0


# ---------------------------------------------------------------- 3. the adopted view

def test_queries_after_an_insertion(ctx):
    """acc_cfk_keydeps, acc_cfk_notify and acc_cfk_map_reduce_full on the store after an insertion against the host
    restatements over the model's state"""
    import test_cfk_recovery_gpu as RV
    case, steps = chain(UC.SEEDS[2])
    state = steps[0][2]
    s = new_store(ctx, case["base"])
    try:
        s.register_unmanaged(case["waiters"])
        RG.assert_store(ctx, s, state, "after the insertion")
        ob, mo, mt = CC.snap_as_batch(state)
        QG.assert_result(s.keydeps(QG.member_queries(ob)), oracle.keydeps_batch(ob), "keydeps")
        want = NM.model(state)
        got = s.notify()
        for f in NM.FIELDS + NM.VIEW_FIELDS:
            np.testing.assert_array_equal(got[f], want[f], err_msg=f"notify {f}")
        q = CC.recovery_queries(ob, 7, 60)
        for sa, td, ts_ in ((L.ACC_STARTED_BEFORE, L.ACC_DEP_WITHOUT, L.ACC_STATUS_IS_PROPOSED),
                            (L.ACC_STARTED_ANY, L.ACC_DEP_WITH, L.ACC_STATUS_ANY)):
            o = oracle.map_reduce_full(ob, mo, mt, q, sa, td, ts_)
            g = s.map_reduce_full(q, sa, td, ts_)
            RV.assert_same(g, o, f"map_reduce_full {sa} {td} {ts_}", ("arena_off", "arena", "kd_off", "key_idx", "u_off", "dep_txn"))
    finally:
        s.close()


# ---------------------------------------------------------------- 4. errors leave everything as it was

def _snapshot(s):
    snap = s.snapshot()
    t = s.unmanaged()
    return s.state(), [np.asarray(getattr(snap, f)) for f in RG.BATCH_FIELDS], t


def _same(a, b):
    for x, y in zip((a[0], dict(enumerate(a[1])), a[2]), (b[0], dict(enumerate(b[1])), b[2])):
        assert x.keys() == y.keys()
        for k in x:
            np.testing.assert_array_equal(x[k], y[k], err_msg=str(k))


def test_errors_leave_store_and_table_unchanged(ctx):
    from accord_amd.deps import AccordError
    case, _ = chain(UC.SEEDS[0])
    s = new_store(ctx, case["base"])
    try:
        s.register_unmanaged(case["waiters"])
        before = _snapshot(s)
        A, B = UC.ts(4), UC.ts(8)
        sp = lambda h: UC.ts(h, UC.SYNC_POINT, 1, 1)  # noqa: E731
        good = UC.waiters_of([(sp(90003), None, [(100, [A, B]), (110, [A])]), (sp(90007), None, [(100, [A])])])

        def bad(**kw):
            w = {k: np.array(v, copy=True) for k, v in good.items()}
            for k, v in kw.items():
                w[k] = np.asarray(v, w[k].dtype)
            return w
        lsb = lambda kind, dom: UC.ts(90003, kind, 1, dom)[1]  # noqa: E731
        cases = [("key_off start", bad(key_off=[1, 2, 3])), ("key_off decreasing", bad(key_off=[0, 3, 2])),
                 ("key_off end", bad(key_off=[0, 2, 2])), ("dep_off start", bad(dep_off=[1, 2, 3, 4])),
                 ("dep_off decreasing", bad(dep_off=[0, 3, 2, 4])), ("dep_off end", bad(dep_off=[0, 2, 3, 3])),
                 ("keys unsorted", bad(key=[110, 100, 100])), ("keys duplicate", bad(key=[100, 100, 100])),
                 ("deps unsorted", bad(dmsb=good["dmsb"][[1, 0, 2, 3]], dlsb=good["dlsb"][[1, 0, 2, 3]])),
                 ("deps duplicate", bad(dlsb=good["dlsb"][[0, 0, 2, 3]])),
                 ("kind 6", bad(lsb=[lsb(6, 1), good["lsb"][1]])), ("kind 7", bad(lsb=[lsb(7, 0), good["lsb"][1]])),
                 ("managed write", bad(lsb=[lsb(UC.WRITE, 0), good["lsb"][1]])),
                 ("managed sync point", bad(lsb=[lsb(UC.SYNC_POINT, 0), good["lsb"][1]])),
                 ("waiter twice", bad(lsb=[good["lsb"][0], good["lsb"][0]]))]
        for name, w in cases:
            with pytest.raises(AccordError) as e:
                s.register_unmanaged(w)
            assert e.value.code == E_ARG, name
            _same(_snapshot(s), before)
        with pytest.raises(AccordError) as e:
            s.register_unmanaged(good, tier=3)
        assert e.value.code == E_ARG
        for keys in ([110, 100], [100, 100]):
            with pytest.raises(AccordError) as e:
                s.notify_unmanaged(np.array(keys, np.uint64))
            assert e.value.code == E_ARG
        _same(_snapshot(s), before)
        # mem, through the C ABI (the Python entry points always pass ACC_MEM_HOST)
        import ctypes as C
        p = lambda k: good[k].ctypes.data  # noqa: E731
        ui = L.CfkUnmanagedIn(7, len(good["msb"]), len(good["key"]), len(good["dmsb"]), L.TsCols(p("msb"), p("lsb"), p("node")),
                              L.TsCols(p("xmsb"), p("xlsb"), p("xnode")), p("key_off"), p("key"), p("dep_off"),
                              L.TsCols(p("dmsb"), p("dlsb"), p("dnode")), 0)
        assert ctx._lib.acc_cfk_register_unmanaged(ctx.handle, s._h, C.byref(ui), C.byref(L.CfkUnmanagedOut())) == E_ARG
        kc = np.array([100], np.uint64)
        ni = L.CfkUnmanagedNotifyIn(7, 1, kc.ctypes.data)
        assert ctx._lib.acc_cfk_notify_unmanaged(ctx.handle, s._h, C.byref(ni), C.byref(L.CfkUnmanagedEvents())) == E_ARG
        _same(_snapshot(s), before)
        # LocalOnly and key-domain EphemeralRead waiters are unmanaged; no waiters is a no-op
        ok = s.register_unmanaged(bad(lsb=[lsb(UC.LOCAL_ONLY, 0), lsb(UC.EPHEMERAL_READ, 0) + (4 << 16)]))
        assert len(ok["outcome"]) == 3
        empty = {k: v[:0] for k, v in good.items()}
        empty.update(key_off=np.zeros(1, np.uint32), dep_off=np.zeros(1, np.uint32))
        after = _snapshot(s)
        assert len(s.register_unmanaged(empty)["outcome"]) == 0
        _same(_snapshot(s), after)
    finally:
        s.close()


def test_state_errors(ctx):
    from accord_amd import workload as W
    from accord_amd.deps import AccordError
    sp = UC.ts(90003, UC.SYNC_POINT, 1, 1)
    w = UC.waiters_of([(sp, None, [(100, [UC.ts(4)])])])
    s = new_store(ctx)
    try:   # a non-empty status-only store
        s.update(W.keydeps_batch(20, 2, 10, 3, "uniform", 0.0))
        for call in (lambda: s.register_unmanaged(w), lambda: s.notify_unmanaged()):
            with pytest.raises(AccordError) as e:
                call()
            assert e.value.code == E_STATE
        assert s.unmanaged()["key"].size == 0
    finally:
        s.close()
    # acc_cfk_notify's illegal kind, inherited: an EphemeralRead entry on an asked key (test_cfk_notify_gpu.test_illegal_kind)
    upd = NC.stream_of([(8, NM.WRITE, NC.STABLE, None, 500, [(4, NM.EPHEMERAL_READ)]), (12, NM.WRITE, NC.STABLE, None, 510, [])])
    s = new_store(ctx, upd)
    try:
        w2 = UC.waiters_of([(sp, None, [(500, [UC.ts(8)]), (510, [UC.ts(12)])])])
        assert list(s.register_unmanaged(w2)["outcome"]) == [UM.PENDING_APPLY] * 2
        before = _snapshot(s)
        for keys in (None, np.array([500], np.uint64)):
            with pytest.raises(AccordError) as e:
                s.notify_unmanaged(keys)
            assert e.value.code == E_STATE
        _same(_snapshot(s), before)
        assert len(s.notify_unmanaged(np.array([510], np.uint64))["ev_kind"]) == 0
    finally:
        s.close()
