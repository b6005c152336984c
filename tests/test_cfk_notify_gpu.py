"""GPU parity for acc_cfk_notify (CfkStore.notify, ReplicaStore.notify, preaccept_batch(notify=True)): the execution
releases of CommandsForKey.notify (local/CommandsForKey.java:1501-1635) read from the resident store.

Expected values come from the literal Python model (cfk_notify_model.model) over the state the C restatement of the update
gives (oracle.cfk_apply; after a prune cfk_redundant_model.with_redundant_before). Every comparison is exact array
equality. The seeds and shapes meet their host conditions in test_cfk_notify_model.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import cfk_cases as CC
import cfk_notify_cases as NC
import cfk_notify_model as NM
import cfk_redundant_model as M
import oracle
import test_cfk_redundant_gpu as RG

pytestmark = pytest.mark.gpu

FIELDS = NM.FIELDS + NM.VIEW_FIELDS
TIERS = (0, 1, 2, 3)     # the default, ACC_NOTIFY_TIER_LANE, _WAVE, _SORT


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


def assert_notify(got, want, msg):
    for f in FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{msg}: {f}")


def check(c, s, state, msg, keys=None, tiers=(0,)):
    want = NM.model(state, keys)
    for tier in tiers:
        assert_notify(s.notify(keys, tier=tier), want, f"{msg}, tier {tier}")
    st = c.stats()
    assert st["cfk.notify_keys"] == len(want["key"]), msg
    assert st["cfk.notify_releases"] == int((want["ev_kind"] == NM.RELEASE).sum()), msg
    return want


# ---------------------------------------------------------------- 1. hand-worked

def test_literal_abcd(ctx):
    from accord_amd.deps import CfkStore
    s = CfkStore(ctx)
    try:
        state = CC.empty_snapshot()
        for upd, want_state, rows in NC.literal_abcd():
            state = oracle.cfk_apply(state, upd)
            s.apply_deps(upd)
            RG.assert_store(ctx, s, want_state, "literal")
            for tier in TIERS:
                assert NC.rows_as_hlc(want_state, s.notify(tier=tier)) == rows
            check(ctx, s, state, "literal", tiers=TIERS)
        np.testing.assert_array_equal(s.notify()["rel_keys"], [0, 0, 0, 1])
    finally:
        s.close()


def test_literal_kinds(ctx):
    from accord_amd.deps import CfkStore
    for upd, want_state, rows in NC.literal_kinds():
        s = CfkStore(ctx)
        try:
            s.apply_deps(upd)
            RG.assert_store(ctx, s, want_state, "kinds")
            for tier in TIERS:
                assert NC.rows_as_hlc(want_state, s.notify(tier=tier)) == rows
        finally:
            s.close()


# ---------------------------------------------------------------- 2. chained batches

@functools.lru_cache(maxsize=None)
def chain(seed):
    """[(batch, state after it, the model's rows for every key)] of frontier_case(seed)"""
    state, out = CC.empty_snapshot(), []
    for part in NC.batches(NC.frontier_case(seed)):
        state = oracle.cfk_apply(state, part)
        m = NM.model(state)
        NC.conditions(state, m)
        out.append((part, state, m))
    return out


@pytest.mark.parametrize("seed", NC.SEEDS)
def test_chained_batches(ctx, seed):
    from accord_amd.deps import CfkStore
    s = CfkStore(ctx)
    try:
        for b, (part, state, want) in enumerate(chain(seed)):
            msg = f"seed {seed} batch {b}"
            s.apply_deps(part)
            got = s.notify()
            assert_notify(got, want, msg)
            # rel_keys = per txn the keys that release it
            vi, n = NM.view_index(state)
            rel = np.bincount(vi[want["ev_entry"][want["ev_kind"] == NM.RELEASE].astype(np.int64)], minlength=n)
            np.testing.assert_array_equal(got["rel_keys"], rel, err_msg=msg)
            assert ctx.stats()["cfk.notify_candidates"] == int(((state["status"] == 4) | (state["status"] == 5)).sum())
            codes = state["key"]
            subset = np.unique(np.concatenate([codes[::3], codes[-1:], np.array([1, 105, 99999], np.uint64)]))
            check(ctx, s, state, msg + " subset", subset)
            check(ctx, s, state, msg + " absent only", np.array([3, 7], np.uint64))
            got = check(ctx, s, state, msg + " no keys", np.zeros(0, np.uint64))
            assert len(got["ev_off"]) == 1 and not got["rel_keys"].any()
            if b == len(chain(seed)) - 1:
                check(ctx, s, state, msg, tiers=TIERS[1:])
        RG.assert_store(ctx, s, state, "notify modified the store")
    finally:
        s.close()


# ---------------------------------------------------------------- 3. tier edges

# (entries, bumped, live) per key. Segment lengths 1, 63, 64, 65, 255, 256, 257; bumped counts on both sides of
# NT_LANE_MAX, NT_LANE_FORCE_MAX and NT_WAVE_MAX; live (candidate) counts 0, 1, 64, 65 and 1100, past the wave tier;
# a hot key of 5,000 entries with 1,500 candidates, ranked by the sort tier; 16K entries in all, past one SCAN_TILE.
EDGE_SHAPES = [(1, 0, 1), (1, 1, 1), (63, 1, 5), (64, NC.NT_LANE_MAX, 20), (65, NC.NT_LANE_MAX + 1, 64),
               (255, NC.NT_LANE_FORCE_MAX, 65), (256, NC.NT_LANE_FORCE_MAX + 1, 0), (257, 100, 1),
               (1300, NC.NT_WAVE_MAX, 64), (1300, NC.NT_WAVE_MAX + 1, 65), (2400, 1100, 1100), (5000, 2500, 1500),
               (300, 40, 30), (NC.SCAN_TILE - 2960, 700, 40)]


@functools.lru_cache(maxsize=None)
def edge_case():
    upd = NC.segments_case(11, EDGE_SHAPES)
    state = oracle.cfk_apply(CC.empty_snapshot(), upd)
    assert len(state["status"]) == sum(n for n, _, _ in EDGE_SHAPES) > 2 * NC.SCAN_TILE - 1
    return upd, state, NM.model(state)


def test_tier_edges(ctx):
    from accord_amd.deps import CfkStore
    upd, state, want = edge_case()
    assert int((want["ev_kind"] == NM.RELEASE).sum()) > 0 and len(want["held"]) > 0
    s = CfkStore(ctx)
    try:
        s.apply_deps(upd)
        for f in RG.STATE_FIELDS:
            np.testing.assert_array_equal(s.state()[f], state[f], err_msg=f)
        sorted_by = {}
        for tier in TIERS:
            assert_notify(s.notify(tier=tier), want, f"tier {tier}")
            sorted_by[tier] = ctx.stats()["cfk.notify_sorted"]
        big = lambda cap: sum(nb for _, nb, _ in EDGE_SHAPES if nb > cap)  # noqa: E731
        assert sorted_by == {0: big(NC.NT_WAVE_MAX), 1: big(NC.NT_LANE_FORCE_MAX), 2: big(NC.NT_WAVE_MAX), 3: big(0)}
        # single keys and a few keys: the asked entry space starts inside the store's
        codes = state["key"]
        for keys in (codes[4:5], codes[9:10], codes[11:12], codes[[0, 5, 9, 12]], codes[[3, 10]]):
            want_k = NM.model(state, keys)
            for tier in TIERS:
                assert_notify(s.notify(keys, tier=tier), want_k, f"keys {keys} tier {tier}")
    finally:
        s.close()


@pytest.mark.parametrize("shape", EDGE_SHAPES[:10], ids=lambda sh: "x".join(map(str, sh)))
def test_single_key_stores(ctx, shape):
    from accord_amd.deps import CfkStore
    upd = NC.segments_case(5, [shape])
    state = oracle.cfk_apply(CC.empty_snapshot(), upd)
    s = CfkStore(ctx)
    try:
        s.apply_deps(upd)
        check(ctx, s, state, f"shape {shape}", tiers=TIERS)
    finally:
        s.close()


# ---------------------------------------------------------------- 4. pruning

def test_after_redundant_before(ctx):
    from accord_amd.deps import CfkStore
    seed = NC.SEEDS[0]
    parts = [p for p, _, _ in chain(seed)]
    s = CfkStore(ctx)
    try:
        m = M.BoundMap(1)
        state = CC.empty_snapshot()
        dropped = 0
        for b, part in enumerate(parts):
            state = RG.apply(ctx, s, state, m, part, f"batch {b}")
            check(ctx, s, state, f"batch {b}", tiers=TIERS)
            if b in (1, 3):
                # a bound a little below the frontier: between two TxnIds, so APPLIED prefixes go and live entries lose
                # missing ids; the second prune has three bounds
                j = 300 * 9 // 10 * (b + 1) // 5 // 3
                ranges = M.ranges_of([(M.KEY_LO, M.KEY_HI, M.ts(4 * j + 2))] if b == 1 else
                                     [(M.KEY_LO, 130, M.ts(4 * j + 2)), (130, 170, M.ts(4 * j + 42)), (170, M.KEY_HI, M.ts(4 * j - 38))])
                before = len(state["status"])
                state = RG.prune(ctx, s, state, m, ranges, f"prune after batch {b}")
                dropped += before - len(state["status"])
                check(ctx, s, state, f"pruned after batch {b}", tiers=TIERS)
        assert dropped > 50
    finally:
        s.close()


# ---------------------------------------------------------------- 5. errors and empties

def test_errors_and_empties(ctx):
    from accord_amd import _lib as L
    from accord_amd.deps import CfkStore, IllegalArgumentException, IllegalStateException
    from accord_amd import workload as W
    part, state, want = chain(NC.SEEDS[1])[0]
    s = CfkStore(ctx)
    try:
        # an empty store
        got = s.notify()
        assert len(got["key"]) == 0 and list(got["ev_off"]) == [0] and len(got["rel_keys"]) == 0
        got = s.notify(np.array([100, 110], np.uint64))
        assert list(got["min_uncommitted"]) == [NM.NONE] * 2 and list(got["ev_off"]) == [0, 0, 0]
        got = s.notify(np.zeros(0, np.uint64))
        assert list(got["ev_off"]) == [0]
        s.apply_deps(part)
        codes = state["key"]
        bad_mem = L.CfkNotifyIn(7, 0, None, 0)
        view = L.CfkNotifyView()
        for call in (lambda: s.notify(codes[[2, 1]]), lambda: s.notify(codes[[1, 1]]), lambda: s.notify(codes[[0, 3, 3, 5]]),
                     lambda: s.notify(tier=4), lambda: s.notify(codes[:2], tier=77),
                     lambda: ctx.check(ctx._lib.acc_cfk_notify(ctx.handle, s._h, C.byref(bad_mem), C.byref(view)))):
            with pytest.raises(IllegalArgumentException):
                call()
            RG.assert_store(ctx, s, state, "after a failed call")
            assert_notify(s.notify(), want, "after a failed call")
    finally:
        s.close()
    # a status-only store (acc_cfk_update)
    s = CfkStore(ctx)
    try:
        b = W.keydeps_batch(50, 2, 10, 7, "uniform")
        s.update(b)
        with pytest.raises(IllegalStateException):
            s.notify()
        with pytest.raises(IllegalStateException):
            s.notify(np.array([100], np.uint64))
        np.testing.assert_array_equal(s.snapshot().key_code, b.key_code)
    finally:
        s.close()


# ---------------------------------------------------------------- 6. the replica store

def test_replica_store(ctx):
    from accord_amd.deps import ReplicaStore
    seed = NC.SEEDS[2]
    r = ReplicaStore(ctx)
    try:
        for b, (part, state, want) in enumerate(chain(seed)):
            out = r.preaccept_batch(part, scan=False, notify=True)
            touched = np.unique(part["key"])
            np.testing.assert_array_equal(out["notify"]["key"], touched)
            assert_notify(out["notify"], r.cfk.notify(touched), f"batch {b}: preaccept_batch against CfkStore.notify")
            assert_notify(out["notify"], NM.model(state, touched), f"batch {b}: touched keys")
            assert_notify(r.notify(), want, f"batch {b}: every key")
            some = state["key"][1::4]
            assert_notify(r.notify(some), r.cfk.notify(some), f"batch {b}: some keys")
    finally:
        r.close()


# ---------------------------------------------------------------- 7. keys in device memory; two stores on one context

def test_device_keys_and_two_stores(ctx):
    """acc_cfk_notify through the C ABI with key_code in HBM (what a shim passes), the caller's array left as it was; and
    two stores of different sizes asked in turn on one context: each call's view is its own store's"""
    import torch
    from accord_amd import _lib as L
    from accord_amd.deps import CfkStore, device_array
    small_want = chain(NC.SEEDS[0])[0][2]
    upd, state, want = edge_case()
    a, b = CfkStore(ctx), CfkStore(ctx)
    try:
        a.apply_deps(upd)
        b.apply_deps(chain(NC.SEEDS[0])[0][0])
        keys = np.ascontiguousarray(state["key"][[1, 4, 9, 11, 13]])
        t = torch.from_numpy(keys.view(np.int64)).to(torch.device("cuda", ctx.device))
        torch.cuda.synchronize()
        for tier in TIERS:
            ni = L.CfkNotifyIn(L.ACC_MEM_DEVICE, len(keys), t.data_ptr(), tier)
            v = L.CfkNotifyView()
            ctx.check(ctx._lib.acc_cfk_notify(ctx.handle, a._h, C.byref(ni), C.byref(v)))
            w = NM.model(state, keys)
            assert (int(v.n_keys), int(v.n_events), int(v.n_txn)) == (len(keys), len(w["ev_entry"]), len(w["rel_keys"]))
            for f, dt in (("ev_entry", np.uint32), ("ev_txn", np.uint32), ("ev_pos", np.uint32), ("ev_kind", np.uint8)):
                np.testing.assert_array_equal(device_array(ctx, getattr(v, f), len(w[f]), dt), w[f], err_msg=f"tier {tier} {f}")
            np.testing.assert_array_equal(device_array(ctx, v.ev_off, len(keys) + 1, np.uint64), w["ev_off"])
            np.testing.assert_array_equal(device_array(ctx, v.next, len(keys), np.uint32), w["next"])
            np.testing.assert_array_equal(t.cpu().numpy().view(np.uint64), keys)
            assert_notify(b.notify(tier=tier), small_want, f"the small store after the large one, tier {tier}")
            assert_notify(a.notify(tier=tier), want, f"the large store after the small one, tier {tier}")
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 8. the reference's illegalState

def test_illegal_kind(ctx):
    """a STABLE Write whose deps name an EphemeralRead id: CommandsForKey.update adds the id as TRANSITIVELY_KNOWN, and
    notify's backfill meets it (:1553-1555, illegalState). Asking only other keys is no error."""
    from accord_amd.deps import CfkStore, IllegalStateException
    upd = NC.stream_of([(8, NM.WRITE, NC.STABLE, None, 500, [(4, NM.EPHEMERAL_READ)]), (12, NM.WRITE, NC.STABLE, None, 510, [])])
    state = oracle.cfk_apply(CC.empty_snapshot(), upd)
    assert [int(x) for x in state["status"]] == [NC.TK, NC.STABLE, NC.STABLE]
    with pytest.raises(NM.IllegalState):
        NM.model(state)
    s = CfkStore(ctx)
    try:
        s.apply_deps(upd)
        for f in RG.STATE_FIELDS:
            np.testing.assert_array_equal(s.state()[f], state[f], err_msg=f)
        for keys in (None, np.array([500], np.uint64), np.array([500, 510], np.uint64)):
            with pytest.raises(IllegalStateException):
                s.notify(keys)
        check(ctx, s, state, "the other key", np.array([510, 520], np.uint64), tiers=TIERS)
        for f in RG.STATE_FIELDS:
            np.testing.assert_array_equal(s.state()[f], state[f], err_msg=f)
    finally:
        s.close()
