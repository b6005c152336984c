"""GPU parity for acc_cfk_redundant_before (CfkStore.redundant_before / redundant_map): the resident CommandsForKey store
pruned by a RedundantBefore map (CommandsForKey.withRedundantBefore, local/CommandsForKey.java:1654-1684) and
acc_cfk_apply_deps ignoring the deps below a key's bound (:1088-1089).

Expected values come from the Python model (cfk_redundant_model.py) alternating with the C restatement of the update
(oracle.cfk_apply over the model's trimmed deps); the two views are cfk_cases.snap_as_batch of the model state. Every
comparison is exact array equality. The seeds were chosen on the host model alone (see host_conditions)."""
import functools

import numpy as np
import pytest

import cfk_cases as CC
import cfk_redundant_model as M
import oracle
import recovery_cases as RC
import test_cfk_query_gpu as KQ
import test_cfk_query_mixed_gpu as MX
import test_cfk_recovery_gpu as CR

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("key", "ent_off", "emsb", "elsb", "enode", "xmsb", "xlsb", "xnode", "status", "miss_off", "mmsb", "mlsb", "mnode")
BATCH_FIELDS = ("txn_msb", "txn_lsb", "txn_node", "exe_msb", "exe_lsb", "exe_node", "status", "key_off", "key_code")
STATS = ("cfk.redundant_keys_advanced", "cfk.redundant_entries_dropped", "cfk.redundant_missing_dropped")
RB_VEC = 4       # csrc/cfkredundant.hip: destination elements one lane of the segmented copy moves (a wave: 256)
SEEDS = (5, 7)   # cfk_case seeds whose chained cases meet host_conditions under both variants


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_hot4():
    from accord_amd.deps import Context
    c = Context(0, cfk_hot=4)
    yield c
    c.close()


def assert_store(c, s, state, msg):
    """state(), snapshot() and missing_view() of the store against the model state"""
    from accord_amd.deps import cfk_batch_host
    g = s.state()
    for f in STATE_FIELDS:
        np.testing.assert_array_equal(g[f], state[f], err_msg=f"{msg}: state {f}")
    b, mo, mt = CC.snap_as_batch(state)
    snap = s.snapshot()
    gb, gmo, gmt = cfk_batch_host(c, s.missing_view())
    for f in BATCH_FIELDS:
        np.testing.assert_array_equal(getattr(snap, f), getattr(b, f), err_msg=f"{msg}: view {f}")
        np.testing.assert_array_equal(getattr(gb, f), getattr(b, f), err_msg=f"{msg}: missing view {f}")
    np.testing.assert_array_equal(gmo, mo, err_msg=f"{msg}: missing_off")
    np.testing.assert_array_equal(gmt, mt, err_msg=f"{msg}: missing_txn")


def assert_stats(c, counts, msg):
    st = c.stats()
    assert {k: st[k] for k in STATS} == {
        "cfk.redundant_keys_advanced": counts["keys_advanced"], "cfk.redundant_entries_dropped": counts["entries_dropped"],
        "cfk.redundant_missing_dropped": counts["missing_dropped"]}, msg


def assert_map(s, m, msg):
    g = s.redundant_map()
    want = m.intervals()
    assert g["end_inclusive"] == m.end_inclusive, msg
    np.testing.assert_array_equal(g["st"], np.array([a for a, _, _ in want], np.uint64), err_msg=msg)
    np.testing.assert_array_equal(g["en"], np.array([b for _, b, _ in want], np.uint64), err_msg=msg)
    assert [M.order(t) for t in zip(g["msb"], g["lsb"], g["node"])] == [v for _, _, v in want], msg


def prune(c, s, state, m, ranges, msg):
    """one redundant_before on store and model; returns the model state after it"""
    old = m.copy()
    m.add(ranges)
    counts = {}
    state = M.with_redundant_before(state, old.get, m.get, counts)
    s.redundant_before(ranges, m.end_inclusive)
    assert_stats(c, counts, msg)
    assert_store(c, s, state, msg)
    assert_map(s, m, msg)
    return state


def apply(c, s, state, m, upd, msg):
    trimmed, n = M.trim_deps(upd, m.get)
    state = oracle.cfk_apply(state, trimmed)
    s.apply_deps(upd)
    assert c.stats()["cfk.deps_trimmed"] == n, msg
    assert_store(c, s, state, msg)
    return state


# ---------------------------------------------------------------- 1. hand-worked

def test_handmade(ctx):
    from accord_amd.deps import CfkStore
    upd, ranges, before, after = M.handmade()
    s = CfkStore(ctx)
    try:
        m = M.BoundMap(1)
        state = apply(ctx, s, CC.empty_snapshot(), m, upd, "handmade stream")
        assert M.describe(state) == before
        state = prune(ctx, s, state, m, ranges, "handmade prune")
        assert M.describe(state) == after
        assert M.describe(s.state()) == after
    finally:
        s.close()


# ---------------------------------------------------------------- 2. range bound types

@pytest.mark.parametrize("end_inclusive", [1, 0], ids=["end_inclusive", "start_inclusive"])
def test_range_bound_types(ctx, end_inclusive):
    """keys 100 .. 400 and the range 100 .. 300: (100, 300] holds 200 and 300, [100, 300) holds 100 and 200; a bound
    above every TxnId removes exactly the covered keys"""
    from accord_amd.deps import CfkStore
    upd, _, _, _ = M.handmade()
    s = CfkStore(ctx)
    try:
        m = M.BoundMap(end_inclusive)
        state = apply(ctx, s, CC.empty_snapshot(), m, upd, "stream")
        state = prune(ctx, s, state, m, M.ranges_of([(100, 300, M.ts(30))]), f"end_inclusive {end_inclusive}")
        assert [int(k) for k in s.state()["key"]] == ([100, 400] if end_inclusive else [300, 400])
    finally:
        s.close()


# ---------------------------------------------------------------- 3. pointwise max and the equals path

def test_pointwise_max_and_unchanged_bounds(ctx):
    from accord_amd.deps import CfkStore
    upd, _, _, _ = M.handmade()
    everything = lambda t: M.ranges_of([(M.KEY_LO, M.KEY_HI, t)])  # noqa: E731
    s = CfkStore(ctx)
    try:
        m = M.BoundMap(1)
        state = apply(ctx, s, CC.empty_snapshot(), m, upd, "stream")
        state = prune(ctx, s, state, m, everything(M.ts(10)), "bound 10")       # A, B leave every key
        assert len(state["status"]) == 12
        view = s.view()
        ptrs = (view.txn_id.msb, view.key_off, view.key_code)
        state = prune(ctx, s, state, m, everything(M.ts(6)), "a lower bound")   # absorbed by the max
        assert ctx.stats()["cfk.redundant_keys_advanced"] == 0
        view = s.view()
        assert (view.txn_id.msb, view.key_off, view.key_code) == ptrs, "the fast path rewrote the view"
        # an update below the unchanged bound is inserted, and stays through a repeated call with that bound
        low = M.updates_of([(M.ts(6), M.PRE, [100], [])])
        state = apply(ctx, s, state, m, low, "insert below the bound")
        assert M.describe(state)[100][0] == (6, M.PRE, [])
        state = prune(ctx, s, state, m, everything(M.ts(10)), "the same bound again")
        assert ctx.stats()["cfk.redundant_keys_advanced"] == 0
        assert M.describe(s.state())[100][0] == (6, M.PRE, [])
        state = prune(ctx, s, state, m, everything(M.ts(11)), "a higher bound")
        assert ctx.stats()["cfk.redundant_keys_advanced"] == 4
        assert M.describe(s.state())[100][0][0] == 12
    finally:
        s.close()


# ---------------------------------------------------------------- 4. segment and list sizes

# entries per key: the lanes of a wave and the 256 destination elements a wave of the segmented copy moves, +-1; 1025: more
# than one block of it; 2 .. 5 and 66, 301: around RB_VEC, and top entries whose missing[] holds 1, 63, 64, 65 and 300 ids
LENS = [1, 2, 3, RB_VEC, RB_VEC + 1, 63, 64, 65, 66, 255, 256, 257, 301, 1025]
CUTS = ["0", "1", "2", "3", "4", "63", "64", "65", "mid", "len-1", "len"]


def size_code(i):
    return 1000 + 10 * i


@functools.lru_cache(maxsize=None)
def size_case():
    """key i holds LENS[i] Writes on hlc 4, 8, .. (its own node id: a TxnId lives on one key): all PREACCEPTED but the last, which is ACCEPTED without deps, so its
    missing[] names every entry below it (0, 1, .., 1024 ids); the reference state, computed once"""
    steps = []
    for i, n in enumerate(LENS):
        steps += [(M.ts(4 * j + 4, node=i + 1), M.PRE if j + 1 < n else M.ACC, [size_code(i)], []) for j in range(n)]
    upd = M.updates_of(steps)
    state = oracle.cfk_apply(CC.empty_snapshot(), upd)
    top = state["ent_off"][1:].astype(np.int64) - 1
    assert [int(x) for x in np.diff(state["miss_off"].astype(np.int64))[top]] == [n - 1 for n in LENS]
    return upd, state


def cut_of(kind, n):
    c = {"mid": n // 2, "len-1": n - 1, "len": n}.get(kind)
    return min(int(kind), n) if c is None else c


@pytest.mark.parametrize("kind", CUTS)
def test_segment_and_list_sizes(ctx, kind):
    """every key cut at `kind` (clipped to its length): the bound lies between entry cut - 1 and entry cut, so `cut`
    entries go and the top entry's missing[] loses `cut` ids: none, one, 63 / 64 / 65, half, all but one, all (the key
    keeps its top entry alone, missing[] emptied) and, at len, the key itself"""
    from accord_amd.deps import CfkStore
    upd, state = size_case()
    ranges = M.ranges_of([(size_code(i) - 1, size_code(i), M.ts(4 * cut_of(kind, n) + 2)) for i, n in enumerate(LENS)])
    s = CfkStore(ctx)
    try:
        s.apply_deps(upd)
        m = M.BoundMap(1)
        after = prune(ctx, s, state, m, ranges, f"cut {kind}")
        want = {size_code(i): n - cut_of(kind, n) for i, n in enumerate(LENS) if n > cut_of(kind, n)}
        assert {int(k): int(c) for k, c in zip(after["key"], np.diff(after["ent_off"].astype(np.int64)))} == want
    finally:
        s.close()


# ---------------------------------------------------------------- 5. + 6. chained batches and prunes

@functools.lru_cache(maxsize=None)
def chain(seed, variant):
    upd = CC.cfk_case(seed, n_txn=300, n_keys=12, p_accinv=0)
    return M.chained_case(upd, variant, oracle.cfk_apply)


def lacking_trimmed_deps(steps):
    """(key, dep compare key) of deps that a bound removed from an update while the key held no such entry"""
    out, m = [], M.BoundMap(1)
    for s in steps:
        if s["op"] == "prune":
            m = s["map"]
            continue
        u, st = s["upd"], s["state"]
        held = {int(k): {M.order((st["emsb"][e], st["elsb"][e], st["enode"][e]))
                         for e in range(int(st["ent_off"][i]), int(st["ent_off"][i + 1]))} for i, k in enumerate(st["key"])}
        for j, code in enumerate(u["key"]):
            for i in range(int(u["dep_off"][j]), int(u["dep_off"][j + 1])):
                d = M.order((u["dmsb"][i], u["dlsb"][i], u["dnode"][i]))
                if d < M.order(m.get(int(code))) and d not in held.get(int(code), set()):
                    out.append((int(code), d))
    return out


def host_conditions(steps, variant):
    """what a seed must give, checked on the model alone, before the device is asked"""
    for st in steps:
        CC.snap_as_batch(st["state"])            # asserts one status and executeAt per TxnId across its keys
    assert KQ.no_committed_ties(steps[-1]["state"]), "seed holds an executeAt tie: pick another"
    prunes = [st for st in steps if st["op"] == "prune"]
    assert len(prunes) == M.N_BATCHES - 1
    assert all(p["counts"]["entries_dropped"] > 0 and p["counts"]["missing_dropped"] > 0 for p in prunes)
    assert any(st["op"] == "apply" and st["trimmed"] > 0 for st in steps)
    assert lacking_trimmed_deps(steps), "no trimmed dep that its key lacks: pick another seed"
    if variant == "three":   # some txn is pruned from some of its keys only
        b0, b1 = CC.snap_as_batch(steps[0]["state"])[0], CC.snap_as_batch(steps[1]["state"])[0]
        n0 = {M.order(t): int(k) for t, k in zip(zip(b0.txn_msb, b0.txn_lsb, b0.txn_node), np.diff(b0.key_off.astype(np.int64)))}
        n1 = {M.order(t): int(k) for t, k in zip(zip(b1.txn_msb, b1.txn_lsb, b1.txn_node), np.diff(b1.key_off.astype(np.int64)))}
        assert any(0 < n1[t] < n0[t] for t in n1)


def run_chain(c, seed, variant, scans):
    from accord_amd.deps import CfkStore
    steps = chain(seed, variant)
    host_conditions(steps, variant)
    final = steps[-1]["state"]
    s = CfkStore(c)
    try:
        for i, st in enumerate(steps):
            msg = f"seed {seed} {variant} step {i} {st['op']}"
            if st["op"] == "apply":
                s.apply_deps(st["upd"])
                assert c.stats()["cfk.deps_trimmed"] == st["trimmed"], msg
            else:
                s.redundant_before(st["ranges"])
                assert_stats(c, st["counts"], msg)
                assert_map(s, st["map"], msg)
            assert_store(c, s, st["state"], msg)
        g = s.state()
        tk = {(int(g["key"][k]), M.order((g["emsb"][e], g["elsb"][e], g["enode"][e])))
              for k in range(len(g["key"])) for e in range(int(g["ent_off"][k]), int(g["ent_off"][k + 1]))
              if g["status"][e] == CC.TK}
        # (a lacking dep may be inserted by a later update of its own, with a status of its own; never as TRANSITIVELY_KNOWN
        # unless the model's trimmed stream makes it one too, which the state comparison above has settled)
        want_tk = {(int(final["key"][k]), M.order((final["emsb"][e], final["elsb"][e], final["enode"][e])))
                   for k in range(len(final["key"])) for e in range(int(final["ent_off"][k]), int(final["ent_off"][k + 1]))
                   if final["status"][e] == CC.TK}
        assert tk == want_tk
        if not scans:
            return
        ob, mo, mt = CC.snap_as_batch(final)
        KQ.assert_result(s.keydeps(KQ.member_queries(ob)), oracle.keydeps_batch(ob), f"seed {seed} {variant} keydeps")
        items = [(MX.ts(4 * 300 + 9, (4 << 1) | MX.RANGE, 2), None, [], [(M.KEY_LO, M.KEY_HI)])]
        MX.assert_result(s.keydeps_mixed(MX.make_mixed(items), 1), MX.expect_mixed(ob, items, 1), f"seed {seed} {variant} mixed")
        q = CC.recovery_queries(ob, seed, 80)
        hits = 0
        for sa, td, tst in RC.ALL_TESTS:
            o = oracle.map_reduce_full(ob, mo, mt, q, sa, td, tst)
            CR.assert_same(s.map_reduce_full(q, sa, td, tst), o, f"seed {seed} {variant} recovery {(sa, td, tst)}")
            hits += len(o.dep_txn)
        assert hits > 0
    finally:
        s.close()


@pytest.mark.parametrize("variant", ["single", "three"])
@pytest.mark.parametrize("seed", SEEDS)
def test_chained(ctx, seed, variant):
    run_chain(ctx, seed, variant, scans=True)


@pytest.mark.parametrize("variant", ["single", "three"])
def test_deps_trimming_through_the_closed_form(ctx_hot4, variant):
    """the same chain with the closed-form threshold at 4 elements: nearly every key takes the data-parallel form of the
    update (the default context above leaves them to the replay), fed the trimmed deps"""
    run_chain(ctx_hot4, SEEDS[0], variant, scans=False)
    assert ctx_hot4.stats().get("cfk.hot_keys", 0) > 0


# ---------------------------------------------------------------- 7. empty store and errors

def test_empty_store_and_errors(ctx):
    from accord_amd.deps import CfkStore, IllegalArgumentException, IllegalStateException
    upd, ranges, _, _ = M.handmade()
    s = CfkStore(ctx)
    try:
        m = M.BoundMap(1)
        assert_map(s, m, "no map yet")
        s.redundant_before(M.ranges_of([]))                      # n_ranges == 0: a no-op
        assert_map(s, m, "after a no-op")
        m.add(ranges)
        s.redundant_before(ranges)                               # an empty store records the map
        assert_map(s, m, "empty store")
        assert ctx.stats()["cfk.redundant_keys_advanced"] == 0
        state = apply(ctx, s, CC.empty_snapshot(), m, upd, "keys arriving under a bound")
        # key 200 (bound C): D's and E's dep A is ignored, so A is never added; key 100 (bound below A) has it
        assert [r[0] for r in M.describe(s.state())[200]] == [8, 12, 16, 20]
        assert [r[0] for r in M.describe(s.state())[100]] == [4, 8, 12, 16, 20]
        bad = [("unsorted", M.ranges_of([(300, 400, M.ts(40)), (100, 200, M.ts(40))]), 1),
               ("overlapping", M.ranges_of([(100, 250, M.ts(40)), (249, 400, M.ts(40))]), 1),
               ("start == end", M.ranges_of([(100, 100, M.ts(40))]), 1),
               ("start > end", M.ranges_of([(200, 100, M.ts(40))]), 1),
               ("end_inclusive 2", M.ranges_of([(0, 500, M.ts(40))]), 2),
               ("another bound type", M.ranges_of([(0, 500, M.ts(40))]), 0)]
        for name, r, ei in bad:
            with pytest.raises(IllegalArgumentException):
                s.redundant_before(r, ei)
            assert_store(ctx, s, state, name)
            assert_map(s, m, name)
        state = prune(ctx, s, state, m, M.ranges_of([(0, 500, M.ts(40))]), "a valid call after the failures")
        assert len(state["key"]) == 0 and len(s.state()["key"]) == 0
        assert s.snapshot().n_txn == 0
        state = apply(ctx, s, state, m, upd, "the store takes updates again")
    finally:
        s.close()
    s = CfkStore(ctx)
    try:
        s.update(CC.snap_as_batch(oracle.cfk_apply(CC.empty_snapshot(), upd))[0])   # status-only state
        with pytest.raises(IllegalStateException):
            s.redundant_before(ranges)
        assert s.snapshot().n_txn == 5
        assert len(s.redundant_map()["st"]) == 0
    finally:
        s.close()
