"""GPU parity for the recovery scans of the resident range-command store (acc_rcmd_update_cmds, acc_rcmd_state_view,
acc_rcmd_map_reduce_full: RangeCmdStore.update with state columns, .state(), .map_reduce_full,
ReplicaStore.begin_recovery_ranges).

Expected values: always oracle.map_reduce_full_ranges over the table a plain-Python model of the store holds
(rcmd_state_model.StateModel: test_rcmd_gpu.Model's ranges fold plus the state rules), queries passed with is_range = X's
domain bit, results compared as {(start, end): [TxnIds]} per query. After every update the store's table() and state()
are asserted equal to the model's, every column."""
import ctypes as C

import numpy as np
import pytest

import rcmd_state_model as M
from accord_amd import _lib as L
from accord_amd import workload as W
from accord_amd.deps import Context, IllegalArgumentException, IllegalStateException, RangeCmdStore, ReplicaStore
from recovery_cases import range_recovery_case
from test_rcmd_gpu import check_queries, queries, random_queries, ts

pytestmark = pytest.mark.gpu

ERASED, HAS_DEPS, KEEP_DEPS, HISTORICAL = L.ACC_RCMD_ERASED, L.ACC_RCMD_HAS_DEPS, L.ACC_RCMD_KEEP_DEPS, L.ACC_RCMD_HISTORICAL
BEFORE, AFTER, ANY = L.ACC_STARTED_BEFORE, L.ACC_STARTED_AFTER, L.ACC_STARTED_ANY
WITH, WITHOUT, ANY_DEPS = L.ACC_DEP_WITH, L.ACC_DEP_WITHOUT, L.ACC_DEP_ANY
ANY_STATUS, PROPOSED, STABLE = L.ACC_STATUS_ANY, L.ACC_STATUS_IS_PROPOSED, L.ACC_STATUS_IS_STABLE
BEGIN_RECOVERY = list(L.RECOVERY_SCANS.values())


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def cmd_updates(items):
    """items: [(txn_id, flags, [(start, end)], status, execute_at or None, [(dep txn_id, start, end, is_key)])] -> the
    RangeCmdStore.update dict with state columns"""
    ro, rs, re_, do, deps = [0], [], [], [0], []
    for _, _, ranges, _, _, dl in items:
        rs.extend(a for a, _ in ranges); re_.extend(b for _, b in ranges); ro.append(len(rs))
        deps.extend(dl); do.append(len(deps))
    ex = [t if x is None else x for t, _, _, _, x, _ in items]
    return dict(msb=np.array([i[0][0] for i in items], np.uint64), lsb=np.array([i[0][1] for i in items], np.uint64),
                node=np.array([i[0][2] for i in items], np.int32), flags=np.array([i[1] for i in items], np.uint8),
                rng_off=np.array(ro, np.uint32), rng_start=np.array(rs, np.uint64), rng_end=np.array(re_, np.uint64),
                status=np.array([i[3] for i in items], np.uint8), xmsb=np.array([x[0] for x in ex], np.uint64),
                xlsb=np.array([x[1] for x in ex], np.uint64), xnode=np.array([x[2] for x in ex], np.int32),
                dep_off=np.array(do, np.uint32), dep_msb=np.array([d[0][0] for d in deps], np.uint64),
                dep_lsb=np.array([d[0][1] for d in deps], np.uint64), dep_node=np.array([d[0][2] for d in deps], np.int32),
                dep_start=np.array([d[1] for d in deps], np.uint64), dep_end=np.array([d[2] for d in deps], np.uint64),
                dep_is_key=np.array([d[3] for d in deps], np.uint8))


def plain(upd):
    """the same updates without state columns (plain acc_rcmd_update)"""
    out = {k: upd[k] for k in ("msb", "lsb", "node", "rng_off", "rng_start", "rng_end")}
    out["flags"] = np.asarray(upd["flags"], np.uint8) & np.uint8(ERASED)
    return out


def rq(items):
    """items: [(X, [keys] or None, [(start, end)] or None)] -> recovery queries (is_range = X's domain bit)"""
    po, ps, pe = [0], [], []
    for x, keys, ranges in items:
        if x[1] & 1:
            ps.extend(a for a, _ in ranges); pe.extend(b for _, b in ranges)
        else:
            ps.extend(keys); pe.extend([0] * len(keys))
        po.append(len(ps))
    return dict(msb=np.array([x[0] for x, _, _ in items], np.uint64), lsb=np.array([x[1] for x, _, _ in items], np.uint64),
                node=np.array([x[2] for x, _, _ in items], np.int32), is_range=np.array([x[1] & 1 for x, _, _ in items], np.uint8),
                part_off=np.array(po, np.uint32), part_start=np.array(ps, np.uint64), part_end=np.array(pe, np.uint64))


def feed(store, model, upd, msg=""):
    store.update(upd)
    model.apply(upd)
    return M.assert_store(store, model, msg)


# ---------------------------------------------------------------- 1. the hand-worked store

def test_hand_worked_store(ctx):
    cmds, q, expected = M.handmade()
    s, m = RangeCmdStore(ctx, 0), M.StateModel(0)
    try:
        feed(s, m, M.updates_from_cmds(cmds, [1]), "first batch")
        feed(s, m, M.updates_from_cmds(cmds, [2, 0]), "second batch")
        ids = list(zip(cmds["txn_msb"].tolist(), cmds["txn_lsb"].tolist(), cmds["txn_node"].tolist()))
        for params, want in expected.items():
            g = M.check_scan(s, m.cmds(), q, params, msg="handmade")
            assert g[0] == {r: [ids[i] for i in d] for r, d in want.items()}, params
    finally:
        s.close()


# ---------------------------------------------------------------- 2. a chained random stream

# seeds under which the oracle alone finds a non-empty row under each of the four BeginRecovery sets, for both bound
# types (stableStartedBeforeAndWitnessed is the rare one: a command before X that lists X and executes at or after it)
STREAM_SEEDS = (9, 11, 12)


def stream(seed, ei):
    """range_recovery_case cut into 4 update batches in random command order: (name, update dict) steps, some through
    plain update, later batches revisiting earlier commands (a later status, a changed executeAt, the deps of another
    command or KEEP_DEPS, some with another command's ranges added), some TxnIds listed 2-3 times in one batch"""
    cmds, qs = range_recovery_case(seed, n_cmd=300, n_query=120, p_hist=0, p_hist_only=0, end_inclusive=ei)
    rng = np.random.default_rng(seed * 7919 + ei)
    n = len(cmds["txn_msb"])
    ro, do = cmds["rng_off"].astype(np.int64), cmds["dep_off"].astype(np.int64)

    def item(r, deps_of=None, more_ranges_of=None, **over):
        deps_of = r if deps_of is None else deps_of
        tid = lambda a, i: (int(cmds[a + "_msb"][i]), int(cmds[a + "_lsb"][i]), int(cmds[a + "_node"][i]))  # noqa: E731
        ranges = [(int(cmds["rng_start"][j]), int(cmds["rng_end"][j])) for j in range(ro[r], ro[r + 1])]
        if more_ranges_of is not None:
            o = more_ranges_of
            ranges = [(int(cmds["rng_start"][j]), int(cmds["rng_end"][j])) for j in range(ro[o], ro[o + 1])]
        deps = [((int(cmds["dep_msb"][j]), int(cmds["dep_lsb"][j]), int(cmds["dep_node"][j])), int(cmds["dep_start"][j]),
                 int(cmds["dep_end"][j]), int(cmds["dep_is_key"][j])) for j in range(do[deps_of], do[deps_of + 1])]
        it = dict(t=tid("txn", r), flags=int(cmds["flags"][r]), ranges=ranges, status=int(cmds["status"][r]), ex=tid("exe", r), deps=deps)
        it.update(over)
        return (it["t"], it["flags"], it["ranges"], it["status"], it["ex"], it["deps"])

    order = rng.permutation(n)
    steps = []
    for b in range(4):
        rows = [int(r) for r in order[b * n // 4:(b + 1) * n // 4]]
        items = [item(r) for r in rows]
        for r in rows[:12]:                                      # listed 2-3 times: earlier instances with another state
            for _ in range(int(rng.integers(1, 3))):
                other = int(rng.integers(0, n))
                items.insert(int(rng.integers(0, len(items) // 2)),
                             item(r, deps_of=other, status=int(rng.integers(0, 11)), flags=int(rng.choice([0, HAS_DEPS, KEEP_DEPS]))))
        for r in (order[:b * n // 4][rng.integers(0, max(1, b * n // 4), size=25)] if b else []):   # revisits
            r, u = int(r), rng.random()
            fl = int(cmds["flags"][r]) & HAS_DEPS
            over = dict(status=min(10, int(cmds["status"][r]) + int(rng.integers(0, 4))))
            if u < 0.3:
                over["ex"] = tuple(int(x) for x in W.encode_ts(1, 2 * r + 2 + int(rng.integers(1, 60)), 0, 1 + int(rng.integers(0, 4))))
            if u < 0.5:
                over["flags"] = fl | KEEP_DEPS
            else:
                over["deps_of"] = int(rng.integers(0, n))
                over["flags"] = int(rng.choice([0, HAS_DEPS]))
            if rng.random() < 0.3:
                over["more_ranges_of"] = int(rng.integers(0, n))
            items.append(item(r, **over))
        upd = cmd_updates(items)
        if b == 1:                                               # the first third through plain update
            cut = len(items) // 3
            steps.append((f"batch {b} plain", plain(cmd_updates(items[:cut]))))
            upd = cmd_updates(items[cut:])
        steps.append((f"batch {b}", upd))
    return steps, M.domain_queries(qs)


@pytest.mark.parametrize("ei", [0, 1])
@pytest.mark.parametrize("seed", STREAM_SEEDS)
def test_chained_random_stream(ctx, seed, ei):
    steps, q = stream(seed, ei)
    s, m = RangeCmdStore(ctx, ei), M.StateModel(ei)
    nonempty = {p: 0 for p in BEGIN_RECOVERY}
    try:
        for name, upd in steps:
            feed(s, m, upd, name)
            st = ctx.stats()
            for k, v in m.stats.items():
                assert st["rcmd." + k] == v, (name, k)
            if name.endswith("plain"):
                continue
            cmds = m.cmds()
            for params in M.ALL_PARAMS:
                g = M.check_scan(s, cmds, q, params, msg=name)
                if params in nonempty:
                    nonempty[params] += sum(1 for d in g if d)
            M.check_scan(s, cmds, q, (ANY, WITHOUT, PROPOSED, False), test_kinds=0x3F, msg=name)
            M.check_scan(s, cmds, q, (BEFORE, ANY_DEPS, ANY_STATUS, True), test_kinds=1 << W.WRITE, msg=name)
        assert "in_batch_repeat" in m.seen and "merged" in m.seen, m.seen
        # the oracle alone (check_scan compared equal to it) found something under each BeginRecovery set
        assert all(v > 0 for v in nonempty.values()), nonempty
    finally:
        s.close()


# ---------------------------------------------------------------- 3. window edges

def brute_raw_entries(tab, q, params, ei, test_kinds=-1):
    """(participant, stored entry) intersections whose command is inside the TxnId window and the Kinds mask"""
    wb = {0: 0b011010, 1: 0b011011, 2: 0, 3: 0b010000, 4: 0b010000}   # Kind.witnessedBy()
    idt = lambda t: (t[0], t[1] & 0xFFFFFFFFFFFF001E, t[2])  # noqa: E731
    total = 0
    for i in range(len(q["msb"])):
        x = idt((int(q["msb"][i]), int(q["lsb"][i]), int(q["node"][i])))
        mask = wb[(int(q["lsb"][i]) >> 1) & 7] if test_kinds < 0 else test_kinds
        for p in range(int(q["part_off"][i]), int(q["part_off"][i + 1])):
            a, b = int(q["part_start"][p]), int(q["part_end"][p])
            for c in range(len(tab["msb"])):
                t = idt((int(tab["msb"][c]), int(tab["lsb"][c]), int(tab["node"][c])))
                if tab["flags"][c] & ERASED or not (mask >> ((int(tab["lsb"][c]) >> 1) & 7)) & 1:
                    continue
                if (params[0] == BEFORE and not t < x) or (params[0] == AFTER and not t > x):
                    continue
                for j in range(int(tab["rng_off"][c]), int(tab["rng_off"][c + 1])):
                    s, e = int(tab["rng_start"][j]), int(tab["rng_end"][j])
                    if q["is_range"][i]:
                        total += s < b and a < e
                    else:
                        total += (s < a <= e) if ei else (s <= a < e)
    return total


@pytest.mark.parametrize("ei", [0, 1])
def test_window_edges(ctx, ei):
    kinds = [W.WRITE, W.READ, W.WRITE, W.EXCLUSIVE_SYNC_POINT, W.SYNC_POINT, W.WRITE]
    items = [(ts(10 * (i + 1), kinds[i], node=2), HAS_DEPS if i % 2 else 0, [(10 * i, 10 * i + 35)], 3 + i, None, []) for i in range(6)]
    items[4] = (items[4][0], ERASED, [], 9, None, [])
    s, m = RangeCmdStore(ctx, ei), M.StateModel(ei)
    try:
        tab, _ = feed(s, m, cmd_updates(items), "edges")
        xs = [ts(5, W.WRITE, node=2), ts(70, W.WRITE, node=2), ts(30, W.WRITE, node=2), ts(30, W.WRITE, node=2, extra=0x100),
              ts(30, W.WRITE, node=1), ts(40, W.EXCLUSIVE_SYNC_POINT, node=2, rng=0), ts(20, W.READ, node=2, rng=0)]
        q = rq([(x, [12, 35, 61], [(0, 100)]) for x in xs])
        cmds = m.cmds()
        for sa in (BEFORE, AFTER, ANY):
            for td, tst in ((ANY_DEPS, ANY_STATUS), (WITHOUT, ANY_STATUS), (ANY_DEPS, STABLE)):
                params = (sa, td, tst, False)
                g = M.check_scan(s, cmds, q, params, msg="edges")
                st = ctx.stats()
                assert st["rcr.raw_entries"] == brute_raw_entries(tab, q, params, ei), params
                assert st["rcr.kept_entries"] <= st["rcr.raw_entries"] and st["rcr.queries"] == len(q["part_start"])
                if td == ANY_DEPS and tst == ANY_STATUS:
                    assert st["rcr.kept_entries"] == st["rcr.raw_entries"]   # the window and the kinds are the whole test
            own = M.check_scan(s, cmds, q, (sa, ANY_DEPS, ANY_STATUS, False))[2]
            x_is_listed = any(M.ident(xs[2]) == M.ident(t) for deps in own.values() for t in deps)
            assert x_is_listed == (sa == ANY), "only ANY visits the command Timestamp.equals to X"
        below = M.check_scan(s, cmds, q, (BEFORE, ANY_DEPS, ANY_STATUS, False))
        assert not below[0]                                              # X below every stored TxnId: nothing started before
        above = M.check_scan(s, cmds, q, (AFTER, ANY_DEPS, ANY_STATUS, False))
        assert not above[1]                                              # X above every stored TxnId: nothing started after
        for sa in (BEFORE, AFTER, ANY):
            flagged = M.check_scan(s, cmds, q, (sa, ANY_DEPS, ANY_STATUS, False))
            assert flagged[2] == flagged[3] and flagged[2]               # raw flag bits outside the identity change nothing
    finally:
        s.close()


# ---------------------------------------------------------------- 4. compaction boundaries of the filter

SPANS = (0, 1, 63, 64, 65, 300)
PATTERNS = {"all": lambda i, n: True, "none": lambda i, n: False, "every other": lambda i, n: i % 2 == 0,
            "first": lambda i, n: i == 0, "last": lambda i, n: i == n - 1}


@pytest.mark.parametrize("ei", [0, 1])
def test_filter_compaction_boundaries(ctx, ei):
    """Group j holds SPANS[j] commands, each over [1000 j, 1000 j + 10) and [1000 j + 20, 1000 j + 30): a key participant
    at 1000 j + 5 or 1000 j + 25 has a span of exactly SPANS[j] raw entries, in TxnId order within the group. Survivors
    (IS_STABLE) follow the pattern within each group. Query j lists group j's two keys; one more query lists all
    twelve. 24 participants are 6 blocks of 4 waves: 6 and 3 launches at wave_grid_max 1 and 2."""
    small = [Context(0, wave_grid_max=1), Context(0, wave_grid_max=2)]
    try:
        for name, keep in PATTERNS.items():
            items, h = [], 0
            for j, n in enumerate(SPANS):
                for i in range(n):
                    h += 1
                    items.append((ts(h, W.WRITE), 0, [(1000 * j, 1000 * j + 10), (1000 * j + 20, 1000 * j + 30)],
                                  6 if keep(i, n) else 2, None, []))
            keys = [[1000 * j + 5, 1000 * j + 25] for j in range(len(SPANS))]
            q = rq([(ts(9000 + j, W.WRITE, rng=0), k, None) for j, k in enumerate(keys)]
                   + [(ts(9100, W.WRITE, rng=0), sorted(sum(keys, [])), None)])
            kept = 4 * sum(sum(1 for i in range(n) if keep(i, n)) for n in SPANS)
            results = []
            for c, launches in ((ctx, 1), (small[0], 6), (small[1], 3)):
                s, m = RangeCmdStore(c, ei), M.StateModel(ei)
                try:
                    feed(s, m, cmd_updates(items), name)
                    results.append(M.check_scan(s, m.cmds(), q, (ANY, ANY_DEPS, STABLE, False), msg=name))
                    st = c.stats()
                    assert st["rcr.raw_entries"] == 4 * sum(SPANS) and st["rcr.kept_entries"] == kept, (name, st)
                    assert st["rcr.wave_launches"] == launches, (name, st["rcr.wave_launches"])
                finally:
                    s.close()
            assert results[0] == results[1] == results[2]
            assert not results[0][0] and (name == "none") == (not results[0][5])
    finally:
        for c in small:
            c.close()


# ---------------------------------------------------------------- 5. the deps probe

@pytest.mark.parametrize("ei", [0, 1])
def test_deps_probe(ctx, ei):
    x = ts(500, W.WRITE)
    xk = ts(500, W.WRITE, rng=0)                                  # the same TxnId as a key-domain query
    lo = [((ts(h, W.WRITE)), 1000 + h, 0, 1) for h in range(1, 300)]      # 299 deps below X
    hi = [((ts(h, W.WRITE)), 1000 + h, 0, 1) for h in range(501, 800)]    # 299 deps above X
    R = [(100, 200)]
    hit_key, miss_key = (x, 150, 0, 1), (x, 250, 0, 1)
    cmds = [
        (HAS_DEPS, []),                                           # 0: no deps
        (HAS_DEPS, [hit_key]),                                    # 1: one dep, X
        (HAS_DEPS, [hit_key, hi[0]]),                             # 2: two, X first
        (HAS_DEPS, lo + [hit_key]),                               # 3: 300, X last
        (HAS_DEPS, lo[:150] + hi[:150]),                          # 4: 300, X absent
        (HAS_DEPS, lo[:5] + [miss_key, (x, 300, 400, 0), hit_key] + hi[:5]),   # 5: X three times, only the last intersects
        (HAS_DEPS, [(x, 100, 0, 1)]),                             # 6: a key on the start bound: inside [100, 200) only
        (HAS_DEPS, [(x, 200, 0, 1)]),                             # 7: a key on the end bound: inside (100, 200] only
        (HAS_DEPS, [(x, 200, 260, 0)]),                           # 8: a range that only touches
        (HAS_DEPS, [(x, 50, 100, 0)]),                            # 9: touching from below
        (0, [hit_key]),                                           # 10: X listed, HAS_DEPS clear
        (HAS_DEPS, [(x, 199, 201, 0)]),                           # 11: a range that overlaps by one
    ]
    items = [(ts(600 + i, W.WRITE), f, R, 6, None, d) for i, (f, d) in enumerate(cmds)]
    s, m = RangeCmdStore(ctx, ei), M.StateModel(ei)
    try:
        feed(s, m, cmd_updates(items), "deps")
        q = rq([(x, None, [(0, 1000)]), (xk, [150], None)])
        mc = m.cmds()
        with_ = M.check_scan(s, mc, q, (ANY, WITH, ANY_STATUS, False), msg="WITH")
        assert ctx.stats()["rcr.dep_probes"] == 2 * 11            # every command with HAS_DEPS, per participant
        without = M.check_scan(s, mc, q, (ANY, WITHOUT, ANY_STATUS, False), msg="WITHOUT")
        anyd = M.check_scan(s, mc, q, (ANY, ANY_DEPS, ANY_STATUS, False), msg="ANY_DEPS")
        assert ctx.stats()["rcr.dep_probes"] == 0
        ids = [it[0] for it in items]
        pos = lambda g: sorted(ids.index(t) for t in g.get((100, 200), []))  # noqa: E731
        inside = [1, 2, 3, 5, 11] + ([7] if ei else [6])
        for k in range(2):
            assert pos(with_[k]) == sorted(inside), (k, pos(with_[k]))
            assert pos(without[k]) == sorted(set(range(12)) - set(inside) - {10})
            assert pos(anyd[k]) == list(range(12))
        M.check_scan(s, mc, q, (AFTER, WITHOUT, STABLE, False), msg="AFTER")
        M.check_scan(s, mc, q, (BEFORE, WITH, STABLE, False), msg="BEFORE")
    finally:
        s.close()


# ---------------------------------------------------------------- 6. the life of a command's state

@pytest.mark.parametrize("ei", [0, 1])
def test_state_lifecycle(ctx, ei):
    a, b, low, kd = ts(100, W.WRITE), ts(200, W.WRITE), ts(50, W.WRITE), ts(150, W.WRITE, rng=0)
    x = ts(10, W.WRITE)
    dep = [(x, 15, 0, 1)]
    s, m = RangeCmdStore(ctx, ei), M.StateModel(ei)
    try:
        # KEEP_DEPS on a new command: none; a key-domain TxnId with state columns is skipped
        feed(s, m, cmd_updates([(a, KEEP_DEPS | HAS_DEPS, [(10, 20)], 3, None, dep), (kd, HAS_DEPS, [(1, 2)], 5, None, dep)]), "new keep")
        st = s.state()
        assert st["flags"].tolist() == [0] and st["dep_off"].tolist() == [0, 0] and ctx.stats()["rcmd.skipped_key_domain"] == 1
        feed(s, m, cmd_updates([(a, HAS_DEPS, [], 4, b, dep)]), "deps stored")
        # kept across an insert of a lower TxnId that shifts the row
        feed(s, m, cmd_updates([(a, KEEP_DEPS, [(30, 40)], 6, None, []), (low, 0, [(0, 5)], 1, None, [])]), "keep and shift")
        st = s.state()
        assert st["dep_off"].tolist() == [0, 0, 1] and st["flags"].tolist() == [0, HAS_DEPS] and st["status"].tolist() == [1, 6]
        # plain update: a new row is NotDefined at its TxnId, a stored state stays
        feed(s, m, plain(cmd_updates([(b, 0, [(50, 60)], 0, None, []), (a, 0, [(70, 80)], 0, None, [])])), "plain")
        st = s.state()
        assert st["status"].tolist() == [1, 6, 0] and (int(st["xmsb"][2]), int(st["xlsb"][2]), int(st["xnode"][2])) == b
        assert st["dep_off"].tolist() == [0, 0, 1, 1]
        q = rq([(x, None, [(0, 100)])])
        for p in M.ALL_PARAMS:
            M.check_scan(s, m.cmds(), q, p, msg="lifecycle")
        # a store rebuilt from state() + table() of this one answers identically
        tab, st = s.table(), s.state()
        s2, m2 = RangeCmdStore(ctx, ei), M.StateModel(ei)
        try:
            feed(s2, m2, M.updates_from_cmds(M.cmds_of(tab, st, ei), range(len(tab["msb"]))), "rebuilt")
            for f in M.STATE_FIELDS:
                np.testing.assert_array_equal(s2.state()[f], st[f], err_msg=f)
            for p in M.ALL_PARAMS:
                M.check_scan(s2, m.cmds(), q, p, msg="rebuilt")
        finally:
            s2.close()
        # erase drops the deps; a later update with deps is ignored
        feed(s, m, cmd_updates([(a, ERASED, [], 9, None, dep)]), "erase")
        feed(s, m, cmd_updates([(a, HAS_DEPS, [(1, 2)], 3, None, dep)]), "after erase")
        st = s.state()
        assert ctx.stats()["rcmd.erased_ignored"] == 1
        assert st["flags"].tolist() == [0, ERASED, 0] and st["status"].tolist() == [1, 9, 0] and st["dep_off"].tolist() == [0, 0, 0, 0]
    finally:
        s.close()


# ---------------------------------------------------------------- 7. empties and errors

def snapshot(s):
    return s.table(), s.state()


def assert_unchanged(s, snap, msg):
    tab, st = snapshot(s)
    for f in M.TABLE_FIELDS:
        assert tab[f].tobytes() == snap[0][f].tobytes(), f"{msg}: table {f}"
    for f in M.STATE_FIELDS:
        assert st[f].tobytes() == snap[1][f].tobytes(), f"{msg}: state {f}"


def raw_scan(ctx, s, q, **over):
    """acc_rcmd_map_reduce_full with fields the Python wrapper does not expose"""
    a = {k: np.ascontiguousarray(q[k], dt) for k, dt in (("msb", np.uint64), ("lsb", np.uint64), ("node", np.int32),
                                                         ("key_off", np.uint32), ("key_code", np.uint64), ("rng_off", np.uint32),
                                                         ("rng_start", np.uint64), ("rng_end", np.uint64))}
    p = lambda k: a[k].ctypes.data  # noqa: E731
    f = dict(end_inclusive=s.end_inclusive, started_at=0, test_dep=2, test_status=0, flags=0, test_kinds=-1)
    f.update(over)
    ri = L.CfkRecoveryIn(len(a["msb"]), L.ACC_MEM_HOST, len(a["key_code"]), len(a["rng_start"]), L.TsCols(p("msb"), p("lsb"), p("node")),
                         p("key_off"), p("key_code"), p("rng_off"), p("rng_start"), p("rng_end"), f["end_inclusive"],
                         f["started_at"], f["test_dep"], f["test_status"], f["flags"], f["test_kinds"])
    view = L.RangedepsView()
    ctx.check(ctx._lib.acc_rcmd_map_reduce_full(ctx.handle, s._h, C.byref(ri), C.byref(view)))
    return ctx.copy_out_range(view)


def test_empties_and_errors(ctx):
    ei = 1
    x = ts(10, W.WRITE)
    q1 = rq([(x, None, [(0, 100)]), (ts(11, W.WRITE, rng=0), [5, 15], None)])
    s, m = RangeCmdStore(ctx, ei), M.StateModel(ei)
    try:
        # an empty store; no queries; queries without participants; only erased commands
        for p in BEGIN_RECOVERY:
            assert M.check_scan(s, m.cmds(), q1, p, msg="empty store") == [{}, {}]
        assert s.state()["dep_off"].tolist() == [0]
        feed(s, m, cmd_updates([(ts(20, W.WRITE), ERASED, [(0, 50)], 9, None, []), (ts(30, W.WRITE), ERASED, [], 10, None, [])]), "erased only")
        for p in BEGIN_RECOVERY + [(ANY, ANY_DEPS, ANY_STATUS, False)]:
            assert M.check_scan(s, m.cmds(), q1, p, msg="erased only") == [{}, {}]
        good = [(ts(40, W.WRITE), HAS_DEPS, [(0, 50)], 6, None, [(x, 5, 0, 1), (ts(12, W.WRITE), 10, 20, 0)]),
                (ts(50, W.WRITE), HAS_DEPS, [(40, 90)], 3, ts(60, W.WRITE), [(x, 45, 0, 1)])]
        feed(s, m, cmd_updates(good), "good")
        mc = m.cmds()
        assert M.check_scan(s, mc, rq([]), (ANY, ANY_DEPS, ANY_STATUS, False), msg="no queries") == []
        none = rq([(x, None, []), (ts(11, W.WRITE, rng=0), [], None)])
        assert M.check_scan(s, mc, none, (ANY, ANY_DEPS, ANY_STATUS, False), msg="no participants") == [{}, {}]
        assert any(M.check_scan(s, mc, q1, (ANY, ANY_DEPS, ANY_STATUS, False)))

        # ---- update errors: ACC_E_ARG, the table and the state byte-equal to before
        snap = snapshot(s)
        t = ts(70, W.WRITE)
        d2 = [(ts(12, W.WRITE), 5, 0, 1), (ts(13, W.WRITE), 10, 20, 0)]

        def bad(**over):
            u = cmd_updates([(t, HAS_DEPS, [(1, 2)], 3, None, d2), (ts(80, W.WRITE), 0, [(3, 4)], 3, None, [])])
            for k, (i, v) in over.items():
                u[k] = u[k].copy()
                u[k][i] = v
            return u
        longer = bad()                                               # one dep more than dep_off covers
        for k, _ in M.DEP_COLS:
            longer[k] = np.concatenate([longer[k], longer[k][-1:]])
        cases = {
            "dep_off not ending at n_deps": longer,
            "unsorted dep TxnIds": cmd_updates([(t, HAS_DEPS, [(1, 2)], 3, None, d2[::-1])]),
            "dep range start >= end": bad(dep_end=(1, 10)),
            "dep_is_key = 2": bad(dep_is_key=(0, 2)),
            "dep_off not from 0": bad(dep_off=(0, 1)),
            "dep_off decreasing": bad(dep_off=(1, 3)),
            "dep_off ending below": bad(dep_off=(2, 1)),
            "status = 11": bad(status=(1, 11)),
            "HISTORICAL": bad(flags=(0, HISTORICAL)),
            "an unknown flag": bad(flags=(1, 16)),
        }
        for name, u in cases.items():
            with pytest.raises(IllegalArgumentException):
                s.update(u)
            assert_unchanged(s, snap, name)
        with pytest.raises(IllegalArgumentException):                # plain update keeps its flag rule
            s.update(dict(plain(bad()), flags=np.array([HAS_DEPS, 0], np.uint8)))
        assert_unchanged(s, snap, "plain flags")
        feed(s, m, bad(), "the next valid update")

        # ---- query errors; the next valid call on the context succeeds
        mq = M.mixed(q1)
        mc = m.cmds()
        errors = [dict(end_inclusive=0), dict(started_at=3), dict(test_dep=3), dict(test_status=3), dict(test_kinds=0x40),
                  dict(flags=2)]
        for over in errors:
            with pytest.raises(IllegalArgumentException):
                raw_scan(ctx, s, mq, **over)
            M.check_scan(s, mc, q1, (ANY, ANY_DEPS, ANY_STATUS, False), msg=str(over))
        local = rq([(ts(10, W.LOCAL_ONLY), None, [(0, 100)])])
        with pytest.raises(IllegalStateException):
            s.map_reduce_full(M.mixed(local), ANY, ANY_DEPS, ANY_STATUS)
        M.check_scan(s, mc, local, (ANY, ANY_DEPS, ANY_STATUS, False), test_kinds=0x3F, msg="a mask: X's kind is not read")
        mism = M.mixed(q1)
        mism["lsb"] = mism["lsb"] ^ np.uint64(1)                     # the domain bit against the participants
        with pytest.raises(IllegalArgumentException):
            s.map_reduce_full(mism, ANY, ANY_DEPS, ANY_STATUS)
        M.check_scan(s, mc, q1, (BEFORE, WITH, STABLE, False), msg="after the errors")
    finally:
        s.close()


# ---------------------------------------------------------------- 8. unchanged neighbours

def test_unchanged_neighbours(ctx):
    ei = 1
    steps, _ = stream(STREAM_SEEDS[0], ei)
    s, m = RangeCmdStore(ctx, ei), M.StateModel(ei)
    try:
        for name, upd in steps[:3]:
            feed(s, m, upd, name)
        rng = np.random.default_rng(5)
        ids = list(zip(*(s.table()[k].tolist() for k in ("msb", "lsb", "node"))))
        check_queries(s, queries(random_queries(rng, 200, ids, np.arange(0, 1000))), ei, "rangedeps after a mixed stream")
    finally:
        s.close()
    import oracle
    from recovery_cases import rangedeps_as_dict
    cmds, q = range_recovery_case(17, n_cmd=200, n_query=60)
    for sa, td, tst, after in BEGIN_RECOVERY + [(ANY, ANY_DEPS, ANY_STATUS, False), (ANY, WITH, ANY_STATUS, True)]:
        g = ctx.map_reduce_full_ranges(cmds, q, sa, td, tst, executes_after=after)
        o = oracle.map_reduce_full_ranges(cmds, q, sa, td, tst, -1, after)
        for f in ("arena_off", "rd_off", "u_off", "arena", "range_id", "dep_txn"):
            np.testing.assert_array_equal(getattr(g, f), getattr(o, f), err_msg=f)
        assert [rangedeps_as_dict(g, i) for i in range(60)] == [rangedeps_as_dict(o, i) for i in range(60)]


# ---------------------------------------------------------------- 9. ReplicaStore.begin_recovery_ranges

def test_replica_store_range_half(ctx):
    ei = 1
    u = W.cfk_update_stream(300, keys_per_txn=3, n_keys=100, seed=0x51)
    cuts = W.cfk_stream_cuts(u, 100, 100, 2)
    cmds, qs = range_recovery_case(41, n_cmd=120, n_query=40, p_hist=0, p_hist_only=0, end_inclusive=ei)
    qs = M.domain_queries(qs)
    rs, m = ReplicaStore(ctx, ei), M.StateModel(ei)
    try:
        for b, (a0, a1) in enumerate(zip([0] + cuts[:-1], cuts)):
            rp = M.updates_from_cmds(cmds, range(40 * b, 40 * b + 40))
            rs.preaccept_batch(W.cfk_slice(u, a0, a1), scan=False, range_part=rp)
            m.apply(rp)
            M.assert_store(rs.rcmd, m, f"replica batch {b}")
        mq = M.mixed(qs)
        plain_keys = set(rs.begin_recovery(mq))                     # the key half: exactly the keys it had
        assert plain_keys == {"accepted_started_before_without", "stable_started_before_with",
                              "has_accepted_started_after_without", "has_stable_executes_after_without"}
        r = dict(ranges=rs.begin_recovery_ranges(mq))
        assert set(r["ranges"]) == plain_keys
        names = dict(accepted_started_before_without="acceptedOrCommittedStartedBeforeWithoutWitnessing",
                     stable_started_before_with="stableStartedBeforeAndWitnessed",
                     has_accepted_started_after_without="hasAcceptedOrCommittedStartedAfterWithoutWitnessing",
                     has_stable_executes_after_without="hasStableExecutesAfterWithoutWitnessing")
        mc = m.cmds()
        tab = dict(msb=mc["txn_msb"], lsb=mc["txn_lsb"], node=mc["txn_node"])
        found = 0
        for name, scan in names.items():
            want = M.expect(mc, qs, L.RECOVERY_SCANS[scan])
            got = r["ranges"][name]
            if name.startswith("has_"):
                assert got.dtype == bool and got.tolist() == [bool(w) for w in want], name
            else:
                assert M.as_txn_dicts(got, len(qs["msb"]), tab) == want, name
            found += sum(1 for w in want if w)
        assert found > 0
    finally:
        rs.close()
