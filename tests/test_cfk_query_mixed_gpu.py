"""GPU parity for acc_cfk_keydeps_mixed (CfkStore.keydeps_mixed): PreAccept's deps for key- and range-domain txns against
the resident CommandsForKey store (impl/InMemoryCommandStore.java:257-292; the Range case, :274-289, runs
CommandsForKey.mapReduceActive on every CFK inside each range). Expected values are the C restatement's: key rows as in
test_cfk_query_gpu.py (oracle.keydeps_batch over the host restatement of the store's txn-major view + the query as a
PREACCEPTED entry), range rows from oracle.keydeps_mixed_queries over that view with the range queries appended as
range-domain txns (no keys, their ranges in rng_off) — a range txn is no CFK member, so the store indices stay as they
are and a range row's key_idx / kd_key follow the covered-key convention.

The lane tier (csrc/cfkquery.hip: one lane per covered key with a short segment) is a knob of the call (lane_seg), and
results may not depend on it: every case runs with the tier at its default, forced narrow, forced wide and off.
The tie rule holds here as for acc_cfk_keydeps: stores are asserted free of committed executeAt ties on the host
(no_committed_ties) before the device is asked."""
import numpy as np
import pytest

import cfk_cases as CC
import oracle
from accord_amd import _lib as L
from accord_amd import workload as W

pytestmark = pytest.mark.gpu

FIELDS = ("arena_off", "kd_off", "u_off", "arena", "key_idx", "dep_txn")
WRITE, ESP = 1 << 1, 4 << 1
RANGE = 1           # the TxnId's domain bit
SMALL_CAP = 11      # the one-wave build tier's hit cap in the context that exercises the sorting tier
NONE = L.ACC_CFQ_LANE_NONE


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_small_cap():
    from accord_amd.deps import Context
    c = Context(0, cfq_wave_cap=SMALL_CAP)
    yield c
    c.close()


def ts(hlc, flags=WRITE, node=1):
    return tuple(int(x) for x in W.encode_ts(1, hlc, flags, node))


def make_mixed(items):
    """items: [(txn_id, execute_at or None, [key codes], [(start, end)])] -> the CfkStore.keydeps_mixed queries dict"""
    qm, ql, qn, xm, xl, xn, ko, kc, ro, rs, re_ = [], [], [], [], [], [], [0], [], [0], [], []
    for tid, ex, keys, ranges in items:
        ex = tid if ex is None else ex
        qm.append(tid[0]); ql.append(tid[1]); qn.append(tid[2])
        xm.append(ex[0]); xl.append(ex[1]); xn.append(ex[2])
        kc.extend(keys)
        ko.append(len(kc))
        rs.extend(a for a, _ in ranges); re_.extend(b for _, b in ranges)
        ro.append(len(rs))
    return dict(msb=np.array(qm, np.uint64), lsb=np.array(ql, np.uint64), node=np.array(qn, np.int32),
                xmsb=np.array(xm, np.uint64), xlsb=np.array(xl, np.uint64), xnode=np.array(xn, np.int32),
                key_off=np.array(ko, np.uint32), key_code=np.array(kc, np.uint64), rng_off=np.array(ro, np.uint32),
                rng_start=np.array(rs, np.uint64), rng_end=np.array(re_, np.uint64))


def with_queries(ob, entries):
    """ob with entries [(txn_id, execute_at or None, [key codes])] appended as PREACCEPTED txns (indices ob.n_txn + i; the
    store indices stay as they are)"""
    cat = lambda a, v, dt: np.concatenate([np.asarray(a, dt), np.array(v, dt)])  # noqa: E731
    ex = [t if x is None else x for t, x, _ in entries]
    koff = int(ob.key_off[-1]) + np.cumsum([len(k) for _, _, k in entries])
    return W.Batch(cat(ob.txn_msb, [t[0] for t, _, _ in entries], np.uint64), cat(ob.txn_lsb, [t[1] for t, _, _ in entries], np.uint64),
                   cat(ob.txn_node, [t[2] for t, _, _ in entries], np.int32), cat(ob.exe_msb, [x[0] for x in ex], np.uint64),
                   cat(ob.exe_lsb, [x[1] for x in ex], np.uint64), cat(ob.exe_node, [x[2] for x in ex], np.int32),
                   cat(ob.status, [CC.PRE] * len(entries), np.uint8), cat(ob.key_off, koff, np.uint32),
                   cat(ob.key_code, [c for _, _, k in entries for c in k], np.uint64))


def range_rows(ob, items, end_inclusive):
    """[(key_idx, dep_txn, arena, kd_key)] of the range-domain items: one oracle run over ob + every one of them appended"""
    if not items:
        return []
    kb = with_queries(ob, [(tid, ex, []) for tid, ex, _, _ in items])
    roff = np.concatenate([np.zeros(ob.n_txn, np.int64), np.cumsum([0] + [len(r) for _, _, _, r in items])]).astype(np.uint32)
    rb = W.RangeBatch(kb, roff, np.array([a for _, _, _, r in items for a, _ in r], np.uint64),
                      np.array([b for _, _, _, r in items for _, b in r], np.uint64), end_inclusive)
    idx = [ob.n_txn + i for i in range(len(items))]
    o = oracle.keydeps_mixed_queries(rb, idx)
    return [o.txn(t) + (o.kd_key[int(o.kd_off[t]):int(o.kd_off[t + 1])],) for t in idx]


def key_row(ob, item):
    """one key-domain query: the oracle over ob + the query as a PREACCEPTED entry, queried alone"""
    tid, ex, keys, _ = item
    k, d, a = oracle.keydeps_batch(with_queries(ob, [(tid, ex, keys)]), queries=[ob.n_txn]).txn(ob.n_txn)
    return k, d, a, np.array(keys, np.uint64)[k.astype(np.int64)]


def join_rows(parts):
    """[(key_idx, dep_txn, arena, kd_key)] per query -> one result over len(parts) queries (FIELDS + kd_key)"""
    r = {}
    for f, i in (("kd_off", 0), ("u_off", 1), ("arena_off", 2)):
        r[f] = np.concatenate([[0], np.cumsum([len(p[i]) for p in parts])]).astype(np.uint64)
    for f, i, dt in (("key_idx", 0, np.uint32), ("dep_txn", 1, np.uint32), ("arena", 2, np.int32), ("kd_key", 3, np.uint64)):
        r[f] = np.concatenate([np.asarray(p[i]) for p in parts]).astype(dt) if parts else np.zeros(0, dt)
    return r


def is_range(item):
    return bool(item[0][1] & 1)


def expect_mixed(ob, items, end_inclusive):
    rr = iter(range_rows(ob, [it for it in items if is_range(it)], end_inclusive))
    return join_rows([next(rr) if is_range(it) else key_row(ob, it) for it in items])


def assert_result(g, want, msg):
    for f in FIELDS + ("kd_key",):
        np.testing.assert_array_equal(np.asarray(getattr(g, f)), np.asarray(want[f]), err_msg=f"{msg}: {f}")


def no_committed_ties(state):
    """no key holds two committed-class entries with one executeAt (the state the tie rule rejects)"""
    off = state["ent_off"].astype(np.int64)
    for k in range(len(state["key"])):
        seen = set()
        for e in range(off[k], off[k + 1]):
            if CC.COMMITTED <= int(state["status"][e]) <= CC.APPLIED:
                x = (int(state["xmsb"][e]), int(state["xlsb"][e]) & 0xFFFFFFFFFFFF001E, int(state["xnode"][e]))
                if x in seen:
                    return False
                seen.add(x)
    return True


def cover(codes, j0, j1, end_inclusive):
    """the range that covers exactly the sorted store keys codes[j0:j1] (the neighbours lie further than 1 away)"""
    return (int(codes[j0]) - 1, int(codes[j1 - 1])) if end_inclusive else (int(codes[j0]), int(codes[j1 - 1]) + 1)


# ---------------------------------------------------------------- 1. hand-worked

def test_handmade(ctx):
    from accord_amd.deps import CfkStore
    upd, _ = CC.handmade()       # key 500: [A COMMITTED, B COMMITTED, C ACCEPTED]; a Write at hlc 16: M = B, A pruned
    s = CfkStore(ctx)
    try:
        s.apply_deps(upd)
        for lane_seg in (0, 1, NONE):
            for rng, ei in (((499, 500), 1), ((500, 501), 0)):
                g = s.keydeps_mixed(make_mixed([(ts(16, WRITE | RANGE), None, [], [rng])]), ei, lane_seg)
                np.testing.assert_array_equal(g.arena_off, [0, 3])
                np.testing.assert_array_equal(g.arena, [3, 0, 1])
                np.testing.assert_array_equal(g.kd_off, [0, 1])
                np.testing.assert_array_equal(g.key_idx, [0])
                np.testing.assert_array_equal(g.kd_key, [500])
                np.testing.assert_array_equal(g.u_off, [0, 2])
                np.testing.assert_array_equal(g.dep_txn, [1, 2])
            for rng, ei in (((500, 501), 1), ((499, 500), 0)):      # the bound on 500 is the open one
                g = s.keydeps_mixed(make_mixed([(ts(16, WRITE | RANGE), None, [], [rng])]), ei, lane_seg)
                for f in ("arena_off", "kd_off", "u_off"):
                    np.testing.assert_array_equal(getattr(g, f), [0, 0])
                assert len(g.arena) == len(g.key_idx) == len(g.dep_txn) == len(g.kd_key) == 0
    finally:
        s.close()


# ---------------------------------------------------------------- 2. + 5. seeded stores

SEEDS = (22, 46, 54)     # the seeds whose states hold no committed executeAt tie (test_cfk_query_gpu.py)


def foreign_items(ob, seed):
    rng = np.random.default_rng(seed ^ 0xF0)
    codes = np.unique(ob.key_code)
    items = []
    for i in range(20):
        hlc = 2 * int(rng.integers(0, 4 * ob.n_txn + 8)) + 1      # odd: no store TxnId or executeAt (all even)
        tid = ts(hlc, int(rng.choice(CC.KINDS)) << 1, 1 + int(rng.integers(0, 4)))
        ex = ts(hlc + 2 * int(rng.integers(1, 40)), 0, 1 + int(rng.integers(0, 4))) if i % 2 else None
        keys = sorted({7} | set(int(x) for x in rng.choice(codes, size=2, replace=False)))   # 7: no CFK
        items.append((tid, ex, keys, []))
    return items


def foreign_range_items(ob, seed):
    """12 range-domain queries on odd hlcs: ten with one or two ranges whose endpoints come from the grid 90, 95, .. 280
    (the keys are 100, 110, .. 210, so endpoints land on key codes and beside them), one covering no key, one all"""
    rng = np.random.default_rng(seed ^ 0xA5)
    grid = np.arange(90, 281, 5)
    items = []
    for i in range(12):
        hlc = 2 * int(rng.integers(0, 4 * ob.n_txn + 8)) + 1
        tid = ts(hlc, (int(rng.choice(CC.KINDS)) << 1) | RANGE, 1 + int(rng.integers(0, 4)))
        ex = ts(hlc + 2 * int(rng.integers(1, 40)), 0, 1 + int(rng.integers(0, 4))) if i % 2 else None
        if i == 10:
            ranges = [(300, 400)]
        elif i == 11:
            ranges = [(50, 500)]
        else:
            p = sorted(int(x) for x in rng.choice(grid, size=2 * int(rng.integers(1, 3)), replace=False))
            ranges = [(p[j], p[j + 1]) for j in range(0, len(p), 2)]
        items.append((tid, ex, [], ranges))
    return items


def interleave(keys, ranges):
    out, r = [], iter(ranges)
    for i, k in enumerate(keys):
        out.append(k)
        if i % 5 < 3:                 # 20 key queries take 12 range queries between them
            out.append(next(r))
    assert next(r, None) is None
    return out


@pytest.mark.parametrize("end_inclusive", [1, 0], ids=["end_inclusive", "start_inclusive"])
@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_key_and_range_queries(ctx, seed, end_inclusive):
    from accord_amd.deps import CfkStore
    upd = CC.cfk_case(seed, n_txn=200, n_keys=12, keys_per=3)
    n = len(upd["msb"])
    a, rest = CC.split_updates(upd, int(n * 0.4))
    b, d = CC.split_updates(rest, int(n * 0.7) - int(n * 0.4))
    s = CfkStore(ctx)
    try:
        o_state = CC.empty_snapshot()
        for step, part in enumerate((a, b, d)):
            s.apply_deps(part)
            o_state = oracle.cfk_apply(o_state, part)
            assert no_committed_ties(o_state), "seed holds an executeAt tie: pick another"
            ob = CC.snap_as_batch(o_state)[0]
            keys = foreign_items(ob, seed + step)
            items = interleave(keys, foreign_range_items(ob, seed + step))
            want = expect_mixed(ob, items, end_inclusive)
            rq = [i for i, it in enumerate(items) if is_range(it)]
            assert len(rq) == 12 and sum(int(want["u_off"][i + 1] - want["u_off"][i]) for i in rq) > 0
            for lane_seg in (0, 1, NONE):
                g = s.keydeps_mixed(make_mixed(items), end_inclusive, lane_seg)
                assert_result(g, want, f"seed {seed} slice {step} lane_seg {lane_seg}")
            # key-only equivalence: the key queries alone through both entries
            kq = make_mixed(keys)
            g, k = s.keydeps_mixed(kq, end_inclusive), s.keydeps(kq)
            for f in FIELDS + ("kd_key",):
                np.testing.assert_array_equal(getattr(g, f), getattr(k, f), err_msg=f"seed {seed} slice {step} key-only {f}")
    finally:
        s.close()


# ---------------------------------------------------------------- 3. + 4. segment shapes

def segment_stream(codes, lens, accepted_tail):
    """one-key Writes: entry i of key j (codes[j], lens[j] entries) at hlc 4 (i K + j) + 4, so one executeAt cuts every
    segment part-way; the last accepted_tail(L) entries of a key ACCEPTED, the others first seen COMMITTED with
    executeAt = TxnId (distinct TxnIds: no ties)"""
    K = len(codes)
    cols = {k: [] for k in ("msb", "lsb", "node", "xmsb", "xlsb", "xnode", "status", "flags")}
    key = []
    for j, (code, Ln) in enumerate(zip(codes, lens)):
        for i in range(Ln):
            m, l, nd = ts(4 * (i * K + j) + 4)
            st = CC.ACC if i >= Ln - accepted_tail(Ln) else CC.COMMITTED
            for k, v in zip(cols, (m, l, nd, m, l, nd, st, 0)):
                cols[k].append(v)
            key.append(code)
    U = len(key)
    upd = {k: np.array(v, dt) for (k, v), dt in zip(cols.items(), (np.uint64, np.uint64, np.int32, np.uint64, np.uint64,
                                                                  np.int32, np.uint8, np.uint8))}
    upd.update(key_off=np.arange(U + 1, dtype=np.uint32), key=np.array(key, np.uint64), dep_off=np.zeros(U + 1, np.uint32),
               dmsb=np.zeros(0, np.uint64), dlsb=np.zeros(0, np.uint64), dnode=np.zeros(0, np.int32))
    return upd


# around the lane of a wave's 64, the 256-entry chunk and its multiples, and the lane tier's thresholds under test
LADDER = [1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513]


def ladder_case():
    """the store of test_segment_ladder (one key per LADDER length), its txn-major view and the test's queries"""
    K = len(LADDER)
    codes = [1000 + 10 * j for j in range(K)]
    upd = segment_stream(codes, LADDER, lambda Ln: min(10, Ln // 2))
    assert len(upd["key"]) == 1575
    o_state = oracle.cfk_apply(CC.empty_snapshot(), upd)
    assert no_committed_ties(o_state)
    ob = CC.snap_as_batch(o_state)[0]
    top = 4 * (512 * K + K) + 4
    cut = lambda i: 4 * (i * K) + 1                     # noqa: E731  below entry i of every key
    items = [
        (ts(top + 5, WRITE | RANGE), None, [], [(999, 1121)]),                              # everything, above every TxnId
        (ts(cut(40), WRITE | RANGE), None, [], [(1000, 1040), (1060, 1120)]),              # S inside the segments
        (ts(cut(3), ESP | RANGE), ts(cut(260) + 2, 0, 2), [], [(999, 1121)]),              # bumped executeAt
        (ts(cut(70) + 2), None, [1090], []),
        (ts(top + 7), None, [1090, 1120], []),
    ]
    return upd, ob, items


@pytest.mark.parametrize("end_inclusive", [1, 0], ids=["end_inclusive", "start_inclusive"])
def test_segment_ladder(ctx, ctx_small_cap, end_inclusive):
    from accord_amd.deps import CfkStore
    K = len(LADDER)
    upd, ob, items = ladder_case()
    want = expect_mixed(ob, items, end_inclusive)
    assert int(want["u_off"][1]) == 115                 # per key its last committed Write and its accepted tail
    assert int(want["kd_off"][1]) == K
    for c, name in ((ctx, "default cap"), (ctx_small_cap, "small cap")):
        s = CfkStore(c)
        try:
            s.apply_deps(upd)
            for lane_seg in (0, 1, 32, 64, 256, NONE):
                g = s.keydeps_mixed(make_mixed(items), end_inclusive, lane_seg)
                assert_result(g, want, f"ladder {name} lane_seg {lane_seg}")
        finally:
            s.close()


@pytest.mark.parametrize("end_inclusive", [1, 0], ids=["end_inclusive", "start_inclusive"])
def test_many_short_segments(ctx, end_inclusive):
    """130 keys of 1..3 entries: ranges around the 64 lanes of a wave and the piece boundaries of the expansion"""
    from accord_amd.deps import CfkStore
    K = 130
    codes = [2000 + 10 * j for j in range(K)]
    lens = [1 + j % 3 for j in range(K)]
    upd = segment_stream(codes, lens, lambda Ln: 1 if Ln >= 2 else 0)
    o_state = oracle.cfk_apply(CC.empty_snapshot(), upd)
    assert no_committed_ties(o_state)
    ob = CC.snap_as_batch(o_state)[0]
    top = 4 * (3 * K) + 4
    cv = lambda j0, j1: cover(codes, j0, j1, end_inclusive)   # noqa: E731
    items = []
    for h, (j0, j1) in enumerate([(0, 63), (0, 64), (0, 65), (0, 128), (0, 129), (0, 130), (37, 107)]):
        items.append((ts(top + 1 + 2 * h, WRITE | RANGE), None, [], [cv(j0, j1)]))             # above every TxnId
        items.append((ts(4 * K + 1 + 2 * h, ESP | RANGE, 2), None, [], [cv(j0, j1)]))           # around entry 1 of every key
    # three ranges, the first two touch at 2635: keys 0..63, key 64, keys 66..129
    items.append((ts(top + 31, WRITE | RANGE), None, [], [(cv(0, 64)[0], 2635), (2635, cv(64, 65)[1]), cv(66, 130)]))
    items.append((ts(top + 33), None, [2000, 2005, 2640], []))
    want = expect_mixed(ob, items, end_inclusive)
    assert [int(x) for x in np.diff(want["kd_off"])[0:12:2]] == [63, 64, 65, 128, 129, 130]
    s = CfkStore(ctx)
    try:
        s.apply_deps(upd)
        for lane_seg in (0, 1, 2, 3, NONE):
            g = s.keydeps_mixed(make_mixed(items), end_inclusive, lane_seg)
            assert_result(g, want, f"short segments lane_seg {lane_seg}")
    finally:
        s.close()


# ---------------------------------------------------------------- 6. steady-state chain

FOREIGN_NODE = 77     # no txn of the stream comes from this node, so no stored executeAt equals a range query's timestamp


@pytest.mark.parametrize("dist", ["uniform", "zipf"])
def test_steady_state_with_range_queries(ctx, dist):
    from accord_amd.deps import ReplicaStore
    u = W.cfk_update_stream(6_000, 4, 800, dist=dist, window=600)
    assert not np.any(u["node"] == FOREIGN_NODE) and not np.any(u["xnode"] == FOREIGN_NODE)
    nb = 4
    cuts = W.cfk_stream_cuts(u, 3_000, 500, nb)
    rs = ReplicaStore(ctx)
    rng = np.random.default_rng(0x5EED)
    try:
        init = W.cfk_slice(u, 0, cuts[0])
        rs.preaccept_batch(init, scan=False)
        o_state = oracle.cfk_apply(CC.empty_snapshot(), init)
        range_edges = 0
        for b in range(nb):
            part = W.cfk_slice(u, cuts[b], cuts[b + 1])
            q = W.preaccept_queries(part)
            assert len(q["msb"]) == 500
            o_state = oracle.cfk_apply(o_state, part)
            ob = CC.snap_as_batch(o_state)[0]
            codes = o_state["key"]
            # 20 foreign range txns: a stored TxnId's time from another node, a run of 1..40 store keys (or none: below them)
            ritems = []
            for i in range(20):
                t = int(rng.integers(0, ob.n_txn))
                kind = int(rng.choice(CC.KINDS))
                tid = (int(ob.txn_msb[t]), (int(ob.txn_lsb[t]) & 0xFFFFFFFFFFFF0000) | (kind << 1) | RANGE, FOREIGN_NODE)
                j0 = int(rng.integers(1, len(codes) - 40))
                ranges = [(0, int(codes[0]) - 1)] if i == 7 and int(codes[0]) > 1 else \
                    [(int(codes[j0]) - 1, int(codes[j0 + int(rng.integers(1, 41)) - 1]))]
                ritems.append((tid, None, [], ranges))
            stored = set(zip((int(x) for x in o_state["xmsb"]), (int(x) & 0xFFFFFFFFFFFF001E for x in o_state["xlsb"]),
                             (int(x) for x in o_state["xnode"])))
            assert not any((t[0], t[1] & 0xFFFFFFFFFFFF001E, t[2]) in stored for t, _, _, _ in ritems)
            rq = make_mixed(ritems)
            both = dict(msb=np.concatenate([q["msb"], rq["msb"]]), lsb=np.concatenate([q["lsb"], rq["lsb"]]),
                        node=np.concatenate([q["node"], rq["node"]]),
                        is_range=np.concatenate([q["is_range"], np.ones(20, np.uint8)]),
                        part_off=np.concatenate([q["part_off"], q["part_off"][-1] + rq["rng_off"][1:]]).astype(np.uint32),
                        part_start=np.concatenate([q["part_start"], rq["rng_start"]]),
                        part_end=np.concatenate([q["part_end"], rq["rng_end"]]))
            r = rs.preaccept_batch(part, both, scan="new")
            index = {(int(m), int(l) & 0xFFFFFFFFFFFF001E, int(nd)): t
                     for t, (m, l, nd) in enumerate(zip(ob.txn_msb, ob.txn_lsb, ob.txn_node))}
            new = [index[(int(m), int(l) & 0xFFFFFFFFFFFF001E, int(nd))] for m, l, nd in zip(q["msb"], q["lsb"], q["node"])]
            ok = oracle.keydeps_batch(ob, queries=new)
            krows = []
            for t in new:
                k, d, a = ok.txn(t)
                krows.append((k, d, a, ob.key_code[int(ob.key_off[t]):int(ob.key_off[t + 1])][k.astype(np.int64)]))
            rrows = range_rows(ob, ritems, rs.end_inclusive)
            assert_result(r["keydeps_new"], join_rows(krows + rrows), f"{dist} batch {b}")
            range_edges += sum(len(p[1]) for p in rrows)
            # the query neither modified the store nor wrote into the buffers the next update adopts
            g_state = rs.cfk.state()
            for k in o_state:
                np.testing.assert_array_equal(np.asarray(g_state[k]), np.asarray(o_state[k]), err_msg=f"{dist} batch {b} state {k}")
        assert range_edges
    finally:
        rs.close()


# ---------------------------------------------------------------- 7. errors and edges

def test_errors_and_edges(ctx):
    from accord_amd.deps import CfkStore, IllegalArgumentException, IllegalStateException
    upd, _ = CC.handmade()
    s = CfkStore(ctx)
    empty = CfkStore(ctx)
    status_only = CfkStore(ctx)
    R16 = ts(16, WRITE | RANGE)
    try:
        s.apply_deps(upd)
        good = make_mixed([(ts(16), None, [500], []), (R16, None, [], [(400, 600)])])

        def check_good():
            g = s.keydeps_mixed(good)
            np.testing.assert_array_equal(g.arena, [3, 0, 1, 3, 0, 1])
            np.testing.assert_array_equal(g.dep_txn, [1, 2, 1, 2])
            np.testing.assert_array_equal(g.kd_key, [500, 500])

        def rejected(q, exc=IllegalArgumentException, **kw):
            with pytest.raises(exc):
                s.keydeps_mixed(q, **kw)
            check_good()

        check_good()
        rejected(make_mixed([(R16, None, [500], [(400, 600)])]))                           # a range-domain query lists keys
        rejected(make_mixed([(ts(16), None, [500], [(400, 600)])]))                        # a key-domain query lists ranges
        rejected(make_mixed([(R16, None, [], [(600, 600)])]))                              # start == end
        rejected(make_mixed([(R16, None, [], [(600, 400)])]))                              # start > end
        rejected(make_mixed([(R16, None, [], [(550, 600), (400, 500)])]))                  # out of order
        rejected(make_mixed([(R16, None, [], [(400, 500), (499, 600)])]))                  # overlapping
        rejected(dict(good, rng_off=np.array([1, 1, 1], np.uint32)))                       # rng_off does not start at 0
        rejected(dict(good, rng_off=np.array([0, 1, 0], np.uint32)))                       # rng_off decreases
        rejected(dict(good, rng_off=np.array([0, 0, 0], np.uint32)))                       # rng_off ends off n_ranges
        rejected(dict(good, key_off=np.array([1, 1, 1], np.uint32)))                       # key_off does not start at 0
        rejected(make_mixed([(ts(16), None, [501, 500], [])]))                             # unsorted keys
        rejected(make_mixed([(ts(16, 7 << 1 | RANGE), None, [], [(400, 600)])]))           # Kind.ofOrdinal
        rejected(make_mixed([(ts(16, 5 << 1 | RANGE), None, [], [(400, 600)])]), IllegalStateException)   # LocalOnly
        rejected(good, end_inclusive=2)
        rejected(good, lane_seg=257)
        g = s.keydeps_mixed(make_mixed([(R16, None, [], [(400, 500), (500, 600)])]))       # touching ranges are allowed
        np.testing.assert_array_equal(g.dep_txn, [1, 2])
        np.testing.assert_array_equal(s.keydeps_mixed(good, lane_seg=256).dep_txn, [1, 2, 1, 2])

        status_only.update(W.keydeps_batch(50, 2, 10, 7, "uniform"))
        with pytest.raises(IllegalStateException):
            status_only.keydeps_mixed(good)

        for st in (empty, s):
            g = st.keydeps_mixed(make_mixed([]))                                           # n_query = 0
            for f in ("arena_off", "kd_off", "u_off"):
                np.testing.assert_array_equal(getattr(g, f), [0])
            assert len(g.arena) == len(g.key_idx) == len(g.dep_txn) == 0
        g = empty.keydeps_mixed(good)                                                      # empty store
        for f in ("arena_off", "kd_off", "u_off"):
            np.testing.assert_array_equal(getattr(g, f), [0, 0, 0])
        # a range query with zero ranges, ranges that cover nothing, and one that does, in one call
        g = s.keydeps_mixed(make_mixed([(R16, None, [], []), (R16, None, [], [(1, 499), (500, 900)]), (R16, None, [], [(499, 500)])]))
        np.testing.assert_array_equal(g.arena_off, [0, 0, 0, 3])
        np.testing.assert_array_equal(g.kd_off, [0, 0, 0, 1])
        np.testing.assert_array_equal(g.u_off, [0, 0, 0, 2])
        np.testing.assert_array_equal(g.dep_txn, [1, 2])
        q = {k: v for k, v in good.items() if k not in ("xmsb", "xlsb", "xnode")}          # no executeAt columns
        np.testing.assert_array_equal(s.keydeps_mixed(q).dep_txn, [1, 2, 1, 2])
        check_good()
    finally:
        s.close()
        empty.close()
        status_only.close()


def test_tie_rule_in_the_lane_tier(ctx):
    """two committed entries of one key executing at one timestamp: a range query whose executeAt is that timestamp
    fails with IllegalStateException from the lane tier and from the chunk path alike; any other one is answered"""
    from accord_amd.deps import CfkStore, IllegalStateException
    x = ts(20, 0, 1)
    cols = {k: [] for k in ("msb", "lsb", "node", "xmsb", "xlsb", "xnode", "status", "flags")}
    for h in (4, 8):
        m, l, nd = ts(h)
        for k, v in zip(cols, (m, l, nd, x[0], x[1], x[2], CC.COMMITTED, 0)):
            cols[k].append(v)
    upd = {k: np.array(v, dt) for (k, v), dt in zip(cols.items(), (np.uint64, np.uint64, np.int32, np.uint64, np.uint64,
                                                                  np.int32, np.uint8, np.uint8))}
    upd.update(key_off=np.array([0, 1, 2], np.uint32), key=np.array([500, 500], np.uint64), dep_off=np.zeros(3, np.uint32),
               dmsb=np.zeros(0, np.uint64), dlsb=np.zeros(0, np.uint64), dnode=np.zeros(0, np.int32))
    s = CfkStore(ctx)
    try:
        s.apply_deps(upd)
        for lane_seg in (0, 1, NONE):
            with pytest.raises(IllegalStateException):
                s.keydeps_mixed(make_mixed([(ts(12, WRITE | RANGE), x, [], [(499, 500)])]), 1, lane_seg)
            g = s.keydeps_mixed(make_mixed([(ts(12, WRITE | RANGE), ts(22, 0, 1), [], [(499, 500)])]), 1, lane_seg)
            np.testing.assert_array_equal(g.dep_txn, [0, 1])
    finally:
        s.close()
