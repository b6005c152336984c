"""GPU parity for acc_rcmd_redundant_before / acc_rcmd_redundant_view (RangeCmdStore.redundant_before / redundant_map,
ReplicaStore.mark_shard_durable): the resident range-command store pruned as InMemoryCommandStore.markShardDurable
prunes rangeCommands (impl/InMemoryCommandStore.java:346-370), and its updates registering only what the map leaves
(:757-760).

Expected values come from rcmd_redundant_model.RedundantModel (pinned against Ranges.subtract in
test_rcmd_redundant_model.py). After every step every table column with the dictionary, every state column, the map and
the stats are compared; after every prune also rangedeps of a query batch (test_rcmd_gpu.expect_rangedeps over the
model's table) and the four BeginRecovery scans (rcmd_state_model.check_scan). Every comparison is exact. The stream's
seeds were chosen on the host model alone (stream_steps asserts what it must exercise)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import rcmd_redundant_model as RM
import rcmd_state_model as M
from accord_amd import _lib as L
from accord_amd import workload as W
from accord_amd.deps import (Context, IllegalArgumentException, RangeCmdStore, ReplicaStore, device_array,
                             mixed_queries_from_preaccept)
from cfk_redundant_model import order, ranges_of
from test_rcmd_gpu import assert_rd, conflicts_of, expect_rangedeps, queries, ts, updates
from test_rcmd_recovery_gpu import cmd_updates, rq

pytestmark = pytest.mark.gpu

ERASED, HAS_DEPS, KEEP_DEPS = L.ACC_RCMD_ERASED, L.ACC_RCMD_HAS_DEPS, L.ACC_RCMD_KEEP_DEPS
BEGIN_RECOVERY = list(L.RECOVERY_SCANS.values())
FLAG = 0x20      # an lsb bit outside Timestamp.IDENTITY_LSB


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def check(ctx, s, m, msg, op=None):
    """table, state and map of the store against the model; the stats of the call just made"""
    tab, _ = M.assert_store(s, m, msg)
    RM.assert_map(s, m, msg)
    st = ctx.stats()
    if op == "update":
        for k, v in m.stats.items():
            assert st["rcmd." + k] == v, (msg, k)
        assert st["rcmd.update_ranges_trimmed"] == m.trimmed, msg
        assert st["rcmd.entries"] == len(tab["rng_start"]) and st["rcmd.stored_ranges"] == len(tab["dict_start"]), msg
    if op == "mark":
        for k, v in m.rstats.items():
            assert st["rcmd.redundant_" + k] == v, (msg, k, st["rcmd.redundant_" + k], v)
    return tab


def feed(ctx, s, m, upd, msg):
    s.update(upd)
    m.apply(upd)
    return check(ctx, s, m, msg, "update")


def mark(ctx, s, m, ranges, msg):
    s.redundant_before(ranges)
    m.mark(ranges)
    return check(ctx, s, m, msg, "mark")


def check_reads(s, m, q, recq, msg):
    """rangedeps of q and the four BeginRecovery scans of recq over the pruned state"""
    g = s.rangedeps(q)
    assert_rd(g, expect_rangedeps(m.table(), q, m.ei), msg)
    cmds = m.cmds()
    hits = int((np.diff(g.u_off.astype(np.int64)) > 0).sum())
    for params in BEGIN_RECOVERY:
        hits += sum(1 for d in M.check_scan(s, cmds, recq, params, msg=msg) if d)
    return hits


def assert_invariant(tab, m, msg):
    """no stored range of a non-erased row intersects a map interval whose bound is above the row's TxnId"""
    from bisect import bisect_left
    keys = [order(t) for t in zip(tab["msb"], tab["lsb"], tab["node"])]
    assert keys == sorted(keys), msg
    row = np.repeat(np.arange(len(keys)), np.diff(tab["rng_off"].astype(np.int64)))
    live = (tab["flags"][row] & ERASED) == 0
    for (s, e), v in m.raw_intervals():
        below = row < bisect_left(keys, v)            # the rows whose TxnId is below the bound (the table is sorted)
        hit = below & live & (tab["rng_start"] < np.uint64(e)) & (tab["rng_end"] > np.uint64(s))
        assert not hit.any(), (msg, (s, e), np.flatnonzero(hit)[:5])


def key_dep(t, key):
    return (t, key, 0, 1)


# ---------------------------------------------------------------- 1. the hand-worked store

def hand_worked():
    """Ten commands and one call of five ranges (read [s, e) or (s, e] by the bound type; the arithmetic is the same):
         [10, 20) bound hlc 100 node 1 | [20, 30) bound hlc 50 | [40, 45) bound hlc 100 node 2 (with a bit outside
         compareTo) | [50, 55) bound hlc 100 node -3 | [70, 80) bound hlc 300
       row TxnId            ranges                      after
       0   hlc 5            [12, 18)                    inside [10, 20): dropped (the first row)
       1   hlc 6  erased    -                           a tombstone below every bound: kept
       2   hlc 10           [5, 15) [25, 35) [38, 60)   [5, 10) (tail) [30, 35) (head) [38, 40) [45, 50) [55, 60) (3 pieces)
       3   hlc 20 deps x2   [21, 29)                    inside [20, 30): dropped with its deps
       4   hlc 30           none                        below a bound, no ranges: dropped
       5   hlc 60 deps x1   [15, 25)                    between the bounds of the touching [10, 20) and [20, 30): [20, 25);
                                                        its deps span moves from 2 to 0
       6   hlc 100 node 0   [40, 52)                    below node 2's bound, above node -3's: [45, 52)
       7   hlc 100 node 1   [11, 13)                    equal to the bound of [10, 20): stays
       8   hlc 100 node 2   [41, 44)                    equal but for a bit outside compareTo: stays
       9   hlc 200          [72, 75)                    inside [70, 80): dropped (the last row)"""
    W_ = W.WRITE
    d = [key_dep(ts(1), 7), key_dep(ts(2), 8)]
    items = [
        (ts(5), 0, [(12, 18)], 1, None, []), (ts(6), ERASED, [], 1, None, []),
        (ts(10), 0, [(5, 15), (25, 35), (38, 60)], 2, None, []),
        (ts(20), HAS_DEPS, [(21, 29)], 3, ts(21), d), (ts(30), 0, [], 1, None, []),
        (ts(60), HAS_DEPS, [(15, 25)], 5, ts(61), [key_dep(ts(3), 9)]),
        (ts(100, W_, node=0), 0, [(40, 52)], 1, None, []), (ts(100, W_, node=1), 0, [(11, 13)], 1, None, []),
        (ts(100, W_, node=2), 0, [(41, 44)], 1, None, []), (ts(200), 0, [(72, 75)], 1, None, []),
    ]
    call = ranges_of([(10, 20, ts(100, W_, node=1)), (20, 30, ts(50)), (40, 45, ts(100, W_, node=2, extra=FLAG)),
                      (50, 55, ts(100, W_, node=-3)), (70, 80, ts(300))])
    lower = ranges_of([(10, 20, ts(40)), (20, 30, ts(10)), (70, 80, ts(150))])
    after = [[], [(5, 10), (30, 35), (38, 40), (45, 50), (55, 60)], [(20, 25)], [(45, 52)], [(11, 13)], [(41, 44)]]
    return items, call, lower, after


def read_queries():
    q = queries([(ts(500, W.WRITE, rng=0), None, [5, 9, 12, 22, 31, 39, 47, 51, 58], []),
                 (ts(501, W.WRITE), None, [], [(0, 100)]), (ts(55, W.WRITE), None, [], [(0, 100)]),
                 (ts(502, W.EXCLUSIVE_SYNC_POINT), None, [], [(18, 22), (44, 46)])])
    recq = M.domain_queries(rq([(ts(55, W.WRITE), None, [(0, 100)]), (ts(1, W.WRITE, rng=0), [9, 22, 47], None),
                                (ts(400, W.WRITE), None, [(0, 100)])]))
    return q, recq


@pytest.mark.parametrize("ei", [0, 1])
def test_hand_worked_store(ctx, ei):
    items, call, lower, after = hand_worked()
    q, recq = read_queries()
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    try:
        assert len(s.redundant_map()["st"]) == 0
        feed(ctx, s, m, cmd_updates(items), "fill")
        tab = mark(ctx, s, m, call, "the call")
        off = tab["rng_off"].tolist()
        rows = [list(zip(tab["rng_start"][a:b].tolist(), tab["rng_end"][a:b].tolist())) for a, b in zip(off, off[1:])]
        assert rows == after
        assert tab["flags"].tolist() == [ERASED, 0, HAS_DEPS, 0, 0, 0]
        assert [int(x) >> 16 for x in tab["lsb"]] == [6, 10, 60, 100, 100, 100] and tab["node"].tolist() == [1, 1, 1, 0, 1, 2]
        st = s.state()
        assert st["dep_off"].tolist() == [0, 0, 0, 1, 1, 1, 1] and st["dep_start"].tolist() == [9]
        assert st["status"].tolist() == [1, 2, 5, 1, 1, 1] and int(st["xlsb"][2]) >> 16 == 61
        assert m.rstats == dict(cmds_cut=3, cmds_dropped=4, ranges_before=10, ranges_after=9)
        assert {"cut_head", "cut_tail", "cut_middle_3_pieces", "covered_whole_range", "dropped_first_row", "dropped_last_row",
                "dropped_with_deps", "dropped_already_empty", "equal_bound_stays", "touching_ranges_different_bounds",
                "tombstone_kept"} <= m.seen
        assert check_reads(s, m, q, recq, "after the call") > 0
        # lower bounds are absorbed: nothing is rewritten, and earlier views still read the same data
        v, sv = s.view(), s.state_view()
        before_map = s.redundant_map()
        old = (device_array(ctx, v.rng_start, int(v.n_ranges), np.uint64), device_array(ctx, sv.dep_start, int(sv.n_deps), np.uint64))
        tab2 = mark(ctx, s, m, lower, "lower bounds")
        assert {"noop_call", "lower_bound_absorbed"} <= m.seen
        v2, sv2 = s.view(), s.state_view()
        for a, b in ((v.txn_id.msb, v2.txn_id.msb), (v.rng_off, v2.rng_off), (v.rng_start, v2.rng_start), (v.dict_start, v2.dict_start),
                     (sv.dep_off, sv2.dep_off), (sv.dep_start, sv2.dep_start), (sv.status, sv2.status)):
            assert C.cast(a, C.c_void_p).value == C.cast(b, C.c_void_p).value, "an array moved"
        np.testing.assert_array_equal(device_array(ctx, v.rng_start, int(v.n_ranges), np.uint64), old[0])
        np.testing.assert_array_equal(device_array(ctx, sv.dep_start, int(sv.n_deps), np.uint64), old[1])
        np.testing.assert_array_equal(tab2["rng_start"], tab["rng_start"])
        after_map = s.redundant_map()
        for k in ("st", "en", "msb", "lsb", "node"):
            np.testing.assert_array_equal(after_map[k], before_map[k], err_msg=k)
        check_reads(s, m, q, recq, "after the absorbed call")
    finally:
        s.close()


# ---------------------------------------------------------------- 2. registration under the map

@pytest.mark.parametrize("ei", [0, 1])
def test_registration_under_the_map(ctx, ei):
    """The map first, on an empty store: [2, 3) bound hlc 100, [10, 20) bound hlc 50. The header's order-dependent family
    then folds on trimmed pieces: below hlc 100, [1, 3) -> [1, 2), [3, 5) stays, [2, 4) -> [3, 4); so A ([1,3) [3,5) [2,4))
    and B ([1,3) [2,4) [3,5)) both end as {[1, 2), [3, 5)}, while the same updates of TxnIds above the bound give
    {[1,3), [3,5)} and {[1,5)}."""
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    q, recq = read_queries()
    try:
        mark(ctx, s, m, ranges_of([(2, 3, ts(100)), (10, 20, ts(50))]), "marked while empty")
        assert len(s.table()["msb"]) == 0 and len(s.redundant_map()["st"]) == 2
        A, B, A2, B2 = ts(10), ts(11), ts(110), ts(111)
        fam = [(A, 0, [(1, 3)]), (B, 0, [(1, 3)]), (A2, 0, [(1, 3)]), (B2, 0, [(1, 3)]),
               (A, 0, [(3, 5)]), (B, 0, [(2, 4)]), (A2, 0, [(3, 5)]), (B2, 0, [(2, 4)]),
               (A, 0, [(2, 4)]), (B, 0, [(3, 5)]), (A2, 0, [(2, 4)]), (B2, 0, [(3, 5)]),
               (ts(20), 0, [(12, 18)]),                       # trimmed to nothing: inserted without ranges
               (ts(30), ERASED, [(2, 3)]),                    # an erasing update: its ranges are not read
               (ts(40, rng=0), 0, [(2, 3)]),                  # a key-domain TxnId: skipped
               (ts(60), 0, [(12, 18)]), (ts(61), 0, [(0, 5)])]   # above hlc 50: [12, 18) stays; below hlc 100: [0, 2) [3, 5)
        tab = feed(ctx, s, m, updates(fam), "plain update")
        off = tab["rng_off"].tolist()
        rows = [list(zip(tab["rng_start"][a:b].tolist(), tab["rng_end"][a:b].tolist())) for a, b in zip(off, off[1:])]
        assert rows == [[(1, 2), (3, 5)], [(1, 2), (3, 5)], [], [], [(12, 18)], [(0, 2), (3, 5)], [(1, 3), (3, 5)], [(1, 5)]]
        assert ctx.stats()["rcmd.update_ranges_trimmed"] == 6 and ctx.stats()["rcmd.skipped_key_domain"] == 1
        assert {"trim_partial", "trim_to_nothing_inserted_empty", "in_batch_repeat"} <= m.seen
        d = [key_dep(ts(1), 7), ((ts(2)), 3, 9, 0)]
        batch = [(ts(45), HAS_DEPS, [(0, 30)], 3, ts(46), d),                  # [0, 2) [3, 10) [20, 30)
                 (ts(20), 0, [(8, 22)], 2, None, []),                          # the empty command: [8, 10) [20, 22)
                 (ts(20), KEEP_DEPS, [(9, 12), (15, 21)], 4, None, []),        # [9, 10) [20, 21): a superset short-cut on pieces
                 (ts(10), ERASED, [(1, 2)], 9, None, []), (ts(10), 0, [(50, 60)], 1, None, []),   # erased, then ignored
                 (ts(70, rng=0), 0, [(2, 3)], 1, None, []),
                 (ts(120), HAS_DEPS, [(0, 30)], 7, ts(130), d[:1])]            # above every bound: as given
        feed(ctx, s, m, cmd_updates(batch), "update_cmds")
        assert ctx.stats()["rcmd.update_ranges_trimmed"] == 4 and ctx.stats()["rcmd.erased_ignored"] == 1
        assert_invariant(s.table(), m, "registration")
        assert check_reads(s, m, q, recq, "registration") > 0
        # a prune above hlc 20: the command that was inserted empty and refilled loses what [0, 25) covers and leaves
        mark(ctx, s, m, ranges_of([(0, 25, ts(25))]), "prune after registration")
        assert ts(20)[1] not in s.table()["lsb"].tolist() and ts(10)[1] in s.table()["lsb"].tolist()
        check_reads(s, m, q, recq, "prune after registration")
    finally:
        s.close()


# ---------------------------------------------------------------- 3. a chained random stream

SPACE = 4000
STREAM_SEED = {0: 1, 1: 1}


def rand_ranges(rng, kmax=3, wide=0.35):
    k = int(rng.integers(0, kmax + 1))
    out, lo = [], int(rng.integers(0, SPACE // 2))
    for _ in range(k):
        w = int(rng.integers(300, 1500)) if rng.random() < wide else int(rng.integers(1, 60))
        if lo + w >= SPACE:
            break
        out.append((lo, lo + w))
        lo += w + int(rng.integers(0, 400))
    return out


@functools.lru_cache(maxsize=None)
def stream_steps(seed, ei):
    """12 steps: update_cmds batches of about 200 alternating with prunes, TxnIds drawn around the moving bounds (hlc
    1000 (p + 1) for prune p). Prune 0 covers the key space above every stored TxnId (no row is erased yet: the store
    empties); prune 3 repeats prune 2's ranges with lower bounds. Built with a scratch model, which also picks, for
    some bounds, the raw TxnId of a stored command (a TxnId equal to a bound)."""
    rng = np.random.default_rng(seed * 1009 + ei)
    m = RM.RedundantModel(ei)
    kinds = [W.READ, W.WRITE, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT]
    steps, prev = [], None
    for p in range(6):
        lo, hi = (100, 900) if p == 0 else (1000 * p - 400, 1000 * p + 1600)
        ids = [ts(int(h), kinds[int(rng.integers(4))], node=int(rng.integers(1, 4))) for h in rng.integers(lo, hi, size=150)]
        items = []
        for _ in range(200):
            t = ids[int(rng.integers(len(ids)))]
            u = rng.random()
            if u < 0.04:
                t = (t[0], t[1] & ~1, t[2])
            fl = ERASED if (0.04 <= u < 0.10 and p > 0) else int(rng.choice([0, HAS_DEPS, HAS_DEPS, KEEP_DEPS]))
            nd = 0 if fl & (ERASED | KEEP_DEPS) else int(rng.integers(0, 4))
            deps = sorted((key_dep(ts(int(h)), int(rng.integers(SPACE))) for h in rng.integers(1, 50, size=nd)), key=lambda d: order(d[0]))
            items.append((t, fl, rand_ranges(rng), int(rng.integers(0, 11)), None, deps))
        upd = cmd_updates(items)
        m.apply(upd)
        steps.append(("update", upd))
        b = 1000 * (p + 1)
        if p == 0:
            call = [(0, SPACE, ts(b))]
        elif p == 3:
            call = [(s, e, ts(b - 2500, node=int(rng.integers(1, 4)))) for s, e, _ in prev]
        else:
            live = [c[0] for c in m.cmd.values() if not c[1] and c[2] is not None and len(c[2])]
            call, at = [], int(rng.integers(0, 300))
            while at < SPACE - 200:
                w = int(rng.integers(20, 260))
                bound = ts(b - int(rng.choice([0, 400, 900])), node=int(rng.integers(1, 4)))
                if live and rng.random() < 0.25:
                    bound = live[int(rng.integers(len(live)))]
                call.append((at, at + w, bound))
                at += w + (0 if rng.random() < 0.4 else int(rng.integers(1, 500)))
        prev = call
        r = ranges_of(call)
        m.mark(r)
        steps.append(("mark", r))
    assert m.seen >= RM.TAGS, sorted(RM.TAGS - m.seen)
    return steps


def stream_queries(rng, n):
    items = []
    for i in range(n):
        kind = [W.WRITE, W.READ, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT][i % 4]
        t = ts(int(rng.integers(100, 8000)), kind, node=int(rng.integers(1, 5)), rng=i % 2)
        if i % 2:
            a = int(rng.integers(0, SPACE - 700))
            items.append((t, None, [], [(a, a + int(rng.integers(1, 600)))]))
        else:
            items.append((t, None, sorted(int(x) for x in rng.choice(SPACE, size=3, replace=False)), []))
    return items


@pytest.mark.parametrize("ei", [0, 1])
def test_chained_random_stream(ctx, ei):
    steps = stream_steps(STREAM_SEED[ei], ei)
    rng = np.random.default_rng(77 + ei)
    qi = stream_queries(rng, 120)
    q = queries(qi)
    recq = M.domain_queries(rq([(t, k, r) for t, _, k, r in qi[:40]]))
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    hits = 0
    try:
        for i, (op, arg) in enumerate(steps):
            if op == "update":
                tab = feed(ctx, s, m, arg, f"step {i} update")
            else:
                tab = mark(ctx, s, m, arg, f"step {i} mark")
                hits += check_reads(s, m, q, recq, f"step {i} mark")
            assert_invariant(tab, m, f"step {i}")
        assert m.seen >= RM.TAGS, sorted(RM.TAGS - m.seen)
        assert hits > 0
    finally:
        s.close()


# ---------------------------------------------------------------- 4. past one block and one scan tile

@pytest.mark.parametrize("ei", [0, 1])
def test_past_one_block_and_scan_tile(ctx, ei):
    """10,000 commands, 25,000 ranges, 30,000 deps and 600 input ranges: more than BLOCK (256) and than one k_scan_1p
    tile (4,096 u64 / 8,192 u32 elements) of each. Input range j = [100 j + 20, 100 j + 70) with bound hlc 3,000 /
    7,000 / 20,000 by j mod 3 (the commands are hlc 1,000 .. 10,999), so every block of rows and of ranges holds rows
    that are cut, rows that are dropped (every fifth command holds one narrow range inside a range of the highest
    bound) and rows that stay."""
    N, NJ = 10_000, 600
    dd = [key_dep(ts(1 + j), 100 + j) for j in range(3)]
    items = []
    for i in range(N):
        a = (i * 37) % 59_000
        if i % 5 == 4:
            j = 3 * ((i * 7) % (NJ // 3)) + 2
            rr = [(100 * j + 30, 100 * j + 40)]
        else:
            rr = [(a, a + 150), (a + 200, a + 230), (a + 300, a + 420)]
        items.append((ts(1000 + i, node=1 + i % 3), HAS_DEPS, rr, i % 11, None, dd))
    call = ranges_of([(100 * j + 20, 100 * j + 70, ts((3000, 7000, 20000)[j % 3])) for j in range(NJ)])
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    try:
        tab = feed(ctx, s, m, cmd_updates(items), "fill")
        assert len(tab["msb"]) == N and len(tab["rng_start"]) >= 25_000 and len(s.state()["dep_msb"]) == 30_000
        tab = mark(ctx, s, m, call, "the prune")
        assert m.rstats["cmds_dropped"] == N // 5 and m.rstats["cmds_cut"] > 4000
        assert len(s.redundant_map()["st"]) == NJ
        # dropped and cut rows in every block of 256 old rows
        kept = {int(x) >> 16 for x in tab["lsb"]}
        assert all(any(1000 + r not in kept for r in range(b, b + 256)) for b in range(0, N - 256, 256))
        late = [(ts(500 + 40 * i, node=2), HAS_DEPS, [(150 * i, 150 * i + 400)], 3, None, dd[:1]) for i in range(200)]
        late += [(ts(1000 + 7 * i, node=1 + (7 * i) % 3), KEEP_DEPS, [(97 * i, 97 * i + 300)], 5, None, []) for i in range(200)]
        feed(ctx, s, m, cmd_updates(late), "the update after it")
        assert m.trimmed > 256
        assert_invariant(s.table(), m, "multi-tile")
        rng = np.random.default_rng(5)
        qi = []
        for i in range(200):
            t = ts(int(rng.integers(500, 12000)), [W.WRITE, W.READ, W.EXCLUSIVE_SYNC_POINT][i % 3], node=4, rng=i % 2)
            a = int(rng.integers(0, 59_000))
            qi.append((t, None, [], [(a, a + int(rng.integers(1, 300)))]) if i % 2 else (t, None, [a, a + 33, a + 260], []))
        recq = M.domain_queries(rq([(t, k, r) for t, _, k, r in qi[:40]]))
        assert check_reads(s, m, queries(qi), recq, "multi-tile") > 100
    finally:
        s.close()


# ---------------------------------------------------------------- 5. empties and errors

def snapshot(s):
    return s.table(), s.state(), s.redundant_map()


def assert_unchanged(s, snap, msg):
    tab, st, mp = s.table(), s.state(), s.redundant_map()
    for got, want in zip((tab, st, mp), snap):
        for k, v in want.items():
            np.testing.assert_array_equal(got[k], v, err_msg=f"{msg}: {k}")


def raw_call(ctx, s, ranges, **over):
    a = dict(rs=np.ascontiguousarray(ranges["rng_start"], dtype=np.uint64), re=np.ascontiguousarray(ranges["rng_end"], dtype=np.uint64),
             bm=np.ascontiguousarray(ranges["msb"], dtype=np.uint64), bl=np.ascontiguousarray(ranges["lsb"], dtype=np.uint64),
             bn=np.ascontiguousarray(ranges["node"], dtype=np.int32))
    p = lambda k: a[k].ctypes.data  # noqa: E731
    f = dict(mem=L.ACC_MEM_HOST, n_ranges=len(a["rs"]), end_inclusive=s.end_inclusive)
    f.update(over)
    ri = L.CfkRedundantIn(f["mem"], f["n_ranges"], f["end_inclusive"], p("rs"), p("re"), L.TsCols(p("bm"), p("bl"), p("bn")))
    return ctx._lib.acc_rcmd_redundant_before(ctx.handle, s._h, C.byref(ri))


def test_empties_and_errors(ctx):
    ei = 0
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    q, recq = read_queries()
    try:
        # an empty store: no-op calls, a prune, rejected calls
        mark(ctx, s, m, ranges_of([]), "n_ranges == 0 on an empty store")
        assert len(s.redundant_map()["st"]) == 0
        with pytest.raises(IllegalArgumentException):
            s.redundant_before(ranges_of([(5, 5, ts(9))]))
        assert len(s.redundant_map()["st"]) == 0, "a rejected first call leaves the store without a map"
        mark(ctx, s, m, ranges_of([(90, 95, ts(9))]), "a prune of an empty store")
        items, call, _, _ = hand_worked()
        feed(ctx, s, m, cmd_updates(items), "fill")
        snap = snapshot(s)
        good = ranges_of([(10, 20, ts(100)), (20, 30, ts(100))])
        for name, bad in (("unsorted", [(20, 30, ts(100)), (10, 20, ts(100))]), ("overlapping", [(10, 21, ts(100)), (20, 30, ts(100))]),
                          ("start == end", [(10, 10, ts(100))]), ("start > end", [(10, 20, ts(100)), (40, 30, ts(100))])):
            with pytest.raises(IllegalArgumentException):
                s.redundant_before(ranges_of(bad))
            assert_unchanged(s, snap, name)
        assert raw_call(ctx, s, good, mem=7) == L.ACC_E_ARG
        assert raw_call(ctx, s, good, end_inclusive=2) == L.ACC_E_ARG
        assert raw_call(ctx, s, good, end_inclusive=1 - ei) == L.ACC_E_ARG
        assert ctx._lib.acc_rcmd_redundant_before(ctx.handle, s._h, None) == L.ACC_E_ARG
        assert ctx._lib.acc_rcmd_redundant_before(ctx.handle, None, C.byref(L.CfkRedundantIn())) == L.ACC_E_ARG
        assert ctx._lib.acc_rcmd_redundant_view(ctx.handle, s._h, None) == L.ACC_E_ARG
        assert_unchanged(s, snap, "rejected calls")
        mark(ctx, s, m, ranges_of([]), "n_ranges == 0")
        assert_unchanged(s, snap, "n_ranges == 0")
        # TxnId.NONE as a bound cuts nothing (the map records it)
        mark(ctx, s, m, ranges_of([(0, 1000, (0, 0, 0))]), "bound NONE")
        assert m.rstats["cmds_cut"] == 0 and m.rstats["cmds_dropped"] == 0
        for k in ("rng_start", "rng_end", "msb"):
            np.testing.assert_array_equal(s.table()[k], snap[0][k])
        # device-memory inputs give what host inputs give
        import torch
        other, mo = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
        try:
            feed(ctx, other, mo, cmd_updates(items), "second store")
            mark(ctx, other, mo, ranges_of([(0, 1000, (0, 0, 0))]), "second store, bound NONE")
            cols = dict(rs=call["rng_start"], re=call["rng_end"], bm=call["msb"], bl=call["lsb"], bn=call["node"])
            t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(torch.device("cuda", 0)) for k, v in cols.items()}
            torch.cuda.synchronize()
            ri = L.CfkRedundantIn(L.ACC_MEM_DEVICE, len(call["msb"]), ei, t["rs"].data_ptr(), t["re"].data_ptr(),
                                  L.TsCols(t["bm"].data_ptr(), t["bl"].data_ptr(), t["bn"].data_ptr()))
            ctx.check(ctx._lib.acc_rcmd_redundant_before(ctx.handle, other._h, C.byref(ri)))
            mo.mark(call)
            check(ctx, other, mo, "device inputs", "mark")
            for k, v in cols.items():
                np.testing.assert_array_equal(t[k].cpu().numpy(), v, err_msg=f"the call wrote into the caller's {k}")
            # two stores on one context, interleaved, with different maps
            mark(ctx, s, m, ranges_of([(0, 16, ts(8)), (16, 40, ts(150))]), "first store")
            check(ctx, other, mo, "second store after the first store's prune")
            feed(ctx, other, mo, updates([(ts(12), 0, [(0, 100)])]), "second store's update under its own map")
            feed(ctx, s, m, updates([(ts(12), 0, [(0, 100)])]), "first store's update under its own map")
            assert not np.array_equal(s.table()["rng_start"], other.table()["rng_start"])
            check(ctx, other, mo, "second store at the end")
            check_reads(other, mo, q, recq, "second store")
            check_reads(s, m, q, recq, "first store")
        finally:
            other.close()
        # a prune that empties the store: no tombstone may be in it
        e, me = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
        try:
            feed(ctx, e, me, cmd_updates([i for i in items if not i[1] & ERASED]), "no tombstones")
            mark(ctx, e, me, ranges_of([(0, 1 << 40, ts(1000))]), "the emptying prune")
            tab = e.table()
            assert len(tab["msb"]) == 0 and tab["rng_off"].tolist() == [0] and len(tab["dict_start"]) == 0
            assert e.state()["dep_off"].tolist() == [0] and "store_emptied" in me.seen
            g = e.rangedeps(q)
            assert g.u_off.tolist() == [0] * (len(q["msb"]) + 1)
            feed(ctx, e, me, cmd_updates([(ts(2000), HAS_DEPS, [(1, 9)], 2, None, [key_dep(ts(1), 3)]), (ts(5), 0, [(1, 9)], 1, None, [])]),
                 "the next update")
            assert len(e.table()["msb"]) == 2 and len(e.table()["rng_start"]) == 1
            check_reads(e, me, q, recq, "after the emptying prune")
        finally:
            e.close()
    finally:
        s.close()


# ---------------------------------------------------------------- 6. ReplicaStore.mark_shard_durable

def test_replica_loop_with_mark_shard_durable(ctx):
    """propose, apply both halves, the PartialDeps of the new txns, prune both halves, the range recovery scans: four
    batches of about 100 queries. The CommandsForKey half against cfk_redundant_model as
    test_cfk_redundant_scale_gpu's replica test checks it; MaxConflicts against oracle.max_conflicts over every earlier
    update (a prune does not touch it)."""
    import cfk_cases as CC
    import cfk_redundant_cases as RCS
    import test_cfk_redundant_gpu as RG
    from accord_amd.deps import _execute_at_after
    ei = 1
    u = W.cfk_update_stream(700, 3, 200, dist="zipf", window=200)
    cuts = W.cfk_stream_cuts(u, 300, 100, 4)
    ids = RCS.first_txn_ids(u)
    lo, hi = int(u["key"].min()) - 1, int(u["key"].max())
    edge = [lo + (hi - lo) * r // 3 for r in range(4)]
    cm, state = RCS.CallMap(1), CC.empty_snapshot()
    rng = np.random.default_rng(23)
    kinds = [W.WRITE, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT]
    rs, m = ReplicaStore(ctx, ei), RM.RedundantModel(ei)
    all_upd = []

    def range_id(i):   # a range-domain TxnId beside key txn i's, on a node no key txn uses (no MaxConflicts tie)
        t = ids[i]
        return (int(t[0]), (int(t[1]) & ~0xF) | (kinds[int(rng.integers(3))] << 1) | 1, 100 + int(rng.integers(4)))

    def range_part(a0, a1):
        items = []
        for _ in range(60):
            i = int(rng.integers(max(0, a0 - 250), a1))
            w = int(rng.integers(1, max(2, (hi - lo) // 3)))
            a = int(rng.integers(lo, hi - w))
            nd = int(rng.integers(0, 3))
            deps = sorted((key_dep(tuple(int(x) for x in ids[int(rng.integers(0, a1))]), int(rng.integers(lo + 1, hi))) for _ in range(nd)),
                          key=lambda d: order(d[0]))
            items.append((range_id(i), HAS_DEPS if nd else 0, [(a, a + w)], int(rng.integers(1, 9)), None, deps))
        return cmd_updates(items)

    try:
        a, state = RCS.apply_step(state, cm, W.cfk_slice(u, 0, cuts[0]))
        rp = range_part(0, 300)
        rs.preaccept_batch(W.cfk_slice(u, 0, cuts[0]), scan=False, range_part=rp)
        m.apply(rp)
        all_upd.append((W.conflicts_updates(W.cfk_slice(u, 0, cuts[0]), ei), rp))
        hits = 0
        for b in range(4):
            part = W.cfk_slice(u, cuts[b], cuts[b + 1])
            newest = 300 + 100 * (b + 1)
            rp = range_part(newest - 100, newest)
            q = W.preaccept_queries(part)
            extra = [range_id(newest - 1 - j) for j in range(6)]
            per = np.diff(q["part_off"].astype(np.int64))
            q = dict(msb=np.concatenate([q["msb"], np.array([t[0] for t in extra], np.uint64)]),
                     lsb=np.concatenate([q["lsb"], np.array([t[1] for t in extra], np.uint64)]),
                     node=np.concatenate([q["node"], np.array([t[2] + 50 for t in extra], np.int32)]),
                     is_range=np.concatenate([np.zeros(len(per), np.uint8), np.ones(6, np.uint8)]),
                     part_off=np.concatenate([[0], np.cumsum(np.concatenate([per, np.ones(6, np.int64)]))]).astype(np.uint32),
                     part_start=np.concatenate([q["part_start"], np.array([lo + 20 * j for j in range(6)], np.uint64)]),
                     part_end=np.concatenate([np.zeros(len(q["part_start"]), np.uint64),
                                              np.array([lo + 20 * j + 60 for j in range(6)], np.uint64)]))
            assert len(q["msb"]) == 106
            r = rs.preaccept_batch(part, q, scan="new", range_part=rp)
            om = oracle.max_conflicts(conflicts_of(all_upd, ei), q)
            for k in ("msb", "lsb", "node", "fast"):
                np.testing.assert_array_equal(r["propose"][k], om[k], err_msg=f"batch {b} propose {k}")
            all_upd.append((W.conflicts_updates(part, ei), rp))
            a, state = RCS.apply_step(state, cm, part)
            RG.assert_store(ctx, rs.cfk, a["state"], f"batch {b} applied")
            m.apply(rp)
            check(ctx, rs.rcmd, m, f"batch {b} range half applied")
            nq = mixed_queries_from_preaccept(q)
            nq.update(zip(("xmsb", "xlsb", "xnode"), _execute_at_after(part, q)))
            assert_rd(r["rangedeps_new"], expect_rangedeps(m.table(), nq, ei), f"batch {b} rangedeps_new")
            hits += int((np.diff(r["rangedeps_new"].u_off.astype(np.int64)) > 0).sum())
            ranges = ranges_of([(edge[k], edge[k + 1], tuple(int(x) for x in ids[newest - (150, 180, 210)[k]])) for k in range(3)])
            p, state = RCS.prune_step(state, cm, ranges)
            rs.mark_shard_durable(ranges)
            m.mark(ranges)
            RG.assert_stats(ctx, p["counts"], f"batch {b} prune")
            RG.assert_map(rs.cfk, p["map"], f"batch {b} prune")
            RG.assert_store(ctx, rs.cfk, p["state"], f"batch {b} pruned")
            check(ctx, rs.rcmd, m, f"batch {b} range half pruned", "mark")
            assert m.rstats["cmds_cut"] + m.rstats["cmds_dropped"] > 0
            recq = M.domain_queries(dict(q, msb=q["msb"][-30:], lsb=q["lsb"][-30:], node=q["node"][-30:], is_range=q["is_range"][-30:],
                                         part_off=(q["part_off"][-31:] - q["part_off"][-31]).astype(np.uint32),
                                         part_start=q["part_start"][int(q["part_off"][-31]):], part_end=q["part_end"][int(q["part_off"][-31]):]))
            g = rs.begin_recovery_ranges(M.mixed(recq))
            mc = m.cmds()
            tab = dict(msb=mc["txn_msb"], lsb=mc["txn_lsb"], node=mc["txn_node"])
            for name, scan in rs._RECOVERY_NAMES.items():
                want = M.expect(mc, recq, L.RECOVERY_SCANS[scan])
                if name.startswith("has_"):
                    assert g[name].tolist() == [bool(w) for w in want], (b, name)
                else:
                    assert M.as_txn_dicts(g[name], len(recq["msb"]), tab) == want, (b, name)
                hits += sum(1 for w in want if w)
        assert hits > 0
    finally:
        rs.close()


# ---------------------------------------------------------------- 7. a store that was never marked

def launched(c):
    """the launch names acc_timing has counted since the last reset"""
    return {name for name, (_, cnt) in c.timing().items() if cnt}


def test_never_marked_store_is_unchanged():
    """no trim pre-pass is launched while the map is empty; once it holds a bound the pre-pass runs"""
    c = Context(0, timing=True)
    try:
        for ei in (0, 1):
            s, m = RangeCmdStore(c, ei), RM.RedundantModel(ei)
            try:
                items, call, _, _ = hand_worked()
                c.timing_reset()
                feed(c, s, m, cmd_updates(items), "never marked")
                names = launched(c)
                assert "rc_fold" in names and "rc_write" in names, names
                assert not [n for n in names if n.startswith(("rt_", "rp_", "rb_"))], names
                assert c.stats()["rcmd.update_ranges_trimmed"] == 0
                s.redundant_before(ranges_of([]))            # a no-op call leaves it never marked
                m.mark(ranges_of([]))
                c.timing_reset()
                feed(c, s, m, cmd_updates(items[:3]), "after a no-op call")
                assert not [n for n in launched(c) if n.startswith(("rt_", "rp_", "rb_"))]
                mark(c, s, m, call, "marked")
                c.timing_reset()
                feed(c, s, m, cmd_updates(items), "marked store")
                assert {"rt_owner", "rt_count", "rt_off", "rt_write"} <= launched(c)
            finally:
                s.close()
    finally:
        c.close()


@pytest.mark.parametrize("ei", [0, 1])
def test_hand_worked_store_of_the_plain_update_through_the_model(ctx, ei):
    """test_rcmd_gpu.test_hand_worked_store's updates and expectations, through the model with an empty map"""
    A, B, Cc, Dd, E, F = (ts(10 * i, W.WRITE) for i in range(1, 7))
    items = [(A, 0, [(1, 3)]), (B, 0, [(1, 3)]), (A, 0, [(3, 5)]), (B, 0, [(2, 4)]), (A, 0, [(2, 4)]), (B, 0, [(3, 5)]),
             (Cc, 0, [(10, 20), (30, 40)]), (Cc, 0, [(12, 15), (30, 35)]), (Dd, 0, []), (E, 0, [(2, 6)]), (E, ERASED, [(100, 200)]),
             (F, 0, [(4, 12)])]
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    try:
        tab = feed(ctx, s, m, updates(items), "hand-worked, empty map")
        off = tab["rng_off"].tolist()
        rows = [list(zip(tab["rng_start"][a:b].tolist(), tab["rng_end"][a:b].tolist())) for a, b in zip(off, off[1:])]
        assert rows == [[(1, 3), (3, 5)], [(1, 5)], [(10, 20), (30, 40)], [], [], [(4, 12)]]
        assert tab["flags"].tolist() == [0, 0, 0, 0, ERASED, 0]
        assert list(zip(tab["dict_start"].tolist(), tab["dict_end"].tolist())) == [(1, 3), (1, 5), (3, 5), (4, 12), (10, 20), (30, 40)]
        st = ctx.stats()
        assert (st["rcmd.inserted"], st["rcmd.updated"], st["rcmd.skipped_key_domain"], st["rcmd.erased_ignored"]) == (6, 0, 0, 0)
        assert len(s.redundant_map()["st"]) == 0 and m.trimmed == 0
    finally:
        s.close()
