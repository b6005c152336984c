"""GPU parity for acc_rcmd_partial_rangedeps (RangeCmdStore.partial_rangedeps, ReplicaStore.preaccept_batch with
redundant_deps): PreAccept's builder.build().with(redundant) (messages/PreAccept.java:245-265) from the resident
range-command store, the stab result united with RedundantBefore.collectDeps (local/RedundantBefore.java:181-190,
418-421).

Expected values come from partial_rangedeps_model.partial_rangedeps (pinned by hand-worked literals in
test_partial_rangedeps_model.py) over the model's table (rcmd_redundant_model.RedundantModel; in the two large cases,
built so that no bound prunes anything, its fold with the ranges added to its map directly), the stab half
test_rcmd_gpu.expect_rangedeps and the map's intervals with the raw bound bits the store's own view reports. Every comparison is exact and on every array: the union dictionary, the CSR, ids, id_row.
The old call is compared beside the new one, on the same queries. The stream was fixed on the host model alone
(stream_case asserts what it must exercise)."""
import functools

import numpy as np
import pytest

import partial_rangedeps_model as PM
import rcmd_redundant_model as RM
from accord_amd import _lib as L
from accord_amd import workload as W
from accord_amd.deps import Context, IllegalArgumentException, IllegalStateException, RangeCmdStore, ReplicaStore
from cfk_redundant_model import NONE, order, ranges_of, updates_of
from test_rcmd_gpu import RD_FIELDS, assert_rd, assert_table, expect_rangedeps, queries, ts, updates

pytestmark = pytest.mark.gpu

ERASED = L.ACC_RCMD_ERASED
NO_ROW = PM.NO_ROW
FLAG = 0x20      # an lsb bit outside Timestamp.IDENTITY_LSB


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def check_partial(ctx, s, m, q, msg, intervals=None):
    """the new call against the model and the old call against expect_rangedeps, on the same queries; returns the
    model's result and the stats of the new call"""
    tab = m.table()
    stab = expect_rangedeps(tab, q, m.ei)
    want = PM.partial_rangedeps(tab, stab, PM.device_intervals(s, m) if intervals is None else intervals, q, m.ei)
    g = s.partial_rangedeps(q)
    st = ctx.stats()
    PM.assert_partial(g, want, msg)
    assert st["rcmd.partial_intervals"] == want["intervals"], (msg, st["rcmd.partial_intervals"], want["intervals"])
    assert st["rcmd.partial_pairs_shared"] == want["shared"], (msg, st["rcmd.partial_pairs_shared"], want["shared"])
    assert st["rcmd.union_ids"] == len(want["msb"]) and st["rcmd.union_ranges"] == len(want["rng_start"]), msg
    assert_rd(s.rangedeps(q), stab, msg + ": acc_rcmd_rangedeps did not change")
    return want, st


# ---------------------------------------------------------------- 1. a store never marked

def test_unmarked_store_is_the_plain_call():
    """No bound above NONE: every array of partial_rangedeps equals rangedeps, ids are the table's columns, id_row is
    arange, and ctx.timing() names no kernel the plain call does not launch."""
    c = Context(0, timing=True)
    s = RangeCmdStore(c, 1)
    try:
        rng = np.random.default_rng(5)
        items = [(ts(100 + 3 * i, [W.WRITE, W.READ, W.SYNC_POINT][i % 3]), ERASED if i % 17 == 5 else 0,
                  [(int(a), int(a) + int(w))]) for i, (a, w) in enumerate(zip(rng.integers(0, 3000, 400), rng.integers(1, 200, 400)))]
        s.update(updates(items))
        qi = [(ts(5000 + i, W.WRITE, rng=i % 2), None, [] if i % 2 else sorted({int(x) for x in rng.integers(0, 3200, 3)}),
               [(int(a), int(a) + 50)] if i % 2 else []) for i, a in enumerate(rng.integers(0, 3000, 300))]
        q = queries(qi)
        tab = s.table()
        c.timing_reset()
        plain = s.rangedeps(q)
        plain_kernels = set(c.timing())
        c.timing_reset()
        g = s.partial_rangedeps(q)
        assert set(c.timing()) <= plain_kernels, sorted(set(c.timing()) - plain_kernels)
        st = c.stats()
        for f in RD_FIELDS:
            np.testing.assert_array_equal(getattr(g, f), getattr(plain, f), err_msg=f)
        for f in ("msb", "lsb", "node"):
            np.testing.assert_array_equal(g.ids[f], tab[f], err_msg=f)
        np.testing.assert_array_equal(g.id_row, np.arange(len(tab["msb"]), dtype=np.uint32))
        assert st["rcmd.union_builds"] == 0 and st["rcmd.partial_intervals"] == 0 and st["rcmd.partial_pairs_shared"] == 0
        assert st["rcmd.union_ids"] == len(tab["msb"]) and st["rcmd.union_ranges"] == len(tab["dict_start"])
        assert int((np.diff(g.u_off.astype(np.int64)) > 0).sum()) > 100
    finally:
        s.close()
        c.close()


# ---------------------------------------------------------------- 2. the hand-worked store

def hand_worked():
    """Nine commands, then one call of five ranges (read [s, e) or (s, e] by the bound type; the query keys lie strictly
    inside, so the arithmetic is the same):
         M3 (2, 8) bound hlc 5 | M1 (10, 20) bound hlc 100 | M2 (30, 40) bound hlc 200, S's TxnId with a bit outside
         compareTo | M4 (70, 80) bound hlc 300 | M5 (90, 95) bound hlc 900
       TxnId              ranges             after the call               union id
       hlc 5   (M3)                                                       0  no row: below the first row
       hlc 20  I          (3, 6)             above M3's bound: stays      1  row 0
       hlc 60  G          (12, 18)           inside M1, below it: dropped
       hlc 100 (M1)                                                       2  no row: between rows
       hlc 150 A          (10, 15) (50, 65)  above M1's bound: stays      3  row 1
       hlc 160 Bq         (10, 25)           stays                        4  row 2
       hlc 200 S SyncPoint (30, 40)          equal to M2's bound: stays   5  row 3 = M2's bound, the row's bits
       hlc 300 E erased   -                  a tombstone                  6  row 4 = M4's bound
       hlc 400 F          (85, 99)           below M5: (85, 90) (95, 99)  7  row 5
       hlc 450 J Read     (32, 36)           stays                        8  row 6
       hlc 500 H          (75, 78)           above M4's bound: stays      9  row 7
       hlc 900 (M5)                                                       10 no row: above the last row
       The union dictionary: M3 (2, 8) before every stored range; M1 (10, 20) shares its start with (10, 15), the shorter,
       and (10, 25), the longer; M2 equals the stored (30, 40); M4 (70, 80) shares nothing, between (50, 65) and (75, 78);
       M5 (90, 95) between F's two pieces:
         (2,8) (3,6) (10,15) (10,20) (10,25) (30,40) (32,36) (50,65) (70,80) (75,78) (85,90) (90,95) (95,99)
       query                                      result: range -> TxnIds
       0 ESP hlc 1000, range (0, 100)             every stored pair and all five intervals; (30,40) -> [S] on both sides, once
       1 Write hlc 1001, keys 13 14 17            (10,15) -> [A]  (10,20) -> [hlc 100]  (10,25) -> [Bq]: three keys in M1, one pair
       2 Write hlc 1002, key 55                   (50,65) -> [A]: stab hits, no interval
       3 Write hlc 1003, key 72                   (70,80) -> [hlc 300]: an interval, no stab hit; the id is an erased row
       4 Write hlc 120, key 35                    (30,40) -> [hlc 200]: the query is below its bound (no STARTED_BEFORE test)
       5 S's TxnId as a key txn, key 35           (30,40) -> [hlc 200]: the query equals its bound (no self exclusion)
       6 Read hlc 1006, key 35                    (30,40) -> [hlc 200]: a Read witnesses neither S nor J; the pair is there
       7 Write hlc 1007, range (88, 97)           (85,90) -> [F]  (90,95) -> [hlc 900]  (95,99) -> [F]
       8 Write hlc 1008, no participants          nothing
       rcmd.partial_intervals = 5 + 1 + 0 + 1 + 1 + 1 + 1 + 1 + 0 = 11, rcmd.partial_pairs_shared = 1 (query 0)."""
    Wr = W.WRITE
    S = ts(200, W.SYNC_POINT)
    items = [(ts(20), 0, [(3, 6)]), (ts(60), 0, [(12, 18)]), (ts(150), 0, [(10, 15), (50, 65)]), (ts(160), 0, [(10, 25)]),
             (S, 0, [(30, 40)]), (ts(300), ERASED, []), (ts(400), 0, [(85, 99)]), (ts(450, W.READ), 0, [(32, 36)]),
             (ts(500), 0, [(75, 78)])]
    call = ranges_of([(2, 8, ts(5)), (10, 20, ts(100)), (30, 40, ts(200, W.SYNC_POINT, extra=FLAG)), (70, 80, ts(300)),
                      (90, 95, ts(900))])
    qi = [(ts(1000, W.EXCLUSIVE_SYNC_POINT), None, [], [(0, 100)]), (ts(1001, Wr, rng=0), None, [13, 14, 17], []),
          (ts(1002, Wr, rng=0), None, [55], []), (ts(1003, Wr, rng=0), None, [72], []), (ts(120, Wr, rng=0), None, [35], []),
          ((S[0], S[1] & ~1, S[2]), None, [35], []), (ts(1006, W.READ, rng=0), None, [35], []),
          (ts(1007, Wr), None, [], [(88, 97)]), (ts(1008, Wr), None, [], [])]
    h = lambda x, k=Wr: order(ts(x, k))  # noqa: E731
    I, A, Bq, So, F, J, H = h(20), h(150), h(160), order(S), h(400), h(450, W.READ), h(500)
    want = [
        {(2, 8): [h(5)], (3, 6): [I], (10, 15): [A], (10, 20): [h(100)], (10, 25): [Bq], (30, 40): [So], (32, 36): [J],
         (50, 65): [A], (70, 80): [h(300)], (75, 78): [H], (85, 90): [F], (90, 95): [h(900)], (95, 99): [F]},
        {(10, 15): [A], (10, 20): [h(100)], (10, 25): [Bq]}, {(50, 65): [A]}, {(70, 80): [h(300)]}, {(30, 40): [So]},
        {(30, 40): [So]}, {(30, 40): [So]}, {(85, 90): [F], (90, 95): [h(900)], (95, 99): [F]}, {}]
    dictionary = [(2, 8), (3, 6), (10, 15), (10, 20), (10, 25), (30, 40), (32, 36), (50, 65), (70, 80), (75, 78), (85, 90),
                  (90, 95), (95, 99)]
    id_row = [NO_ROW, 0, NO_ROW, 1, 2, 3, 4, 5, 6, 7, NO_ROW]
    return items, call, qi, want, dictionary, id_row, S


@pytest.mark.parametrize("ei", [0, 1])
def test_hand_worked_store(ctx, ei):
    items, call, qi, table, dictionary, id_row, S = hand_worked()
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    try:
        s.update(updates(items))
        m.apply(updates(items))
        s.redundant_before(call)
        m.mark(call)
        assert_table(s.table(), m.table(), "hand-worked")
        q = queries(qi)
        want, st = check_partial(ctx, s, m, q, "hand-worked")
        assert [PM.describe(want, t) for t in range(len(qi))] == table, "the model gives the docstring's table"
        assert list(zip(want["rng_start"].tolist(), want["rng_end"].tolist())) == dictionary
        assert want["id_row"].tolist() == id_row
        g = s.partial_rangedeps(q)
        assert (int(g.ids["msb"][5]), int(g.ids["lsb"][5]), int(g.ids["node"][5])) == S, "the stored row's bits, not the bound's"
        assert int(m.table()["flags"][4]) & ERASED and g.id_row[6] == 4, "M4's bound is the erased row"
        assert st["rcmd.partial_intervals"] == 11 and st["rcmd.partial_pairs_shared"] == 1
        assert st["rcmd.union_ids"] == 11 and st["rcmd.union_ranges"] == 13
    finally:
        s.close()


# ---------------------------------------------------------------- 3. a chained random stream

SPACE = 4000
STREAM_SEED = {0: 1, 1: 1}
STREAM_TAGS = {"shared_pair", "bound_not_stored", "bound_equals_erased_row", "interval_range_in_dictionary",
               "redundant_only_query", "stab_only_query", "range_query_spans_gap", "index_reused",
               "index_rebuilt_after_update", "index_rebuilt_after_mark"}


def stream_queries(rng, n, lo, hi):
    items = []
    for i in range(n):
        kind = [W.WRITE, W.READ, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT][i % 4]
        t = ts(int(rng.integers(lo, hi)), kind, node=int(rng.integers(1, 5)), rng=1 if i % 3 == 1 else 0)
        if i % 3 == 1:
            a = int(rng.integers(0, SPACE - 900))
            r = [(a, a + int(rng.integers(1, 500)))]
            if i % 2:
                r.append((r[0][1] + int(rng.integers(0, 3)), r[0][1] + int(rng.integers(3, 300))))
            items.append((t, None, [], r))
        else:
            items.append((t, None, sorted({int(x) for x in rng.integers(0, SPACE, size=int(rng.integers(0, 5)))}), []))
    return items


def tags_of(m, want, q):
    """what a query step exercised, read off the model alone"""
    seen = set()
    tab = m.table()
    iv = [(r, v) for r, v in m.raw_intervals() if v > order(NONE)]
    keys = [order(t) for t in zip(tab["msb"], tab["lsb"], tab["node"])]
    erased = {k for k, f in zip(keys, tab["flags"]) if f & ERASED}
    stored = set(zip(tab["dict_start"].tolist(), tab["dict_end"].tolist()))
    if want["shared"]:
        seen.add("shared_pair")
    if (want["id_row"] == NO_ROW).any():
        seen.add("bound_not_stored")
    if any(v in erased for _, v in iv):
        seen.add("bound_equals_erased_row")
    if any(r in stored for r, _ in iv):
        seen.add("interval_range_in_dictionary")
    live = sorted(r for r, _ in iv)
    for t, (left, right) in enumerate(want["per_query"]):
        if right and not left:
            seen.add("redundant_only_query")
        if left and not right:
            seen.add("stab_only_query")
        for a, b in zip(q["rng_start"][int(q["rng_off"][t]):int(q["rng_off"][t + 1])].tolist(),
                        q["rng_end"][int(q["rng_off"][t]):int(q["rng_off"][t + 1])].tolist()):
            hit = [r for r in live if r[0] < b and a < r[1]]
            if any(x[1] < y[0] for x, y in zip(hit, hit[1:])):
                seen.add("range_query_spans_gap")
    return seen


@functools.lru_cache(maxsize=None)
def stream_case(seed, ei):
    """Four rounds of: an update of about 150 commands around the moving bounds; queries; a prune of ranges with gaps
    between them, some bounds the raw TxnId of a stored command; queries, twice; an update that stores some of the
    map's bounds as range commands over their own interval (the sync point itself: the shared pair), stores a later
    command over another interval's range, and erases a sync point stored the round before; queries. Built on a
    scratch model, which also says how often the union index is built: by the first query step after an update or a
    prune while the map is not empty, and by no other."""
    rng = np.random.default_rng(seed * 7919 + ei)
    m = RM.RedundantModel(ei)
    kinds = [W.READ, W.WRITE, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT]
    steps, seen, stored_sync = [], set(), []
    builds, dirty = 0, None

    def query(n=90):
        nonlocal builds, dirty
        q = queries(stream_queries(rng, n, 100, 1000 * (p + 2)))
        tab = m.table()
        want = PM.partial_rangedeps(tab, expect_rangedeps(tab, q, ei), PM.model_intervals(m), q, ei)
        marked = len(m.map.intervals()) > 0
        if marked and dirty:
            builds += 1
            seen.add("index_rebuilt_after_" + dirty)
        elif marked:
            seen.add("index_reused")
        if marked:
            dirty = None
        seen.update(tags_of(m, want, q))
        steps.append(("query", q, builds))

    def update(items):
        nonlocal dirty
        upd = updates(items)
        m.apply(upd)
        steps.append(("update", upd, builds))
        dirty = "update"

    for p in range(4):
        lo, hi = (100, 900) if p == 0 else (1000 * p - 400, 1000 * p + 1600)
        ids = [ts(int(h), kinds[int(rng.integers(4))], node=int(rng.integers(1, 4))) for h in rng.integers(lo, hi, size=110)]
        items = []
        for _ in range(150):
            t = ids[int(rng.integers(len(ids)))]
            k = int(rng.integers(0, 3))
            pts = np.sort(rng.choice(SPACE, size=2 * k, replace=False)) if k else []
            items.append((t, ERASED if rng.random() < 0.05 and p > 0 else 0, [(int(pts[2 * j]), int(pts[2 * j + 1])) for j in range(k)]))
        update(items)
        query()
        live = [c[0] for c in m.cmd.values() if not c[1] and c[2] is not None and len(c[2])]
        call, at = [], int(rng.integers(0, 200))
        b = 1000 * (p + 1)
        while at < SPACE - 300:
            w = int(rng.integers(20, 260))
            bound = ts(b - int(rng.choice([0, 400, 900])), node=int(rng.integers(1, 4)))
            if live and rng.random() < 0.25:
                bound = live[int(rng.integers(len(live)))]
            if rng.random() < 0.05:
                bound = NONE
            call.append((at, at + w, bound))
            at += w + (0 if rng.random() < 0.4 else int(rng.integers(1, 400)))
        r = ranges_of(call)
        m.mark(r)
        steps.append(("mark", r, builds))
        dirty = "mark"
        query()
        query()
        iv = PM.model_intervals(m)
        livei = [x for x in iv if x[1] > order(NONE)]
        pick = [livei[int(i)] for i in rng.choice(len(livei), size=min(4, len(livei)), replace=False)]
        crafted = [((raw[0], raw[1] | 1, raw[2]), 0, [rng_]) for rng_, _, raw in pick[:3]]        # the sync points themselves
        crafted.append((ts(b + 5000 + p, W.WRITE), 0, [pick[-1][0]]))                              # a later command, an interval's range
        if stored_sync:
            crafted.append((stored_sync[0], ERASED, []))                                          # a bound equal to an erased row
        stored_sync = [c[0] for c in crafted[:3]]
        update(crafted)
        query()
    assert seen >= STREAM_TAGS, sorted(STREAM_TAGS - seen)
    return steps


@pytest.mark.parametrize("ei", [0, 1])
def test_chained_random_stream(ctx, ei):
    steps = stream_case(STREAM_SEED[ei], ei)
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    try:
        for i, (op, arg, builds) in enumerate(steps):
            if op == "update":
                s.update(arg)
                m.apply(arg)
            elif op == "mark":
                s.redundant_before(arg)
                m.mark(arg)
            else:
                assert_table(s.table(), m.table(), f"step {i}")
                RM.assert_map(s, m, f"step {i}")
                _, st = check_partial(ctx, s, m, arg, f"step {i}")
                assert st["rcmd.union_builds"] == builds, (i, st["rcmd.union_builds"], builds)
    finally:
        s.close()


# ---------------------------------------------------------------- 4. crossings

@pytest.mark.parametrize("ei", [0, 1])
def test_build_tier_edges(ctx, ei):
    """rd_build_txns takes a txn's raw pairs in tiers of at most 16, 32, 64 and 8,192 pairs, and beyond. 8,200 nested
    one-range commands all intersect one range query, which by its executeAt sees the k below it: k stab pairs and the
    three collected ones make 16 / 17, 32 / 33, 64 / 65 and 8,192 / 8,193 raw pairs. Of the three intervals (bounds
    below every command: nothing is pruned) (100, 200) sorts before every stored range, (30000, 30010) after, and
    (19990, 19995) shares its start with the stored (19990, 20010), in the middle of every query's ranges."""
    N = 8200
    items = [(ts(1000 + 2 * i, W.WRITE), 0, [(20000 - 1 - i, 20001 + i)]) for i in range(N)]
    call = ranges_of([(100, 200, ts(10)), (19990, 19995, ts(20)), (30000, 30010, ts(30))])
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    try:
        s.update(updates(items))
        m.apply(updates(items))             # nothing is marked yet: nothing to trim
        s.redundant_before(call)
        m.map.add(call)                     # bounds below every command: the prune changes nothing
        assert ctx.stats()["rcmd.redundant_cmds_cut"] == 0 and ctx.stats()["rcmd.redundant_cmds_dropped"] == 0
        raw = [16, 17, 32, 33, 64, 65, 8192, 8193]
        qi = [(ts(90000 + j, W.WRITE), ts(1000 + 2 * (r - 3), W.WRITE, node=0), [], [(50, 40000)]) for j, r in enumerate(raw)]
        want, st = check_partial(ctx, s, m, queries(qi), "tier edges")
        assert np.diff(want["u_off"].astype(np.int64)).tolist() == raw, "k commands and three bounds"
        for t in range(len(raw)):
            r0, r1 = int(want["rd_off"][t]), int(want["rd_off"][t + 1])
            rid = want["range_id"][r0:r1].tolist()
            mid = rid.index(int(np.flatnonzero((want["rng_start"] == 19990) & (want["rng_end"] == 19995))[0]))
            assert rid[0] == 0 and rid[-1] == len(want["rng_start"]) - 1 and 0 < mid < len(rid) - 1
        assert st["rangedeps.s16_txns"] >= 1 and st["rangedeps.s32_txns"] >= 2 and st["rangedeps.s64_txns"] >= 2
        assert st["rangedeps.block_txns"] >= 2 and st["rangedeps.global_txns"] == 1
    finally:
        s.close()


def many_case(ei):
    rng = np.random.default_rng(40 + ei)
    NI, NB, NR = 1200, 700, 5000
    items = []
    for i in range(NR):
        j = int(rng.integers(0, NI))
        a = 100 * j + 61 + int(rng.integers(0, 30))
        items.append((ts(10000 + 3 * i, [W.WRITE, W.READ, W.SYNC_POINT][i % 3], node=1 + i % 3), ERASED if i % 97 == 3 else 0,
                      [(a, a + 1 + int(rng.integers(0, 8)))]))
    # bounds: below every row, between rows (hlc 10000 + 3 i + 1), equal to rows (erased ones among them), above all
    pool = ([ts(int(h)) for h in rng.choice(np.arange(100, 9000), 150, replace=False)]
            + [ts(10001 + 3 * int(i), node=2) for i in rng.choice(NR, 250, replace=False)]
            + [items[int(i)][0] for i in rng.choice(NR, 200, replace=False)]
            + [ts(int(h)) for h in rng.choice(np.arange(30000, 40000), 100, replace=False)])
    assert len({order(t) for t in pool}) == NB
    bounds = pool + [pool[int(i)] for i in rng.integers(0, NB, NI - NB)]
    bounds = [bounds[int(i)] for i in rng.permutation(NI)]
    call = ranges_of([(100 * j, 100 * j + 60, bounds[j]) for j in range(NI)])
    return rng, items, bounds, call


@pytest.mark.parametrize("ei", [0, 1])
def test_many_intervals_rows_and_queries(ctx, ei):
    """5,000 rows, 1,200 intervals with 700 distinct bounds, 720 queries. No merge is partitioned here: every row, bound,
    interval, dictionary range, index entry, participant and query is one thread of a 256-thread workgroup that places
    itself by binary search, so the sizes that matter are the workgroup's: 700 bounds are 3 workgroups of k_pu_gloc and
    k_pu_gwrite, 1,200 intervals 5 of k_pu_keys, k_pu_iloc and k_pu_iwrite, 5,000 rows and about as many dictionary
    ranges and entries 20 of k_pu_rows, k_pu_dict and k_pu_info, 720 queries 3 of k_pu_tinfo and (with over 1,500
    participants) 6 of k_pu_collect and k_pu_records; bounds and interval ranges fall inside every workgroup of rows
    and of dictionary ranges. Interval j is (100 j, 100 j + 60); every stored range lies in a gap (100 j + 60,
    100 j + 100), so whatever the bounds nothing is pruned and the table is the plain fold. One range query each
    touches 0, 1, 2, 65 and 300 intervals."""
    NI, NR = 1200, 5000
    rng, items, bounds, call = many_case(ei)
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    try:
        s.update(updates(items))
        m.apply(updates(items))
        s.redundant_before(call)
        m.map.add(call)
        assert ctx.stats()["rcmd.redundant_cmds_cut"] == 0 and ctx.stats()["rcmd.redundant_cmds_dropped"] == 0
        assert_table(s.table(), m.table(), "many: nothing pruned")
        g = s.redundant_map()
        assert len(g["st"]) == NI
        iv = []
        for j in range(NI):
            raw = (int(g["msb"][j]), int(g["lsb"][j]), int(g["node"][j]))
            assert order(raw) == order(bounds[j]) and int(g["st"][j]) == 100 * j + ei and int(g["en"][j]) == 100 * j + 59 + ei
            iv.append(((100 * j, 100 * j + 60), order(raw), raw))
        qi = [(ts(50000 + c, W.EXCLUSIVE_SYNC_POINT), None, [], [(100 * 7 + 70, 100 * 7 + 70 + w)])
              for c, w in enumerate([20, 60, 160, 6460, 29960])]
        spans = [0, 1, 2, 65, 300]
        for i in range(715):
            t = ts(int(rng.integers(5000, 45000)), [W.WRITE, W.READ, W.EXCLUSIVE_SYNC_POINT][i % 3], node=5, rng=i % 2)
            if i % 2:
                a = int(rng.integers(0, 100 * NI - 500))
                qi.append((t, None, [], [(a, a + int(rng.integers(1, 400)))]))
            else:
                qi.append((t, None, sorted({int(x) for x in rng.integers(0, 100 * NI, size=4)}), []))
        q = queries(qi)
        assert len(q["key_code"]) + len(q["rng_start"]) > 1500
        want, st = check_partial(ctx, s, m, q, "many", intervals=iv)
        assert [len(r) for _, r in want["per_query"][:5]] == spans
        assert (want["id_row"] == NO_ROW).sum() == 500 and len(want["msb"]) == NR + 500
        assert st["rcmd.union_builds"] == 1
        both = sum(1 for left, right in want["per_query"] if left and right)
        assert both > 50
    finally:
        s.close()


# ---------------------------------------------------------------- 5. empties

def test_empty_store_marked_and_no_queries(ctx):
    ei = 1
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    try:
        q = queries([(ts(100, W.WRITE, rng=0), None, [5], []), (ts(101, W.WRITE), None, [], [(0, 30)]),
                     (ts(102, W.WRITE, rng=0), None, [50], [])])
        none = queries([])
        call = ranges_of([(0, 10, ts(7)), (20, 25, ts(9, node=-2)), (40, 45, NONE)])
        s.redundant_before(call)
        m.mark(call)
        want, st = check_partial(ctx, s, m, q, "an empty store with a map")       # the NE == 0 exit must not skip them
        assert [PM.describe(want, t) for t in range(3)] == [{(0, 10): [order(ts(7))]},
                                                            {(0, 10): [order(ts(7))], (20, 25): [order(ts(9, node=-2))]}, {}]
        assert want["id_row"].tolist() == [NO_ROW, NO_ROW] and st["rcmd.union_builds"] == 1
        want, st = check_partial(ctx, s, m, none, "n_query == 0")
        assert len(want["msb"]) == 2 and len(want["rng_start"]) == 2 and st["rcmd.union_builds"] == 1
        # a store filled and then emptied by a prune: only the bounds are left
        s.update(updates([(ts(50), 0, [(1, 9)]), (ts(60), 0, [(21, 24), (60, 70)])]))
        m.apply(updates([(ts(50), 0, [(1, 9)]), (ts(60), 0, [(21, 24), (60, 70)])]))
        check_partial(ctx, s, m, q, "filled")
        s.redundant_before(ranges_of([(0, 1000, ts(500))]))
        m.mark(ranges_of([(0, 1000, ts(500))]))
        assert len(s.table()["msb"]) == 0 and "store_emptied" in m.seen
        want, st = check_partial(ctx, s, m, q, "emptied by a prune")
        assert [PM.describe(want, t) for t in range(3)] == [{(0, 1000): [order(ts(500))]}] * 3
        assert st["rcmd.union_builds"] == 3
        check_partial(ctx, s, m, none, "emptied, n_query == 0")
        # a map of NONE bounds only: the plain call
        e, me = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
        try:
            e.update(updates([(ts(50), 0, [(1, 9)])]))
            me.apply(updates([(ts(50), 0, [(1, 9)])]))
            e.redundant_before(ranges_of([(0, 5, NONE)]))
            me.mark(ranges_of([(0, 5, NONE)]))
            want, st = check_partial(ctx, e, me, q, "NONE bounds only")
            assert want["id_row"].tolist() == [0] and st["rcmd.partial_intervals"] == 0
        finally:
            e.close()
    finally:
        s.close()


# ---------------------------------------------------------------- 6. errors

def test_errors_leave_the_store_and_the_index_unharmed(ctx):
    """every error case of test_rcmd_gpu.test_empties_and_errors, from the new call"""
    import ctypes as C

    from accord_amd.deps import _mixed_queries_in
    ei = 1
    s, m = RangeCmdStore(ctx, ei), RM.RedundantModel(ei)
    try:
        first = [(ts(10), 0, [(1, 5)]), (ts(20), 0, [(3, 9), (9, 12)])]
        s.update(updates(first))
        m.apply(updates(first))
        call = ranges_of([(0, 2, ts(15)), (6, 8, ts(5))])
        s.redundant_before(call)
        m.mark(call)
        q = queries([(ts(100, W.WRITE, rng=0), None, [5], []), (ts(101, W.WRITE), None, [], [(0, 10)])])
        _, st = check_partial(ctx, s, m, q, "before the rejected calls")
        builds = st["rcmd.union_builds"]
        tab = s.table()

        def bad_query(items, exc=IllegalArgumentException, **patch):
            u = queries(items)
            u.update(patch)
            with pytest.raises(exc):
                s.partial_rangedeps(u)

        K, R = ts(100, W.WRITE, rng=0), ts(101, W.WRITE)
        bad_query([(R, None, [5], [])])                                                  # a range-domain query with keys
        bad_query([(K, None, [], [(1, 2)])])                                             # a key-domain query with ranges
        bad_query([(R, None, [], [(5, 5)])])
        bad_query([(R, None, [], [(1, 5), (4, 8)])])
        bad_query([(K, None, [5, 5], [])])                                               # duplicate keys
        bad_query([(K, None, [7, 5], [])])                                               # unsorted keys
        bad_query([(K, None, [5], []), (K, None, [6], [])], key_off=np.array([0, 2, 1], np.uint32))
        bad_query([(R, None, [], [(1, 2)]), (R, None, [], [(1, 2)])], rng_off=np.array([1, 1, 2], np.uint32))
        bad_query([(ts(100, kind=7, rng=0), None, [5], [])])                             # kind ordinal
        bad_query([(ts(100, W.LOCAL_ONLY, rng=0), None, [5], [])], IllegalStateException)
        other = RangeCmdStore(ctx, 0)                                                    # the other bound type
        try:
            keep = []
            qi = _mixed_queries_in(q, ei, 0, keep)
            view = L.RcmdPartialView()
            assert ctx._lib.acc_rcmd_partial_rangedeps(ctx.handle, other._h, C.byref(qi), C.byref(view)) == L.ACC_E_ARG
            qi.end_inclusive = 0
            qi.n_pairs = (1 << 32) - 1                                                   # n_pairs + n_ranges >= 2^32 - 1
            assert ctx._lib.acc_rcmd_partial_rangedeps(ctx.handle, other._h, C.byref(qi), C.byref(view)) == L.ACC_E_ARG
            other.redundant_before(ranges_of([(0, 2, ts(15))]))                          # and with a map
            assert ctx._lib.acc_rcmd_partial_rangedeps(ctx.handle, other._h, C.byref(qi), C.byref(view)) == L.ACC_E_ARG
        finally:
            other.close()
        assert_table(s.table(), tab, "queries do not modify the store")
        _, st = check_partial(ctx, s, m, q, "after the rejected calls")
        assert st["rcmd.union_builds"] == builds, "the cached index served the call after the errors"
    finally:
        s.close()


# ---------------------------------------------------------------- 7. ReplicaStore

def test_replica_store_redundant_deps(ctx):
    """A write on key 100 stored and applied; mark_shard_durable over (99, 100] with a bound above it; then a new write on
    key 100 is pre-accepted: keydeps_new no longer lists the old write, and partial_rangedeps_new holds exactly
    ((99, 100], bound). The same batches without the flag return today's keys, unchanged; without the prune the old
    write is a key dep."""
    ei = 1
    A, B, Nw = ts(10, W.WRITE, rng=0), ts(20, W.SYNC_POINT), ts(30, W.WRITE, rng=0)
    part1 = updates_of([(A, W.PREACCEPTED, [100], []), (A, W.APPLIED, [100], [])])
    part2 = updates_of([(Nw, W.PREACCEPTED, [100], [])])
    call = ranges_of([(99, 100, B)])
    flagged, plain, unpruned = ReplicaStore(ctx, ei), ReplicaStore(ctx, ei), ReplicaStore(ctx, ei)
    try:
        for rs in (flagged, plain, unpruned):
            rs.preaccept_batch(part1, scan="new")
        flagged.mark_shard_durable(call)
        plain.mark_shard_durable(call)
        r = flagged.preaccept_batch(part2, scan="new", redundant_deps=True)
        r0 = plain.preaccept_batch(part2, scan="new")
        r1 = unpruned.preaccept_batch(part2, scan="new")
        assert set(r) == {"propose", "keydeps_new", "partial_rangedeps_new"}
        assert set(r0) == {"propose", "keydeps_new", "rangedeps_new"} == set(r1)
        assert r1["keydeps_new"].u_off.tolist() == [0, 1], "unpruned: the old write is the new one's key dep"
        assert r["keydeps_new"].u_off.tolist() == [0, 0], "pruned: it is listed no more"
        for f in ("arena_off", "kd_off", "u_off", "arena", "key_idx", "dep_txn"):
            np.testing.assert_array_equal(getattr(r["keydeps_new"], f), getattr(r0["keydeps_new"], f), err_msg=f)
        assert r0["rangedeps_new"].u_off.tolist() == [0, 0]
        p = r["partial_rangedeps_new"]
        assert (p.rng_start.tolist(), p.rng_end.tolist()) == ([99], [100])
        assert p.u_off.tolist() == [0, 1] and p.rd_off.tolist() == [0, 1] and p.arena_off.tolist() == [0, 2]
        assert p.range_id.tolist() == [0] and p.dep_txn.tolist() == [0] and p.arena.tolist() == [2, 0]
        assert (int(p.ids["msb"][0]), int(p.ids["lsb"][0]), int(p.ids["node"][0])) == B and p.id_row.tolist() == [NO_ROW]
    finally:
        for rs in (flagged, plain, unpruned):
            rs.close()
