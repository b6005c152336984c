"""GPU parity for the device-resident range-command store (acc_rcmd_*: RangeCmdStore, ReplicaStore.preaccept_batch with
range_part): InMemorySafeStore.update for range commands (impl/InMemoryCommandStore.java:739-762, RangeCommand.update =
ranges.with(add)) and the range-command half of mapReduceActive for new txns (:863-870, :883-960).

Expected values.
  The table: a Python fold of accord_amd.ranges.Ranges.with_ (the host acc_ranges_with) over the updates in array order
  per TxnId (Model below): raw bits of the first instance, flags, rng_off, ranges; the dictionary = the distinct ranges
  of the non-erased commands in (start, end) order. Every with() of that fold is also asserted equal to the independent
  model (ranges_model.py); test_rcmd_fold_gpu.py checks the device fold against that model alone.
  The queries: the host copy of the table as range-domain rows in table order (PREACCEPTED, or INVALID_OR_TRUNCATED for
  erased rows, executeAt = TxnId), every query appended as a row with its TxnId and executeAt (a key-domain query with
  its keys and PREACCEPTED; a range-domain query with its ranges and INVALID_OR_TRUNCATED: evaluated as a query, no
  range command, nothing added to the dictionary), then oracle.rangedeps_batch_queries over the appended rows: row
  n_cmd + i is query i, dep_txn are table indices, the dictionary is the store's.
Every comparison is on every array."""
import numpy as np
import pytest

import oracle
import ranges_model
import rd_cases
from accord_amd import _lib as L
from accord_amd import workload as W
from accord_amd.deps import (IllegalArgumentException, IllegalStateException, RangeCmdStore, ReplicaStore,
                             mixed_queries_from_preaccept)
from accord_amd.ranges import Ranges

pytestmark = pytest.mark.gpu

IDENT = 0xFFFFFFFFFFFF001E
ERASED = L.ACC_RCMD_ERASED
RD_FIELDS = ("rng_start", "rng_end", "arena_off", "rd_off", "u_off", "arena", "range_id", "dep_txn")
TABLE_FIELDS = ("msb", "lsb", "node", "flags", "rng_off", "rng_start", "rng_end", "dict_start", "dict_end")


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


def ts(hlc, kind=W.WRITE, node=1, rng=1, extra=0, epoch=1):
    """a TxnId (msb, lsb, node): flags = kind << 1 | domain bit | extra (bits outside the identity flags)"""
    return tuple(int(x) for x in W.encode_ts(epoch, hlc, (kind << 1) | rng | extra, node))


def ident(t):
    return (t[0], t[1] & IDENT, t[2])


def updates(items):
    """items: [(txn_id, flags, [(start, end)])] -> the RangeCmdStore.update dict"""
    ro, rs, re_ = [0], [], []
    for _, _, ranges in items:
        rs.extend(a for a, _ in ranges); re_.extend(b for _, b in ranges)
        ro.append(len(rs))
    return dict(msb=np.array([t[0] for t, _, _ in items], np.uint64), lsb=np.array([t[1] for t, _, _ in items], np.uint64),
                node=np.array([t[2] for t, _, _ in items], np.int32), flags=np.array([f for _, f, _ in items], np.uint8),
                rng_off=np.array(ro, np.uint32), rng_start=np.array(rs, np.uint64), rng_end=np.array(re_, np.uint64))


def queries(items):
    """items: [(txn_id, execute_at or None, [key codes], [(start, end)])] -> the RangeCmdStore.rangedeps dict"""
    ko, kc, ro, rs, re_ = [0], [], [0], [], []
    for _, _, keys, ranges in items:
        kc.extend(keys); ko.append(len(kc))
        rs.extend(a for a, _ in ranges); re_.extend(b for _, b in ranges); ro.append(len(rs))
    ex = [t if x is None else x for t, x, _, _ in items]
    return dict(msb=np.array([t[0] for t, _, _, _ in items], np.uint64), lsb=np.array([t[1] for t, _, _, _ in items], np.uint64),
                node=np.array([t[2] for t, _, _, _ in items], np.int32), xmsb=np.array([x[0] for x in ex], np.uint64),
                xlsb=np.array([x[1] for x in ex], np.uint64), xnode=np.array([x[2] for x in ex], np.int32),
                key_off=np.array(ko, np.uint32), key_code=np.array(kc, np.uint64), rng_off=np.array(ro, np.uint32),
                rng_start=np.array(rs, np.uint64), rng_end=np.array(re_, np.uint64))


class Model:
    """The host model of the store: InMemorySafeStore.update per update in array order, Ranges.with by the host
    restatement, each result asserted equal to ranges_model.with_. seen: what the stream exercised."""

    def __init__(self, end_inclusive):
        self.ei = end_inclusive
        self.cmd = {}   # identity -> [raw TxnId, erased, Ranges or None]
        self.seen = set()
        self.stats = dict(inserted=0, updated=0, skipped_key_domain=0, erased_ignored=0)

    def apply(self, upd):
        st = dict(inserted=0, updated=0, skipped_key_domain=0, erased_ignored=0)
        before = sorted(self.cmd)
        touched, batch_ids = set(), set()
        for u in range(len(upd["msb"])):
            t = (int(upd["msb"][u]), int(upd["lsb"][u]), int(upd["node"][u]))
            if not t[1] & 1:
                st["skipped_key_domain"] += 1
                continue
            k = ident(t)
            if k in batch_ids:
                self.seen.add("in_batch_repeat")
            batch_ids.add(k)
            a, b = int(upd["rng_off"][u]), int(upd["rng_off"][u + 1])
            add = Ranges(upd["rng_start"][a:b], upd["rng_end"][a:b], self.ei)
            if k not in self.cmd:
                self.cmd[k] = [t, False, None]
                st["inserted"] += 1
                if before and k < before[0]:
                    self.seen.add("insert_below_lowest")
                if before and k > before[-1]:
                    self.seen.add("insert_above_highest")
            elif k in before and k not in touched:
                st["updated"] += 1
            touched.add(k)
            c = self.cmd[k]
            if c[1]:
                st["erased_ignored"] += 1
            elif int(upd["flags"][u]) & ERASED:
                c[1], c[2] = True, None
            elif c[2] is None:
                c[2] = add
            else:
                left = c[2]
                res = left.with_(add)
                # the independent model (ranges_model.py) folds beside the host restatement, at every step
                assert list(res) == ranges_model.with_(list(left), list(add)), (list(left), list(add))
                same = len(res) == len(left) and np.array_equal(res.start, left.start) and np.array_equal(res.end, left.end)
                if len(left) and len(add):
                    if same:
                        self.seen.add("shortcut_unchanged")
                    elif len(res) == len(left) + len(add):
                        self.seen.add("appended_disjoint")
                    elif len(res) < len(left) + len(add):
                        self.seen.add("merged")
                c[2] = res
        self.stats = st

    def table(self):
        keys = sorted(self.cmd, key=lambda k: (k[0], k[1], k[2]))
        rows = [self.cmd[k] for k in keys]
        rs = [r[2].start if r[2] is not None else np.zeros(0, np.uint64) for r in rows]
        re_ = [r[2].end if r[2] is not None else np.zeros(0, np.uint64) for r in rows]
        live = sorted({(int(a), int(b)) for r, s, e in zip(rows, rs, re_) if not r[1] for a, b in zip(s, e)})
        return dict(msb=np.array([r[0][0] for r in rows], np.uint64), lsb=np.array([r[0][1] for r in rows], np.uint64),
                    node=np.array([r[0][2] for r in rows], np.int32),
                    flags=np.array([ERASED if r[1] else 0 for r in rows], np.uint8),
                    rng_off=np.concatenate([[0], np.cumsum([len(x) for x in rs])]).astype(np.uint32),
                    rng_start=np.concatenate(rs + [np.zeros(0, np.uint64)]).astype(np.uint64),
                    rng_end=np.concatenate(re_ + [np.zeros(0, np.uint64)]).astype(np.uint64),
                    dict_start=np.array([a for a, _ in live], np.uint64), dict_end=np.array([b for _, b in live], np.uint64))


def assert_table(got, want, msg=""):
    for f in TABLE_FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{msg}: table {f}")


def expect_rangedeps(tab, q, end_inclusive):
    """the recipe of the module docstring"""
    n, nq = len(tab["msb"]), len(q["msb"])
    cat = lambda a, b, dt: np.concatenate([np.asarray(a, dt), np.asarray(b, dt)])  # noqa: E731
    qrange = (np.asarray(q["lsb"], np.uint64) & np.uint64(1)).astype(bool)
    status = cat(np.where(tab["flags"] & ERASED, W.INVALID_OR_TRUNCATED, W.PREACCEPTED),
                 np.where(qrange, W.INVALID_OR_TRUNCATED, W.PREACCEPTED), np.uint8)
    kb = W.Batch(cat(tab["msb"], q["msb"], np.uint64), cat(tab["lsb"], q["lsb"], np.uint64), cat(tab["node"], q["node"], np.int32),
                 cat(tab["msb"], q["xmsb"], np.uint64), cat(tab["lsb"], q["xlsb"], np.uint64), cat(tab["node"], q["xnode"], np.int32),
                 status, cat(np.zeros(n, np.uint32), q["key_off"], np.uint32), np.asarray(q["key_code"], np.uint64))
    roff = cat(tab["rng_off"][:-1], np.asarray(q["rng_off"], np.int64) + int(tab["rng_off"][-1]), np.uint32)
    rb = W.RangeBatch(kb, roff, cat(tab["rng_start"], q["rng_start"], np.uint64), cat(tab["rng_end"], q["rng_end"], np.uint64),
                      end_inclusive)
    o = oracle.rangedeps_batch_queries(rb, np.arange(n, n + nq)) if nq else None
    out = dict(rng_start=tab["dict_start"], rng_end=tab["dict_end"])
    for off, arr in (("arena_off", "arena"), ("rd_off", "range_id"), ("u_off", "dep_txn")):
        if o is None:
            out[off], out[arr] = np.zeros(1, np.uint64), np.zeros(0, np.uint32)
            continue
        full = getattr(o, off)
        assert int(full[n]) == 0, "the table rows are no queries"
        out[off] = full[n:].astype(np.uint64)
        out[arr] = getattr(o, arr)
    if o is not None:
        np.testing.assert_array_equal(o.rng_start, tab["dict_start"], err_msg="recipe: the oracle's dictionary is the store's")
        np.testing.assert_array_equal(o.rng_end, tab["dict_end"])
    return out


def assert_rd(g, want, msg=""):
    for f in RD_FIELDS:
        np.testing.assert_array_equal(getattr(g, f), want[f], err_msg=f"{msg}: {f}")


def check_queries(store, q, end_inclusive, msg=""):
    tab = store.table()
    g = store.rangedeps(q)
    assert_rd(g, expect_rangedeps(tab, q, end_inclusive), msg)
    return g


def ndeps(g):
    return np.diff(g.u_off.astype(np.int64))


# ---------------------------------------------------------------- 1. hand-worked store

@pytest.mark.parametrize("ei", [0, 1])
def test_hand_worked_store(ctx, ei):
    A, B, Cc, Dd, E, F = (ts(10 * i, W.WRITE) for i in range(1, 7))
    items = [
        (A, 0, [(1, 3)]), (B, 0, [(1, 3)]),
        (A, 0, [(3, 5)]), (B, 0, [(2, 4)]),
        (A, 0, [(2, 4)]), (B, 0, [(3, 5)]),           # A: {[1,3),[3,5)}; B: {[1,5)}
        (Cc, 0, [(10, 20), (30, 40)]), (Cc, 0, [(12, 15), (30, 35)]),   # superset short-cut: unchanged
        (Dd, 0, []),                                    # a command without ranges
        (E, 0, [(2, 6)]), (E, ERASED, [(100, 200)]),    # erased: its ranges leave the table
        (F, 0, [(4, 12)]),
    ]
    m = Model(ei)
    s = RangeCmdStore(ctx, ei)
    try:
        s.update(updates(items))
        m.apply(updates(items))
        tab = s.table()
        assert_table(tab, m.table(), "hand-worked")
        off = tab["rng_off"].tolist()
        pairs = lambda i: list(zip(tab["rng_start"][off[i]:off[i + 1]].tolist(), tab["rng_end"][off[i]:off[i + 1]].tolist()))  # noqa: E731
        assert pairs(0) == [(1, 3), (3, 5)]
        assert pairs(1) == [(1, 5)]
        assert pairs(2) == [(10, 20), (30, 40)]
        assert pairs(3) == [] and pairs(4) == [] and pairs(5) == [(4, 12)]
        assert tab["flags"].tolist() == [0, 0, 0, 0, ERASED, 0]
        assert list(zip(tab["dict_start"].tolist(), tab["dict_end"].tolist())) == [(1, 3), (1, 5), (3, 5), (4, 12), (10, 20), (30, 40)]
        st = ctx.stats()
        assert (st["rcmd.inserted"], st["rcmd.updated"], st["rcmd.skipped_key_domain"], st["rcmd.erased_ignored"]) == (6, 0, 0, 0)
        assert st["rcmd.entries"] == 6 and st["rcmd.stored_ranges"] == 6
        q = queries([
            (ts(100, W.WRITE, rng=0), None, [2, 3, 4, 11], []),
            (ts(101, W.WRITE), None, [], [(0, 2), (4, 11)]),
            (ts(25, W.WRITE, rng=0), None, [2, 3], []),            # only A and B started before
            (ts(102, W.READ, rng=0), None, [5, 12, 40], []),
            (ts(103, W.EXCLUSIVE_SYNC_POINT), None, [], [(0, 1000)]),
            (ts(104, W.WRITE, rng=0), None, [], []),               # no participants
        ])
        g = check_queries(s, q, ei, "hand-worked")
        assert ndeps(g)[0] >= 3 and ndeps(g)[4] == 4 and ndeps(g)[5] == 0
        assert 4 not in g.dep_txn.tolist(), "the erased command is never a dep"
    finally:
        s.close()


# ---------------------------------------------------------------- 2. chained random stream

def random_updates(rng, n_upd, ids, space, lo_id, hi_id):
    items = []
    for _ in range(n_upd):
        t = ids[int(rng.integers(len(ids)))]
        u = rng.random()
        if u < 0.06:
            t = (t[0], t[1] & ~1, t[2])                            # a key-domain TxnId: ignored
        k = int(rng.integers(0, 4))
        pts = np.sort(rng.choice(space, size=2 * k, replace=False)) if k else np.zeros(0, np.int64)
        rngs = [(int(pts[2 * i]), int(pts[2 * i + 1])) for i in range(k)]
        items.append((t, ERASED if 0.06 <= u < 0.16 else 0, rngs))
    items.insert(len(items) // 3, (lo_id, 0, [(5, 9)]))
    items.insert(len(items) // 2, (hi_id, 0, [(7, 30)]))
    return items


def random_queries(rng, nq, ids, space):
    items = []
    for i in range(nq):
        kind = [W.WRITE, W.READ, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT][int(rng.integers(4))]
        is_r = rng.random() < 0.5
        if rng.random() < 0.2:
            t = ids[int(rng.integers(len(ids)))]                   # maybe a member
            t = (t[0], (t[1] & ~0xF) | (kind << 1) | (1 if is_r else 0), t[2])
        else:
            t = ts(int(rng.integers(2000, 6000)), kind, node=int(rng.integers(1, 5)), rng=1 if is_r else 0)
        ex = ts(int(rng.integers(2000, 6200)), W.WRITE, node=900) if rng.random() < 0.2 else None
        if is_r:
            k = int(rng.integers(0, 3))
            pts = np.sort(rng.choice(space, size=2 * k, replace=False)) if k else []
            items.append((t, ex, [], [(int(pts[2 * j]), int(pts[2 * j + 1])) for j in range(k)]))
        else:
            items.append((t, ex, sorted(int(x) for x in rng.choice(space, size=int(rng.integers(0, 5)), replace=False)), []))
    return items


@pytest.mark.parametrize("ei", [0, 1])
def test_chained_random_stream(ctx, ei):
    rng = np.random.default_rng(0xACC0 + ei)
    space = 300
    kinds = [W.READ, W.WRITE, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT, W.EPHEMERAL_READ]
    ids = [ts(int(h), kinds[int(rng.integers(5))], node=int(rng.integers(1, 4))) for h in rng.integers(2000, 6000, size=1500)]
    m = Model(ei)
    s = RangeCmdStore(ctx, ei)
    with_deps = total = 0
    try:
        for b in range(5):
            upd = updates(random_updates(rng, 600, ids, space, ts(1000 - b, W.WRITE), ts(7000 + b, W.WRITE)))
            s.update(upd)
            st = ctx.stats()
            m.apply(upd)
            assert_table(s.table(), m.table(), f"batch {b}")
            for k, v in m.stats.items():
                assert st["rcmd." + k] == v, (b, k)
            g = check_queries(s, queries(random_queries(rng, 500, ids, space)), ei, f"batch {b}")
            with_deps += int((ndeps(g) > 0).sum())
            total += 500
        assert m.seen >= {"merged", "shortcut_unchanged", "appended_disjoint", "in_batch_repeat", "insert_below_lowest",
                          "insert_above_highest"}, m.seen
        assert 2 * with_deps >= total, (with_deps, total)
    finally:
        s.close()


# ---------------------------------------------------------------- 3. timestamps

def test_timestamps_and_witnesses(ctx):
    ei = 1
    # stored TxnIds varying in msb, lsb and node at once, every kind
    stored = [ts(50, W.WRITE, node=3), ts(50, W.WRITE, node=-2), ts(60, W.READ, node=1, epoch=2), ts(40, W.SYNC_POINT, node=7, epoch=2),
              ts(70, W.EXCLUSIVE_SYNC_POINT, node=1), ts(80, W.EPHEMERAL_READ, node=1), ts(90, W.LOCAL_ONLY, node=1),
              ts((1 << 48) + 5, W.WRITE, node=1), ts(30, W.READ, node=5)]
    m = Model(ei)
    s = RangeCmdStore(ctx, ei)
    try:
        upd = updates([(t, 0, [(10 + i, 100 + i)]) for i, t in enumerate(stored)])
        s.update(upd)
        m.apply(upd)
        tab = s.table()
        assert_table(tab, m.table(), "timestamps")
        order = sorted(range(len(stored)), key=lambda i: ident(stored[i]))
        srt = [stored[i] for i in order]
        far = ts((1 << 48) + 99, W.WRITE, epoch=3)
        items = [
            (srt[2], far, [], [(40, 60)]),                         # a member with a bumped executeAt: never its own dep
            (ts(55, W.EXCLUSIVE_SYNC_POINT, rng=0), srt[3], [50], []),   # executeAt equal to a stored TxnId: that one excluded
            (ts(56, W.EXCLUSIVE_SYNC_POINT, rng=0), ts(1, W.WRITE), [50], []),   # executeAt below every stored TxnId
            ((srt[1][0], srt[1][1] | 0x20 | 0x8000, srt[1][2]), far, [], [(0, 1000)]),   # flag bits outside IDENTITY_LSB: that command
        ]
        for qk in (W.READ, W.WRITE, W.EPHEMERAL_READ, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT):   # each query kind x each stored kind
            items.append((ts(57, qk, rng=0, node=11), far, [50], []))
            items.append((ts(58, qk, rng=1, node=11), far, [], [(40, 60)]))
        g = check_queries(s, queries(items), ei, "timestamps")
        n = ndeps(g)
        dep = lambda i: g.dep_txn[int(g.u_off[i]):int(g.u_off[i + 1])].tolist()  # noqa: E731
        assert dep(0) == [0, 1, 6, 8], "reads and writes below the executeAt, the query's own command left out"
        assert 3 not in dep(1) and 2 in dep(1) and max(dep(1)) == 2
        assert n[2] == 0
        assert dep(3) == [0, 2, 6, 8]
        assert n[4 + 8] == 7, "an ExclusiveSyncPoint witnesses every globally visible kind: all but EphemeralRead, LocalOnly"
    finally:
        s.close()


# ---------------------------------------------------------------- 4. tier and tile crossings of the reused stages

@pytest.mark.parametrize("ei", [0, 1])
def test_tier_and_tile_crossings(ctx, ei):
    N = 9000
    nested = [(ts(100 + i, W.WRITE), 0, [(20000 - 1 - i, 20001 + i)]) for i in range(N)]       # all hold key 20000
    flat = [(ts(50000 + i, W.WRITE), 0, [(100000 + i, 100003 + i)]) for i in range(1000)]      # one width class, 1,000 starts
    wide = [(ts(70000 + i, W.WRITE), 0, [(300000 + 37 * i, 300000 + 37 * i + w)]) for i, w in enumerate([2, 9, 200, 5000, 70000] * 8)]
    m = Model(ei)
    s = RangeCmdStore(ctx, ei)
    try:
        upd = updates(nested + flat + wide)
        s.update(upd)
        m.apply(upd)
        assert_table(s.table(), m.table(), "tiers")
        late = ts(90000, W.WRITE)
        items = []
        hits = [15, 16, 17, 31, 32, 33, 63, 64, 65, 1100, 9000]
        for k in hits:     # executeAt = the TxnId of nested command k: the k commands below it
            items.append((ts(95000 + k, W.WRITE, rng=0), ts(100 + k, W.WRITE), [20000], []))
        # a block of 256 key queries over the span of the 1,000 one-class ranges (a class window beyond one 256-entry tile)
        for j in range(256):
            items.append((ts(96000 + j, W.WRITE, rng=0), late, [100000 + 3 * j + 2], []))
        # range queries in all four width groups (below 2^4, 2^8, 2^12, beyond)
        for j, w in enumerate([3, 100, 3000, 100000]):
            items.append((ts(97000 + j, W.WRITE), late, [], [(300010, 300010 + w)]))
            items.append((ts(97100 + j, W.WRITE), late, [], [(19990, 19990 + w)]))
        g = check_queries(s, queries(items), ei, "tiers")
        assert ndeps(g)[:len(hits)].tolist() == hits
        assert (ndeps(g)[len(hits):len(hits) + 256] > 0).all()
        st = ctx.stats()
        assert st["rangedeps.block_txns"] >= 1 and st["rangedeps.global_txns"] >= 1 and st["rangedeps.s16_txns"] >= 1
    finally:
        s.close()


# ---------------------------------------------------------------- 5. erasure

def test_erasure(ctx):
    ei = 0
    A, B, Cc, Z = ts(10), ts(20), ts(30), ts(5)
    m = Model(ei)
    s = RangeCmdStore(ctx, ei)
    try:
        q = queries([(ts(100, W.WRITE, rng=0), None, [12, 25, 55], []), (ts(101, W.WRITE), None, [], [(0, 100)])])
        for step, items in enumerate([
            [(A, 0, [(10, 20)]), (B, 0, [(20, 30)]), (Cc, 0, [(50, 60)])],
            [(A, ERASED, [])],                                      # A's range leaves the dictionary: ids shift
            [(A, 0, [(10, 20)]), (A, ERASED, [])],                  # later updates of it are ignored
            [(Z, ERASED, [(1, 2)])],                                # an absent TxnId: a row that is never a dep
        ]):
            upd = updates(items)
            s.update(upd)
            st = ctx.stats()
            m.apply(upd)
            tab = s.table()
            assert_table(tab, m.table(), f"erasure step {step}")
            g = check_queries(s, q, ei, f"erasure step {step}")
            if step == 0:
                assert tab["dict_start"].tolist() == [10, 20, 50] and g.dep_txn.tolist() == [0, 1, 2, 0, 1, 2]
            if step == 1:
                assert tab["dict_start"].tolist() == [20, 50] and g.range_id.tolist() == [0, 1, 0, 1]
                assert g.dep_txn.tolist() == [1, 2, 1, 2]
            if step == 2:
                assert st["rcmd.erased_ignored"] == 2 and st["rcmd.updated"] == 1 and st["rcmd.inserted"] == 0
            if step == 3:
                assert st["rcmd.inserted"] == 1 and tab["flags"].tolist() == [ERASED, ERASED, 0, 0]
                assert tab["rng_off"].tolist() == [0, 0, 0, 1, 2] and g.dep_txn.tolist() == [2, 3, 2, 3]
    finally:
        s.close()


# ---------------------------------------------------------------- 6. ownership

def test_store_owns_its_arrays(ctx):
    ei = 1
    rng = np.random.default_rng(7)
    ids = [ts(int(h), W.WRITE) for h in rng.integers(2000, 6000, size=400)]
    s = RangeCmdStore(ctx, ei)
    try:
        s.update(updates(random_updates(rng, 500, ids, 300, ts(1000), ts(7000))))
        q = queries(random_queries(rng, 300, ids, 300))
        tab0 = s.table()
        g0 = s.rangedeps(q)
        # an unrelated batch through acc_rangedeps_batch on the same context reuses the rd_* buffer names
        rb = W.rangedeps_batch(3000, 0x51, key_bits=12, max_width_log2=6, end_inclusive=ei)
        o = oracle.rangedeps_batch(rb)
        gb = ctx.calculate_partial_range_deps(rb)
        np.testing.assert_array_equal(gb.dep_txn, o.dep_txn)
        assert_table(s.table(), tab0, "after an unrelated acc_rangedeps_batch")
        g1 = s.rangedeps(q)
        for f in RD_FIELDS:
            np.testing.assert_array_equal(getattr(g1, f), getattr(g0, f), err_msg=f)
        assert_rd(g1, expect_rangedeps(tab0, q, ei), "ownership")
        # and an update after it still sees the table
        s.update(updates([(ts(9000), 0, [(1, 2)])]))
        assert len(s.table()["msb"]) == len(tab0["msb"]) + 1
    finally:
        s.close()


# ---------------------------------------------------------------- 7. empties and errors

def test_empties_and_errors(ctx):
    ei = 1
    s = RangeCmdStore(ctx, ei)
    try:
        q = queries([(ts(100, W.WRITE, rng=0), None, [5], []), (ts(101, W.WRITE), None, [], [(0, 10)])])
        none = queries([])
        t = s.table()
        assert len(t["msb"]) == 0 and t["rng_off"].tolist() == [0] and len(t["dict_start"]) == 0
        g = s.rangedeps(q)                                          # empty store
        assert g.u_off.tolist() == [0, 0, 0] and g.arena_off.tolist() == [0, 0, 0] and len(g.dep_txn) == 0 and len(g.rng_start) == 0
        g = s.rangedeps(none)                                       # n_query == 0
        assert g.u_off.tolist() == [0]
        s.update(updates([]))                                       # n_upd == 0
        assert len(s.table()["msb"]) == 0
        s.update(updates([(ts(10, rng=0), 0, [])]))                 # key-domain TxnIds only
        assert len(s.table()["msb"]) == 0 and ctx.stats()["rcmd.skipped_key_domain"] == 1
        first = [(ts(10), 0, [(1, 5)]), (ts(20), 0, [(3, 9), (9, 12)])]
        s.update(updates(first))                                    # first update on an empty store
        m = Model(ei)
        m.apply(updates(first))
        tab = s.table()
        assert_table(tab, m.table(), "first update")
        assert s.rangedeps(none).u_off.tolist() == [0]
        check_queries(s, q, ei, "after the first update")

        def bad_update(items, **patch):
            u = updates(items)
            u.update(patch)
            with pytest.raises(IllegalArgumentException):
                s.update(u)
            assert_table(s.table(), tab, "a rejected update leaves the store unchanged")

        bad_update([(ts(30, kind=6), 0, [(1, 2)])])                                     # kind ordinal
        bad_update([(ts(30), 2, [(1, 2)])])                                             # a flag bit other than ERASED
        bad_update([(ts(30), 0, [(5, 5)])])                                             # start >= end
        bad_update([(ts(30), 0, [(1, 5), (4, 8)])])                                     # overlapping
        bad_update([(ts(30), 0, [(6, 8), (1, 3)])])                                     # unsorted
        bad_update([(ts(30), 0, [(1, 2)]), (ts(31), 0, [(1, 2)])], rng_off=np.array([1, 1, 2], np.uint32))   # does not start at 0
        bad_update([(ts(30), 0, [(1, 2)]), (ts(31), 0, [(1, 2)])], rng_off=np.array([0, 2, 1], np.uint32))   # decreases
        bad_update([(ts(30), 0, [(1, 2)]), (ts(31), 0, [(1, 2)])], rng_off=np.array([0, 1, 1], np.uint32))   # ends off n_ranges

        def bad_query(items, exc=IllegalArgumentException, **patch):
            u = queries(items)
            u.update(patch)
            with pytest.raises(exc):
                s.rangedeps(u)

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
        # the other bound type
        other = RangeCmdStore(ctx, 0)
        try:
            keep = []
            from accord_amd.deps import _mixed_queries_in
            import ctypes as C
            qi = _mixed_queries_in(q, ei, 0, keep)
            view = L.RangedepsView()
            assert ctx._lib.acc_rcmd_rangedeps(ctx.handle, other._h, C.byref(qi), C.byref(view)) == L.ACC_E_ARG
            qi.end_inclusive = 0
            qi.n_pairs = (1 << 32) - 1                                                   # n_pairs + n_ranges >= 2^32 - 1
            assert ctx._lib.acc_rcmd_rangedeps(ctx.handle, other._h, C.byref(qi), C.byref(view)) == L.ACC_E_ARG
        finally:
            other.close()
        assert_table(s.table(), tab, "queries do not modify the store")
        check_queries(s, q, ei, "after the rejected calls")
    finally:
        s.close()


# ---------------------------------------------------------------- 8. wide bounds through the reused stages

@pytest.mark.parametrize("ei", [0, 1])
@pytest.mark.parametrize("name", list(rd_cases.FAMILIES))
def test_bound_families(ctx, name, ei):
    """Every band of rd_stab_queries' query plan (61, 62, 63 and 64 bits, the hull of a mask of 21 runs) and both sides
    of rd_range_dict's 64-bit key (64 bits unsplit, 65 split, a 64-bit end field, the wide families split) from the
    store: about 400 commands of every width class, 300 key-domain and 300 range-domain queries, members with a bumped
    executeAt among them. The plans taken (rangedeps.query_bits, dict_bits, dict_split) equal the arithmetic on the
    bounds: the store's dictionary masks are the OR of the table's starts and of its ends, the query mask is the OR of
    every query low bound XOR the first one."""
    f = rd_cases.family(name, 0x5EED, ei)
    cmds = f["cmds"]
    kinds = [W.WRITE, W.READ, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT]
    tids = [ts(1000 + 3 * i, kinds[i % 4], node=1 + i % 3) for i in range(len(cmds))]
    items = [(t, ERASED if i % 41 == 20 else 0, r) for i, (t, r) in enumerate(zip(tids, cmds))]   # (the last command stays: d33's end at 2^32)
    m = Model(ei)
    s = RangeCmdStore(ctx, ei)
    try:
        upd = updates(items)
        s.update(upd)
        st = ctx.stats()
        m.apply(upd)
        tab = s.table()
        assert_table(tab, m.table(), f"family {name}")
        sb, eb = rd_cases.plan_bits(rd_cases.or_mask(tab["rng_start"])), rd_cases.plan_bits(rd_cases.or_mask(tab["rng_end"]))
        assert (st["rangedeps.dict_bits"], st["rangedeps.dict_split"]) == (sb + eb, int(sb + eb > 64)), (name, sb, eb)
        if name in rd_cases.FAMILY_DICT:
            assert (sb + eb, int(sb + eb > 64)) == rd_cases.FAMILY_DICT[name]
            assert name != "e64" or (sb, eb) == (0, 64), "the start field is empty, the end field is shifted in by 64"
        else:
            assert sb + eb > 64
        far = ts(1 << 40, W.WRITE, node=900)
        qi = []
        for i, k in enumerate(f["keyq"]):
            t = ts(1000 + 3 * (i * 7 % len(cmds)) + 1, kinds[i % 4], rng=0, node=5)
            qi.append((t, far if i % 3 == 0 else None, k, []))
        for i, r in enumerate(f["rngq"]):
            if i % 6 == 0:
                qi.append((tids[i * 5 % len(cmds)], far, [], r))     # a member with a bumped executeAt
            else:
                qi.append((ts(1000 + 3 * (i * 11 % len(cmds)) + 2, kinds[i % 4], node=6), far if i % 3 == 1 else None, [], r))
        q = queries(qi)
        g = check_queries(s, q, ei, f"family {name}")
        st = ctx.stats()
        ref = int(q["key_code"][0])
        qb = rd_cases.plan_bits(rd_cases.or_mask(q["key_code"], ref) | rd_cases.or_mask(q["rng_start"], ref))
        assert st["rangedeps.query_bits"] == qb, (name, qb)
        if name in rd_cases.FAMILY_QUERY_BITS:
            assert qb == rd_cases.FAMILY_QUERY_BITS[name]
        n = ndeps(g)
        assert (n[:len(f["keyq"])] > 0).sum() >= 50 and (n[len(f["keyq"]):] > 0).sum() >= 50
    finally:
        s.close()


# ---------------------------------------------------------------- 9. ReplicaStore

def test_replica_store_both_halves(ctx):
    ei = 1
    u = W.cfk_update_stream(900, keys_per_txn=3, n_keys=200, seed=0x77)
    cuts = W.cfk_stream_cuts(u, 300, 300, 2)
    rng = np.random.default_rng(11)
    # nodes the key txns do not use: no range TxnId is Timestamp.equals to a key TxnId (MaxConflicts' tie rule)
    ids = [ts(int(h), [W.WRITE, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT][int(rng.integers(3))], node=int(rng.integers(100, 104)))
           for h in rng.integers(1, 2000, size=300)]
    space = np.arange(0, 400)
    with_rp, without = ReplicaStore(ctx, ei), ReplicaStore(ctx, ei)
    m = Model(ei)
    all_upd = []
    try:
        assert len(cuts) == 3
        for b, (a0, a1) in enumerate(zip([0] + cuts[:-1], cuts)):
            part = W.cfk_slice(u, a0, a1)
            rp = updates(random_updates(rng, 120, ids, space, ts(3000 + b, W.WRITE), ts(4000 + b, W.WRITE)))
            q = W.preaccept_queries(part)
            # a few range-domain queries beside the batch's own
            extra = [ts(5000 + 10 * b + j, W.EXCLUSIVE_SYNC_POINT, node=9) for j in range(6)]
            per = np.diff(q["part_off"].astype(np.int64))
            q = dict(msb=np.concatenate([q["msb"], np.array([t[0] for t in extra], np.uint64)]),
                     lsb=np.concatenate([q["lsb"], np.array([t[1] for t in extra], np.uint64)]),
                     node=np.concatenate([q["node"], np.array([t[2] for t in extra], np.int32)]),
                     is_range=np.concatenate([np.zeros(len(per), np.uint8), np.ones(6, np.uint8)]),
                     part_off=np.concatenate([[0], np.cumsum(np.concatenate([per, np.ones(6, np.int64)]))]).astype(np.uint32),
                     part_start=np.concatenate([q["part_start"], np.array([20 * j for j in range(6)], np.uint64)]),
                     part_end=np.concatenate([np.zeros(len(q["part_start"]), np.uint64),
                                              np.array([20 * j + 50 for j in range(6)], np.uint64)]))
            # MaxConflicts as of the earlier batches: key and range updates
            prev = oracle.max_conflicts(conflicts_of(all_upd, ei), q) if all_upd else None
            r = with_rp.preaccept_batch(part, q, scan="new", range_part=rp)
            r0 = without.preaccept_batch(part, q, scan="new")
            m.apply(rp)
            assert_table(with_rp.rcmd.table(), m.table(), f"replica batch {b}")
            nq = mixed_queries_from_preaccept(q)
            from accord_amd.deps import _execute_at_after
            nq.update(zip(("xmsb", "xlsb", "xnode"), _execute_at_after(part, q)))
            assert_rd(r["rangedeps_new"], expect_rangedeps(with_rp.rcmd.table(), nq, ei), f"replica batch {b}")
            assert int((ndeps(r["rangedeps_new"]) > 0).sum()) > 0
            for f in ("arena_off", "kd_off", "u_off", "arena", "key_idx", "dep_txn", "kd_key"):
                np.testing.assert_array_equal(getattr(r["keydeps_new"], f), getattr(r0["keydeps_new"], f), err_msg=f)
            assert len(r0["rangedeps_new"].dep_txn) == 0 and r0["rangedeps_new"].u_off.tolist() == [0] * (len(q["msb"]) + 1)
            if prev is not None:
                for f in ("msb", "lsb", "node", "fast"):
                    np.testing.assert_array_equal(r["propose"][f], prev[f], err_msg=f"propose {f}, batch {b}")
            all_upd.append((W.conflicts_updates(part, ei), rp))
    finally:
        with_rp.close()
        without.close()


def conflicts_of(all_upd, ei):
    """every earlier batch's key updates (with their executeAts) and range updates (executeAt = TxnId, key-domain TxnIds
    dropped) as one oracle.max_conflicts update set"""
    xm, xl, xn, ko, key, ro, rs, re_ = [], [], [], [0], [], [0], [], []
    for ku, rp in all_upd:
        for i in range(len(ku["xmsb"])):
            xm.append(ku["xmsb"][i]); xl.append(ku["xlsb"][i]); xn.append(ku["xnode"][i])
            key.extend(ku["key"][int(ku["key_off"][i]):int(ku["key_off"][i + 1])].tolist())
            ko.append(len(key)); ro.append(len(rs))
        for i in range(len(rp["msb"])):
            xm.append(rp["msb"][i]); xl.append(rp["lsb"][i]); xn.append(rp["node"][i])
            if int(rp["lsb"][i]) & 1:
                a, b = int(rp["rng_off"][i]), int(rp["rng_off"][i + 1])
                rs.extend(rp["rng_start"][a:b].tolist()); re_.extend(rp["rng_end"][a:b].tolist())
            ko.append(len(key)); ro.append(len(rs))
    return dict(end_inclusive=ei, xmsb=np.array(xm, np.uint64), xlsb=np.array(xl, np.uint64), xnode=np.array(xn, np.int32),
                key_off=np.array(ko, np.uint32), key=np.array(key, np.uint64), rng_off=np.array(ro, np.uint32),
                rng_start=np.array(rs, np.uint64), rng_end=np.array(re_, np.uint64))
