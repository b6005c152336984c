"""CommandsForKey.notify over a key-major CommandsForKey state, restated in plain Python — TEST INFRASTRUCTURE.

model(): a literal transliteration of the CommandsForKey constructor's derived fields (local/CommandsForKey.java:422-470)
and of notify(safeStore, kinds, start, end) (:1512-1635) called as notify(AnyGloballyVisible, 0, committed.length): the
loops, the stable sort of committed[], the moving uncommittedIndex with its backfill, and the FAST searches of
utils/SortedArrays.java (binarySearch :993-1027, exponentialSearch :898-934). It is the independent statement that
acc_cfk_notify's closed form is checked against; closed_form() restates that closed form (include/accord_amd.h) in numpy
and test_cfk_notify_model.py checks the two against each other.

Both take the state layout of oracle.cfk_apply / CfkStore.state() and return the dict CfkStore.notify returns (without
ev_txn / rel_keys when with_view is False), plus, for the case conditions, per event `ev_expect` and `ev_missing`
(expectMissingCount and missingCount of a release, 0 for WAITING_TO_EXECUTE) and `held` (entries STABLE and not released).
"""
from __future__ import annotations

import numpy as np

IDENT = 0xFFFFFFFFFFFF001E    # the lsb bits Timestamp.compareTo / equals read
TK, HIST, PRE, ACC, COMMITTED, STABLE, APPLIED, INVALID = range(8)
READ, WRITE, EPHEMERAL_READ, SYNC_POINT, EXCLUSIVE_SYNC_POINT, LOCAL_ONLY = range(6)
WAITING_TO_EXECUTE, RELEASE = 0, 1
NONE = 0xFFFFFFFF


class IllegalState(Exception):
    """the reference's illegalState("Invalid Txn.Kind for CommandsForKey: ...")"""


def order(m, l, n):
    return (int(m), int(l) & IDENT, int(n))


def compare(a, b):
    return -1 if a < b else 1 if a > b else 0


class TxnInfo:
    __slots__ = ("entry", "id", "status", "execute_at", "missing", "kind")

    def __init__(self, entry, tid, status, execute_at, missing, kind):
        self.entry, self.id, self.status, self.execute_at, self.missing, self.kind = entry, tid, status, execute_at, missing, kind


def key_infos(state, k):
    eo, mo = state["ent_off"], state["miss_off"]
    out = []
    for e in range(int(eo[k]), int(eo[k + 1])):
        miss = [order(state["mmsb"][j], state["mlsb"][j], state["mnode"][j]) for j in range(int(mo[e]), int(mo[e + 1]))]
        out.append(TxnInfo(e, order(state["emsb"][e], state["elsb"][e], state["enode"][e]), int(state["status"][e]),
                           order(state["xmsb"][e], state["xlsb"][e], state["xnode"][e]), miss, (int(state["elsb"][e]) >> 1) & 7))
    return out


# ---------------------------------------------------------------- utils/SortedArrays.java, Search.FAST

def binary_search(a, frm, to, find, comparator):
    while frm < to:
        i = (frm + to) >> 1
        c = comparator(find, a[i])
        if c < 0:
            to = i
        elif c > 0:
            frm = i + 1
        else:
            return i
    return -1 - to


def exponential_search(a, frm, to, find, comparator):
    step = 0
    while frm + step < to:
        i = frm + step
        c = comparator(find, a[i])
        if c < 0:
            to = i
            break
        if c > 0:
            frm = i + 1
        else:
            return i
        step = step * 2 + 1
    return binary_search(a, frm, to, find, comparator)


# ---------------------------------------------------------------- CommandsForKey.java:422-470

class Cfk:
    def __init__(self, txns):
        self.txns = txns
        min_uncommitted = next_write = nxt = None
        count_committed = 0
        for txn in txns:
            if txn.status == INVALID:
                continue
            if txn.status >= COMMITTED:
                if txn.status < APPLIED:
                    if txn.kind == WRITE and (next_write is None or compare(next_write.execute_at, txn.execute_at) > 0):
                        next_write = txn
                    if nxt is None or compare(nxt.execute_at, txn.execute_at) > 0:
                        nxt = txn
                count_committed += 1
            elif min_uncommitted is None:
                min_uncommitted = txn
        if min_uncommitted is not None:
            if nxt is not None and compare(min_uncommitted.id, nxt.execute_at) < 0:
                nxt = None
            if next_write is not None and compare(min_uncommitted.id, next_write.execute_at) < 0:
                next_write = None
        self.min_uncommitted, self.next_write, self.next = min_uncommitted, next_write, nxt
        committed = [None] * count_committed
        count_committed = 0
        for txn in txns:
            if txn.status >= COMMITTED and txn.status != INVALID:
                committed[count_committed] = txn
                count_committed += 1
        committed.sort(key=lambda c: c.execute_at)   # Arrays.sort on objects: a stable merge sort
        self.committed = committed

    # ------------------------------------------------------------ :1512-1635
    def notify(self, kinds, start, end):
        """events [(TxnInfo, kind, index in committed[], expectMissingCount, missingCount)] in the order the reference
        makes its calls, and the STABLE entries it holds"""
        txns, committed, min_uncommitted = self.txns, self.committed, self.min_uncommitted
        events, held = [], []
        uncommitted_index = len(txns) if min_uncommitted is None else -1
        unapplied_read = unapplied_write = unapplied_sync = 0
        for i in range(start, end):
            txn = committed[i]
            kind = txn.kind
            if txn.status in (APPLIED, INVALID):
                continue
            if txn.status == COMMITTED:
                if kind in kinds:
                    events.append((txn, WAITING_TO_EXECUTE, i, 0, 0))
            elif txn.status == STABLE:
                if uncommitted_index < 0:
                    uncommitted_index = binary_search(txns, 0, len(txns), min_uncommitted.id, lambda f, v: compare(f, v.id))
                next_uncommitted_index = exponential_search(txns, uncommitted_index, len(txns), txn.execute_at,
                                                            lambda f, v: compare(f, v.id))
                if next_uncommitted_index < 0:
                    next_uncommitted_index = -1 - next_uncommitted_index
                while uncommitted_index < next_uncommitted_index:
                    backfill = txns[uncommitted_index]
                    uncommitted_index += 1
                    if backfill.status >= COMMITTED:
                        continue
                    if backfill.kind in (LOCAL_ONLY, EPHEMERAL_READ):
                        raise IllegalState(backfill.kind)
                    elif backfill.kind == WRITE:
                        unapplied_write += 1
                    elif backfill.kind == READ:
                        unapplied_read += 1
                    elif backfill.kind in (SYNC_POINT, EXCLUSIVE_SYNC_POINT):
                        unapplied_sync += 1
                    else:
                        raise AssertionError(backfill.kind)
                expect = 0
                if kind in (LOCAL_ONLY, EPHEMERAL_READ):
                    raise IllegalState(kind)
                if kind in (SYNC_POINT, EXCLUSIVE_SYNC_POINT):     # the switch falls through
                    expect += unapplied_sync
                if kind in (SYNC_POINT, EXCLUSIVE_SYNC_POINT, WRITE):
                    expect += unapplied_read
                expect += unapplied_write
                missing = txn.missing
                missing_count = len(missing)
                if missing_count > 0 and min_uncommitted is not None:
                    missing_from = binary_search(missing, 0, len(missing), min_uncommitted.id, compare)
                    if missing_from < 0:
                        missing_from = -1 - missing_from
                    missing_count -= missing_from
                if expect == missing_count:
                    events.append((txn, RELEASE, i, expect, missing_count))
                else:
                    held.append(txn)
            if kind in (LOCAL_ONLY, EPHEMERAL_READ):
                raise IllegalState(kind)
            elif kind == WRITE:
                unapplied_write += 1
            elif kind == READ:
                unapplied_read += 1
            elif kind in (SYNC_POINT, EXCLUSIVE_SYNC_POINT):
                unapplied_sync += 1
            else:
                raise AssertionError(kind)
        return events, held


ANY_GLOBALLY_VISIBLE = (READ, WRITE, SYNC_POINT, EXCLUSIVE_SYNC_POINT)


# ---------------------------------------------------------------- the result layout

def _rows(state, keys):
    codes = [int(c) for c in state["key"]]
    if keys is None:
        return np.asarray(state["key"], np.uint64), list(range(len(codes)))
    at = {c: k for k, c in enumerate(codes)}
    return np.asarray(keys, np.uint64), [at.get(int(c)) for c in keys]


def view_index(state):
    """entry -> its txn's index in the store's txn-major view (the distinct TxnIds in order)"""
    ids = [order(m, l, n) for m, l, n in zip(state["emsb"], state["elsb"], state["enode"])]
    rank = {t: i for i, t in enumerate(sorted(set(ids)))}
    return np.array([rank[t] for t in ids], np.uint32), len(rank)


def _pack(state, key, rows, with_view):
    """rows: per asked key None or (min_uncommitted, next, next_write, [(entry, kind, pos, expect, missing)], [held])"""
    ent = lambda v: NONE if v is None else v  # noqa: E731
    mu, nx, nw, off, ev, held = [], [], [], [0], [], []
    for r in rows:
        if r is None:
            r = (None, None, None, [], [])
        mu.append(ent(r[0])); nx.append(ent(r[1])); nw.append(ent(r[2]))
        ev.extend(sorted(r[3]))     # TxnId order within the row = entry order
        held.extend(r[4])
        off.append(len(ev))
    col = lambda i, dt: np.array([e[i] for e in ev], dt)  # noqa: E731
    out = dict(key=key, min_uncommitted=np.array(mu, np.uint32), next=np.array(nx, np.uint32), next_write=np.array(nw, np.uint32),
               ev_off=np.array(off, np.uint64), ev_entry=col(0, np.uint32), ev_kind=col(1, np.uint8), ev_pos=col(2, np.uint32),
               ev_expect=col(3, np.int64), ev_missing=col(4, np.int64), held=np.array(sorted(held), np.uint32))
    if with_view:
        vi, n = view_index(state)
        out["ev_txn"] = vi[out["ev_entry"].astype(np.int64)] if len(ev) else np.zeros(0, np.uint32)
        rel = np.zeros(n, np.uint32)
        np.add.at(rel, out["ev_txn"][out["ev_kind"] == RELEASE].astype(np.int64), 1)
        out["rel_keys"] = rel
    return out


def model(state, keys=None, with_view=True):
    key, at = _rows(state, keys)
    rows = []
    for k in at:
        if k is None:
            rows.append(None)
            continue
        cfk = Cfk(key_infos(state, k))
        events, held = cfk.notify(ANY_GLOBALLY_VISIBLE, 0, len(cfk.committed))
        e = lambda t: None if t is None else t.entry  # noqa: E731
        rows.append((e(cfk.min_uncommitted), e(cfk.next), e(cfk.next_write),
                     [(t.entry, kind, pos, ex, mc) for t, kind, pos, ex, mc in events], [t.entry for t in held]))
    return _pack(state, key, rows, with_view)


# ---------------------------------------------------------------- the closed form (include/accord_amd.h, acc_cfk_notify)

def closed_form(state, keys=None, with_view=True):
    key, at = _rows(state, keys)
    eo, mo = state["ent_off"].astype(np.int64), state["miss_off"].astype(np.int64)
    rows = []
    for k in at:
        if k is None:
            rows.append(None)
            continue
        e0, e1 = int(eo[k]), int(eo[k + 1])
        n = e1 - e0
        ids = [order(state["emsb"][e], state["elsb"][e], state["enode"][e]) for e in range(e0, e1)]
        xs = [order(state["xmsb"][e], state["xlsb"][e], state["xnode"][e]) for e in range(e0, e1)]
        miss = [order(m, l, nd) for m, l, nd in zip(state["mmsb"][mo[e0]:mo[e1]], state["mlsb"][mo[e0]:mo[e1]],
                                                    state["mnode"][mo[e0]:mo[e1]])]
        rank = {t: i for i, t in enumerate(sorted(set(ids) | set(xs) | set(miss)))}     # timestamps as dense integers
        idr = np.array([rank[t] for t in ids], np.int64)
        xr = np.array([rank[t] for t in xs], np.int64)
        mr = np.array([rank[t] for t in miss], np.int64)
        st = state["status"][e0:e1].astype(np.int64)
        kind = (state["elsb"][e0:e1].astype(np.uint64) >> np.uint64(1)).astype(np.int64) & 7
        if np.any((kind == EPHEMERAL_READ) | (kind == LOCAL_ONLY)):
            raise IllegalState(int(kind[(kind == EPHEMERAL_READ) | (kind == LOCAL_ONLY)][0]))
        cls = np.where(kind == WRITE, 0, np.where(kind == READ, 1, 2))                  # W, R, S
        unc = st < COMMITTED
        com = (st >= COMMITTED) & (st <= APPLIED)
        live = com & (st != APPLIED)
        mu = int(np.flatnonzero(unc)[0]) if unc.any() else None
        ci = np.flatnonzero(com)
        ci = ci[np.lexsort((ci, xr[ci]))]                                               # executeAt, ties in TxnId order
        pos = np.full(n, -1, np.int64)
        pos[ci] = np.arange(len(ci))

        def least(sel):
            c = ci[sel[ci]]
            if not len(c):
                return None
            t = int(c[0])
            return None if mu is not None and idr[mu] < xr[t] else t
        nx, nw = least(live), least(live & (cls == 0))
        # c[.]: the unapplied committed-class entries before T in committed[]; u[.]: the uncommitted ids below X
        cnt = np.zeros((3, n), np.int64)
        for c in range(3):
            f = (live & (cls == c))[ci].astype(np.int64)
            cnt[c, ci] = np.cumsum(f) - f
            pu = np.concatenate([[0], np.cumsum((unc & (cls == c)).astype(np.int64))])
            cnt[c] += pu[np.searchsorted(idr, xr, side="left")]
        expect = cnt[0] + np.where(cls != 1, cnt[1], 0) + np.where(cls == 2, cnt[2], 0)
        mlen = np.diff(mo[e0:e1 + 1])
        mcount = mlen.copy()
        if mu is not None:
            for t in np.flatnonzero(mlen > 0):
                a = int(mo[e0 + t] - mo[e0])
                mcount[t] -= int(np.searchsorted(mr[a:a + int(mlen[t])], idr[mu], side="left"))
        rel = (st == STABLE) & (expect == mcount)
        events = [(e0 + int(t), WAITING_TO_EXECUTE, int(pos[t]), 0, 0) for t in np.flatnonzero(st == COMMITTED)]
        events += [(e0 + int(t), RELEASE, int(pos[t]), int(expect[t]), int(mcount[t])) for t in np.flatnonzero(rel)]
        g = lambda t: None if t is None else e0 + t  # noqa: E731
        rows.append((g(mu), g(nx), g(nw), events, [e0 + int(t) for t in np.flatnonzero((st == STABLE) & ~rel)]))
    return _pack(state, key, rows, with_view)


FIELDS = ("key", "min_uncommitted", "next", "next_write", "ev_off", "ev_entry", "ev_kind", "ev_pos")
VIEW_FIELDS = ("ev_txn", "rel_keys")
