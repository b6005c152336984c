"""CommandsForKey's Unmanaged pending records over a key-major CommandsForKey state, in plain Python — TEST
INFRASTRUCTURE.

A literal transliteration of local/CommandsForKey.java: Unmanaged.compareTo (:155-162), registerUnmanaged (:1406-1498),
updatePending (:1333-1388), findPendingCommit / findPendingApply (:1390-1404, SortedArrays.binarySearch with CEIL,
utils/SortedArrays.java:993-1027) and both arms of notifyUnmanaged (:1270-1316), called as the tail of
notifyAndUpdatePending calls them (:1206-1212) with the COMMIT arm run unconditionally. Each key's pending array is kept
sorted as the Java keeps it (SortedArrays.insert, Arrays.sort + linearUnion), and a batch of waiters is registered pair by
pair in array order, each pair seeing the TRANSITIVELY_KNOWN entries the pairs before it inserted. It is the independent
statement that acc_cfk_register_unmanaged (all pairs evaluated at once, then one insertion) and acc_cfk_notify_unmanaged
(per-record predicates over an unsorted table) are checked against.

Model works on the layout of CfkStore.state(); minUncommitted and next come from cfk_notify_model.Cfk.
"""
from __future__ import annotations

import numpy as np

import cfk_notify_model as NM
from cfk_notify_model import APPLIED, COMMITTED, compare, order

COMMIT, APPLY = 0, 1                                  # Unmanaged.Pending
READY, PENDING_COMMIT, PENDING_APPLY = 0, 1, 2        # what registerUnmanaged did with a pair
EV_TO_APPLY, EV_RELEASE = 0, 1
TK = 0
ZERO = (0, 0, 0)
MAX = (1 << 64, 0, 0)                                 # Timestamp.MAX: above every order() tuple


class IllegalState(Exception):
    """the reference's illegalState("Transaction not found: ...")"""


def awaits_only_deps(raw_id):
    """Txn.Kind.awaitsOnlyDeps (primitives/Txn.java:211-214)"""
    return (int(raw_id[1]) >> 1) & 7 in (NM.EXCLUSIVE_SYNC_POINT, NM.EPHEMERAL_READ)


class Info(NM.TxnInfo):
    """a TxnInfo that also keeps the raw bits of its TxnId and executeAt"""

    def __init__(self, raw_id, status, raw_x, missing):
        super().__init__(None, order(*raw_id), status, order(*raw_x), missing, (int(raw_id[1]) >> 1) & 7)
        self.raw_id, self.raw_x = tuple(int(v) for v in raw_id), tuple(int(v) for v in raw_x)


class Unmanaged:
    def __init__(self, pending, txn_id, waiting_until, execute_at=None, deps=None):
        """txn_id, waiting_until, execute_at: raw (msb, lsb, node); deps: the waiter's raw dep list for the key (what the
        Java reads back from the Command when it re-evaluates a COMMIT record)"""
        self.pending, self.txn_id, self.waiting_until = pending, tuple(txn_id), tuple(waiting_until)
        self.execute_at, self.deps = execute_at, deps

    def compare_to(self, that):
        if self.pending != that.pending:
            return -1 if self.pending == COMMIT else 1
        c = compare(order(*self.waiting_until), order(*that.waiting_until))
        if c == 0:
            c = compare(order(*self.txn_id), order(*that.txn_id))
        return c

    def sort_key(self):
        return (self.pending, order(*self.waiting_until), order(*self.txn_id))

    def row(self):
        return (self.pending, self.waiting_until, self.txn_id, self.execute_at,
                tuple(self.deps) if self.pending == COMMIT else ())


def binary_search_ceil(a, frm, to, find, comparator):
    """SortedArrays.binarySearch(..., CEIL): the lowest matching index, else -1 - insertPos"""
    found = -1
    while frm < to:
        i = (frm + to) >> 1
        c = comparator(find, a[i])
        if c < 0:
            to = i
        elif c > 0:
            frm = i + 1
        else:
            to = found = i
    return found if found >= 0 else -1 - to


def sorted_insert(a, v):
    """SortedArrays.insert: v at its place in the sorted array"""
    i = NM.binary_search(a, 0, len(a), v, lambda f, x: f.compare_to(x))
    if i >= 0:
        raise AssertionError("the record is already pending")
    i = -1 - i
    return a[:i] + [v] + a[i:]


class Cfk:
    """one key's CommandsForKey: txns (Info, TxnId order), unmanageds (sorted), shardRedundantBefore"""

    def __init__(self, key, txns, unmanageds, redundant_before=ZERO):
        self.key, self.txns, self.unmanageds, self.redundant_before = key, txns, unmanageds, redundant_before

    # ------------------------------------------------------------ :1406-1498
    def register_unmanaged(self, txn_id, execute_at, txn_ids):
        """-> (the new Cfk, outcome, waiting_until raw or ZERO, [inserted raw TxnIds])"""
        txns = self.txns
        waiting_execute_at = order(*execute_at)
        ids = [order(*t) for t in txn_ids]
        missing = []
        i = NM.binary_search(ids, 0, len(ids), self.redundant_before, compare)
        if i < 0:
            i = -1 - i
        if i < len(ids):
            ready_to_execute = waiting_to_apply = True
            executes_at = None
            j = NM.binary_search(txns, 0, len(txns), ids[i], lambda f, v: compare(f, v.id))
            if j < 0:
                j = -1 - j
            while i < len(ids):
                c = -1 if j == len(txns) else compare(ids[i], txns[j].id)
                if c == 0:
                    txn = txns[j]
                    if txn.status < COMMITTED:
                        ready_to_execute = waiting_to_apply = False
                    elif awaits_only_deps(txn_id) or compare(txn.execute_at, waiting_execute_at) < 0:
                        ready_to_execute &= txn.status >= APPLIED
                        executes_at = non_null_or_max(executes_at, txn)
                    i += 1
                    j += 1
                elif c > 0:
                    j += 1
                else:
                    ready_to_execute = waiting_to_apply = False
                    missing.append(txn_ids[i])
                    i += 1
            if not ready_to_execute:
                new_txns = txns
                if missing:
                    new_txns = []
                    i = j = 0
                    while i < len(missing) and j < len(txns):
                        if compare(order(*missing[i]), txns[j].id) < 0:
                            new_txns.append(Info(missing[i], TK, missing[i], []))
                            i += 1
                        else:
                            new_txns.append(txns[j])
                            j += 1
                    while i < len(missing):
                        new_txns.append(Info(missing[i], TK, missing[i], []))
                        i += 1
                    while j < len(txns):
                        new_txns.append(txns[j])
                        j += 1
                if waiting_to_apply:
                    record = Unmanaged(APPLY, txn_id, executes_at.raw_x)
                    outcome = PENDING_APPLY
                else:
                    record = Unmanaged(COMMIT, txn_id, txn_ids[-1], tuple(execute_at), [tuple(t) for t in txn_ids])
                    outcome = PENDING_COMMIT
                new_pending = sorted_insert(self.unmanageds, record)
                return Cfk(self.key, new_txns, new_pending, self.redundant_before), outcome, record.waiting_until, missing
        return self, READY, ZERO, []       # removeWaitingOn

    # ------------------------------------------------------------ :1333-1388
    def update_pending(self, rec):
        """-> the APPLY record that replaces rec, or None (removeWaitingOn)"""
        waiting_execute_at = order(*rec.execute_at)
        ids = [order(*t) for t in rec.deps]
        txns = self.txns
        i = NM.binary_search(ids, 0, len(ids), self.redundant_before, compare)
        if i < 0:
            i = -1 - i
        if i < len(ids):
            ready_to_execute = True
            executes_at = None
            j = NM.binary_search(txns, 0, len(txns), ids[i], lambda f, v: compare(f, v.id))
            if j < 0:
                j = -1 - j
            while i < len(ids) and j < len(txns):
                c = compare(ids[i], txns[j].id)
                if c > 0:
                    j += 1
                elif c < 0:
                    raise IllegalState("Transaction not found")
                else:
                    txn = txns[j]
                    if awaits_only_deps(rec.txn_id) or compare(txn.execute_at, waiting_execute_at) < 0:
                        ready_to_execute &= txn.status >= APPLIED
                        executes_at = non_null_or_max(executes_at, txn)
                    i += 1
                    j += 1
            if not ready_to_execute:
                return Unmanaged(APPLY, rec.txn_id, executes_at.raw_x)
        return None

    # ------------------------------------------------------------ :1206-1212, 1270-1316
    def notify_and_update_pending(self):
        """-> (the new Cfk, events [(kind, flags, raw txn_id, raw until)] in the order the reference acts)"""
        derived = NM.Cfk(self.txns)
        mu, nxt = derived.min_uncommitted, derived.next
        events = []
        pending = self.unmanageds
        # COMMIT (run unconditionally: without a new commit no record lies below minUncommitted)
        ts = MAX if mu is None else mu.id
        end = binary_search_ceil(pending, 0, len(pending), ts,
                                 lambda f, v: -1 if v.pending == APPLY else compare(f, order(*v.waiting_until)))
        if end < 0:
            end = -1 - end
        add = []
        for i in range(end):
            upd = self.update_pending(pending[i])
            if upd is not None:
                add.append(upd)
                events.append([EV_TO_APPLY, 1, upd.txn_id, upd.waiting_until])
            else:
                events.append([EV_RELEASE, 1, pending[i].txn_id, ZERO])
        add.sort(key=Unmanaged.sort_key)
        pending = linear_union(pending[end:], add)
        # APPLY
        if mu is None or nxt is not None:
            ts = MAX if nxt is None else nxt.execute_at
            start = -1 - NM.binary_search(pending, 0, len(pending), ts, lambda f, v: -1 if v.pending == APPLY else 1)
            end = binary_search_ceil(pending, 0, len(pending), ts,
                                     lambda f, v: 1 if v.pending == COMMIT else compare(f, order(*v.waiting_until)))
            if end < 0:
                end = -1 - end
            if start != end:
                for i in range(start, end):
                    rec = pending[i]
                    mine = [e for e in events if e[0] == EV_TO_APPLY and e[2] == rec.txn_id]
                    if mine:       # moved to APPLY and released in one call: one event, as the device reports it
                        mine[0][0] = EV_RELEASE
                    else:
                        events.append([EV_RELEASE, 0, rec.txn_id, rec.waiting_until])
                pending = pending[:start] + pending[end:]
        return Cfk(self.key, self.txns, pending, self.redundant_before), [tuple(e) for e in events]


def non_null_or_max(a, b):
    """Timestamp.nonNullOrMax over the TxnInfos' executeAts: max(a, b) = a.compareTo(b) >= 0 ? a : b"""
    if a is None:
        return b
    return a if compare(a.execute_at, b.execute_at) >= 0 else b


def linear_union(a, b):
    out, i, j = [], 0, 0
    while i < len(a) and j < len(b):
        c = a[i].compare_to(b[j])
        if c <= 0:
            out.append(a[i])
            i += 1
            j += c == 0
        else:
            out.append(b[j])
            j += 1
    return out + a[i:] + b[j:]


# ---------------------------------------------------------------- a store of them

class Store:
    """key code -> Cfk, with the RedundantBefore map as anything with get(key code) -> raw bound
    (cfk_redundant_model.BoundMap)"""

    def __init__(self, state=None, bounds=None):
        self.cfks = {}
        self.bounds = bounds
        if state is not None:
            self.load(state)

    def bound(self, code):
        return ZERO if self.bounds is None else order(*self.bounds.get(code))

    def load(self, state):
        """the txns of every key replaced by the state's (the records stay)"""
        old = {c: k.unmanageds for c, k in self.cfks.items()}
        self.cfks = {}
        eo, mo = state["ent_off"], state["miss_off"]
        for k, code in enumerate(int(c) for c in state["key"]):
            txns = []
            for e in range(int(eo[k]), int(eo[k + 1])):
                miss = [order(state["mmsb"][j], state["mlsb"][j], state["mnode"][j]) for j in range(int(mo[e]), int(mo[e + 1]))]
                inf = Info((state["emsb"][e], state["elsb"][e], state["enode"][e]), int(state["status"][e]),
                           (state["xmsb"][e], state["xlsb"][e], state["xnode"][e]), miss)
                inf.raw_missing = [(int(state["mmsb"][j]), int(state["mlsb"][j]), int(state["mnode"][j]))
                                   for j in range(int(mo[e]), int(mo[e + 1]))]
                txns.append(inf)
            self.cfks[code] = Cfk(code, txns, old.pop(code, []), self.bound(code))
        for code, recs in old.items():      # a key that left the state keeps its records on an empty CommandsForKey
            if recs:
                self.cfks[code] = Cfk(code, [], recs, self.bound(code))

    def set_bounds(self, bounds):
        self.bounds = bounds
        for c in self.cfks.values():
            c.redundant_before = self.bound(c.key)

    def state(self):
        cols = {k: [] for k in ("emsb", "elsb", "enode", "xmsb", "xlsb", "xnode", "status", "mmsb", "mlsb", "mnode")}
        key, ent_off, miss_off = [], [0], [0]
        for code in sorted(self.cfks):
            txns = self.cfks[code].txns
            if not txns:
                continue
            for t in txns:
                for k, v in zip(("emsb", "elsb", "enode", "xmsb", "xlsb", "xnode", "status"), t.raw_id + t.raw_x + (t.status,)):
                    cols[k].append(v)
                for m in getattr(t, "raw_missing", []):
                    for k, v in zip(("mmsb", "mlsb", "mnode"), m):
                        cols[k].append(v)
                miss_off.append(len(cols["mmsb"]))
            key.append(code)
            ent_off.append(len(cols["emsb"]))
        dt = dict(emsb=np.uint64, elsb=np.uint64, enode=np.int32, xmsb=np.uint64, xlsb=np.uint64, xnode=np.int32,
                  status=np.uint8, mmsb=np.uint64, mlsb=np.uint64, mnode=np.int32)
        out = {k: np.array(v, dt[k]) for k, v in cols.items()}
        out.update(key=np.array(key, np.uint64), ent_off=np.array(ent_off, np.uint32), miss_off=np.array(miss_off, np.uint32))
        return out

    def register(self, waiters, reverse=False):
        """pair by pair in array order (reverse: in reversed order; the results stay in array order)
        -> dict(outcome, until [raw], n_inserted)"""
        w = waiters
        pairs = []
        for i in range(len(w["msb"])):
            tid = (int(w["msb"][i]), int(w["lsb"][i]), int(w["node"][i]))
            ex = (int(w["xmsb"][i]), int(w["xlsb"][i]), int(w["xnode"][i]))
            for j in range(int(w["key_off"][i]), int(w["key_off"][i + 1])):
                d0, d1 = int(w["dep_off"][j]), int(w["dep_off"][j + 1])
                deps = [(int(w["dmsb"][d]), int(w["dlsb"][d]), int(w["dnode"][d])) for d in range(d0, d1)]
                pairs.append((j, tid, ex, int(w["key"][j]), deps))
        outcome, until, inserted = [None] * len(pairs), [None] * len(pairs), 0
        for j, tid, ex, code, deps in (reversed(pairs) if reverse else pairs):
            cfk = self.cfks.get(code) or Cfk(code, [], [], self.bound(code))
            cfk, outcome[j], until[j], ins = cfk.register_unmanaged(tid, ex, deps)
            inserted += len(ins)
            if cfk.txns or cfk.unmanageds:
                self.cfks[code] = cfk
        return dict(outcome=np.array(outcome, np.uint8), until=until, n_inserted=inserted)

    def notify(self, keys=None):
        """-> events [(kind, flags, key code, raw txn_id, raw until)]"""
        codes = sorted(c for c, k in self.cfks.items() if k.unmanageds) if keys is None else [int(c) for c in keys]
        events = []
        for code in codes:
            cfk = self.cfks.get(code)
            if cfk is None:
                continue
            self.cfks[code], ev = cfk.notify_and_update_pending()
            events += [(k, f, code, t, u) for k, f, t, u in ev]
        return events

    def records(self):
        """{key code: [Unmanaged.row()] in compareTo order}"""
        return {code: [r.row() for r in c.unmanageds] for code, c in self.cfks.items() if c.unmanageds}


# ---------------------------------------------------------------- the device's results in the same terms

def device_records(t):
    """CfkStore.unmanaged() -> {key code: [rows] sorted by Unmanaged.compareTo}"""
    out = {}
    for r in range(len(t["key"])):
        d0, d1 = int(t["dep_off"][r]), int(t["dep_off"][r + 1])
        u = Unmanaged(int(t["pending"][r]), (int(t["msb"][r]), int(t["lsb"][r]), int(t["node"][r])),
                      (int(t["until_msb"][r]), int(t["until_lsb"][r]), int(t["until_node"][r])),
                      (int(t["xmsb"][r]), int(t["xlsb"][r]), int(t["xnode"][r])),
                      [(int(t["dmsb"][d]), int(t["dlsb"][d]), int(t["dnode"][d])) for d in range(d0, d1)])
        out.setdefault(int(t["key"][r]), []).append(u)
    return {code: [u.row() for u in sorted(v, key=Unmanaged.sort_key)] for code, v in out.items()}


def comparable(rec):
    """records() / device_records() without an APPLY record's executeAt (the Java record has none; the table keeps the
    column for every record)"""
    return {code: [(p, u, t, None if p == APPLY else x, d) for p, u, t, x, d in rows] for code, rows in rec.items()}


def device_events(ev):
    """CfkStore.notify_unmanaged() -> the sorted multiset of (kind, flags, key, txn, until)"""
    return sorted((int(ev["ev_kind"][i]), int(ev["ev_flags"][i]), int(ev["ev_key"][i]),
                   (int(ev["ev_txn_msb"][i]), int(ev["ev_txn_lsb"][i]), int(ev["ev_txn_node"][i])),
                   (int(ev["ev_until_msb"][i]), int(ev["ev_until_lsb"][i]), int(ev["ev_until_node"][i])))
                  for i in range(len(ev["ev_kind"])))
