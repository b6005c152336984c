"""Command.WaitingOn and the Commands methods that advance it, in plain Python — TEST INFRASTRUCTURE.

A literal restatement of local/Command.java:1402-1609 (WaitingOn.Update over two Python-int bitsets: waitingOn holds the
txnIds in bits [0, n_dep) and the keys in bits [n_dep, n_dep + n_key); appliedOrInvalidated is None for a key-domain
command) and of local/Commands.java: initialiseWaitingOn (:735-753), updateWaitingOn (:755-830),
updateDependencyAndMaybeExecute (:832-857), removeWaitingOnKeyAndMaybeExecute (:859-876). It is independent of the
library: acc_waiting_* (three-state bytes, worklists, two kernel tiers) is checked against it.

Conventions the header of the library documents and this model states on its own:
  * a dependency is looked up in `rcmd`, a dict order(TxnId) -> (status ordinal, raw executeAt); absent or status < 4 is
    ifLoadedAndInitialised == null / not hasBeen(PreCommitted);
  * known().executeAt == ExecuteAtKnown is 4 <= status <= 9 with a non-zero executeAt;
  * forEachWaitingOnId visits every waiting bit below n_dep once, descending, the set mutating under it (the single-word
    path of SimpleBitSet.reverseForEach(from, to), utils/SimpleBitSet.java:389-420; its multi-word path indexes every
    word with fromIndex and is not followed);
  * dependency.asCommitted().waitingOn() of an Applied dependency is read from the store as the call found it, and an
    Applied dependency whose own record still waits is an IllegalState that leaves the store unchanged.
"""
from __future__ import annotations

import numpy as np

IDENTITY_LSB = 0xFFFFFFFFFFFF001E
NOT_WAITING, WAITING, APPLIED_OR_INVALIDATED = 0, 1, 2
AWAITS_ONLY_DEPS, RANGE_DOMAIN = 1, 2
NONE = 0xFFFFFFFF
ZERO = (0, 0, 0)
PRE_COMMITTED, APPLIED, TRUNCATED = 4, 8, 9
EPHEMERAL_READ, EXCLUSIVE_SYNC_POINT = 2, 4


class IllegalState(Exception):
    pass


class IllegalArgument(Exception):
    pass


def order(ts):
    """Timestamp.compareTo as a tuple (primitives/Timestamp.java:208-217)"""
    return (int(ts[0]), int(ts[1]) & IDENTITY_LSB, int(ts[2]))


def raw(ts):
    return (int(ts[0]), int(ts[1]), int(ts[2]))


def kind_of(ts):
    return (int(ts[1]) >> 1) & 7


def awaits_only_deps(ts):
    """Txn.Kind.awaitsOnlyDeps (primitives/Txn.java:211-214)"""
    return kind_of(ts) in (EXCLUSIVE_SYNC_POINT, EPHEMERAL_READ)


def is_range_domain(ts):
    return bool(int(ts[1]) & 1)


class WaitingOn:
    """Command.WaitingOn (+ WaitingOnWithExecuteAt): immutable between updates"""

    def __init__(self, txn_id, execute_at, keys, txn_ids, waiting_on, applied, execute_at_least=None):
        self.txn_id, self.execute_at = raw(txn_id), raw(execute_at)
        self.keys, self.txn_ids = list(keys), [raw(t) for t in txn_ids]
        self.waiting_on, self.applied, self.execute_at_least = waiting_on, applied, execute_at_least

    def is_waiting(self):
        return self.waiting_on != 0

    def next_waiting_on(self):
        """prevSetBit(txnIds.size()) (:1359-1363)"""
        low = self.waiting_on & ((1 << len(self.txn_ids)) - 1)
        return low.bit_length() - 1 if low else NONE


class Update:
    """Command.WaitingOn.Update (:1402-1609)"""

    def __init__(self, w: WaitingOn):
        self.keys, self.txn_ids = w.keys, w.txn_ids
        self.waiting_on, self.applied, self.execute_at_least = w.waiting_on, w.applied, w.execute_at_least
        self.propagated = 0

    def index_of(self, txn_id):
        o = order(txn_id)
        for i, t in enumerate(self.txn_ids):
            if order(t) == o:
                return i
        return -1

    def remove_waiting_on(self, i):                       # :1525-1537
        if (self.waiting_on >> i) & 1:
            self.waiting_on &= ~(1 << i)
            return True
        return False

    def remove_waiting_on_key(self, k):                   # :1520-1523
        return self.remove_waiting_on(len(self.txn_ids) + k)

    def update_execute_at_least(self, x):                 # :1510-1513, Timestamp.nonNullOrMax(x, this): x on a tie
        cur = self.execute_at_least
        self.execute_at_least = raw(x) if cur is None or order(x) >= order(cur) else cur

    def set_applied_or_invalidated(self, i):              # :1552-1566
        if self.applied is None:
            return self.remove_waiting_on(i)
        if (self.applied >> i) & 1:
            return False
        if not self.remove_waiting_on(i):
            return False
        self.applied |= 1 << i
        return True

    def set_applied_and_propagate(self, i, propagate):    # :1568-1584
        if not self.set_applied_or_invalidated(i):
            return False
        if propagate is not None and propagate.applied is not None and propagate.applied != 0:
            mine = {order(t): j for j, t in enumerate(self.txn_ids)}
            for i1, t in enumerate(propagate.txn_ids):    # forEachIntersection(propagate.txnIds, txnIds)
                i2 = mine.get(order(t))
                if i2 is not None and (propagate.applied >> i1) & 1:
                    if self.set_applied_or_invalidated(i2):
                        self.propagated += 1
                        self.on_propagate(i2)
        return True

    def on_propagate(self, i2):
        pass

    def for_each_waiting_on_id(self, fn, only=None):      # :1586-1589 over the single-word reverseForEach
        mask = (1 << len(self.txn_ids)) - 1
        if only is not None:
            mask &= only
        while True:
            reg = self.waiting_on & mask
            if not reg:
                return
            i = reg.bit_length() - 1
            mask &= (1 << i) - 1
            fn(i)


def branch(w, d, rcmd):
    """the step of evaluate() that dep d of record w takes by its own state: 0, 2, 3, 4 or 5, and whether step 1 fires"""
    row = rcmd.get(order(d))
    if row is None or row[0] < PRE_COMMITTED:
        return 0, False
    status, dx = row
    aod = awaits_only_deps(w.txn_id)
    one = aod and status <= TRUNCATED and raw(dx) != ZERO and order(dx) > order(w.txn_id)
    if status >= TRUNCATED:
        return 2, one
    if order(dx) > order(w.execute_at) and not aod:
        return 3, one
    if status == APPLIED:
        return 4, one
    return 5, one


class Store:
    """the registered commands' WaitingOn, keyed by order(TxnId)"""

    def __init__(self):
        self.recs = {}
        self.trace = {s: 0 for s in range(6)}             # how often each step of evaluate() fired
        self.prop_beyond_own = 0                          # propagated slots whose own branch is step 0 or 5
        self.ready_by = dict(key=0, dep=0, both=0)
        self.stats = {}

    # -- Commands.updateWaitingOn (:776-830) for slot i of `upd`, the update of record w
    def _update_dep(self, w, upd, i, rcmd, snap):
        d = upd.txn_ids[i]
        step, one = branch(w, d, rcmd)
        self.trace[step] += 1
        if step == 0:
            return
        dx = rcmd[order(d)][1]
        if one:
            upd.update_execute_at_least(dx)
            self.trace[1] += 1
        if step == 2:
            upd.set_applied_or_invalidated(i)
        elif step == 3:
            upd.remove_waiting_on(i)
        elif step == 4:
            r = snap.get(order(d))
            if r is not None and r.is_waiting():
                raise IllegalState("an Applied dep's own record is still waiting")

            def seen(i2, w=w, upd=upd):
                if branch(w, upd.txn_ids[i2], rcmd)[0] in (0, 5):
                    self.prop_beyond_own += 1
            upd.on_propagate = seen
            upd.set_applied_and_propagate(i, r)

    def _commit(self, w, upd):
        return WaitingOn(w.txn_id, w.execute_at, w.keys, w.txn_ids, upd.waiting_on, upd.applied, upd.execute_at_least)

    def register(self, waiters: dict, rcmd: dict) -> dict:
        """initialiseWaitingOn for every waiter, each against the store as the call found it"""
        n = len(waiters["msb"])
        snap = dict(self.recs)
        new, seen = {}, set()
        evaluated = propagated = 0
        saved = (dict(self.trace), self.prop_beyond_own)
        try:
            for a in range(n):
                tid = raw((waiters["msb"][a], waiters["lsb"][a], waiters["node"][a]))
                x = raw((waiters["xmsb"][a], waiters["xlsb"][a], waiters["xnode"][a]))
                if order(tid) in seen or order(tid) in snap:
                    raise IllegalArgument("waiter registered twice")
                seen.add(order(tid))
                row = rcmd.get(order(tid))
                if row is not None and row[0] >= APPLIED:
                    raise IllegalState("waiter already applied")
                k0, k1 = int(waiters["key_off"][a]), int(waiters["key_off"][a + 1])
                d0, d1 = int(waiters["dep_off"][a]), int(waiters["dep_off"][a + 1])
                deps = [raw((waiters["dmsb"][j], waiters["dlsb"][j], waiters["dnode"][j])) for j in range(d0, d1)]
                keys = [int(k) for k in waiters["key"][k0:k1]]
                bits = 0
                for j in range(d1 - d0):                  # rangeDeps.forEach(executionParticipants, initialiseWaiting)
                    if waiters.get("dep_wait") is None or int(waiters["dep_wait"][d0 + j]):
                        bits |= 1 << j
                for j in range(k1 - k0):                  # keys inside the store's ranges
                    if waiters.get("key_wait") is None or int(waiters["key_wait"][k0 + j]):
                        bits |= 1 << (len(deps) + j)
                w = WaitingOn(tid, x, keys, deps, bits, 0 if is_range_domain(tid) else None)
                evaluated += bin(bits & ((1 << len(deps)) - 1)).count("1")
                upd = Update(w)
                upd.for_each_waiting_on_id(lambda i, w=w, upd=upd: self._update_dep(w, upd, i, rcmd, snap))
                propagated += upd.propagated
                new[order(tid)] = self._commit(w, upd)
        except (IllegalState, IllegalArgument):
            self.trace, self.prop_beyond_own = saved
            raise
        self.recs.update(new)
        out = [new[order((waiters["msb"][a], waiters["lsb"][a], waiters["node"][a]))] for a in range(n)]
        self.stats = dict(register_evaluated=evaluated, propagated=propagated)
        return dict(waiting=np.array([bin(w.waiting_on).count("1") for w in out], np.uint32),
                    eal=[w.execute_at_least or ZERO for w in out])

    def notify(self, changed, releases, rcmd: dict) -> dict:
        """changed: list of raw TxnIds or None (every waiting slot); releases: list of (txn, key, flags, until)"""
        snap = dict(self.recs)
        cur = dict(self.recs)
        chg = None if changed is None else {order(c) for c in changed}
        slots = propagated = released = ignored = 0
        dep_touched, key_touched = set(), set()
        saved = (dict(self.trace), self.prop_beyond_own)
        try:
            for o in sorted(cur):
                w = cur[o]
                nd = len(w.txn_ids)
                only = None if chg is None else sum(1 << i for i, t in enumerate(w.txn_ids) if order(t) in chg)
                low = w.waiting_on & ((1 << nd) - 1) & (only if only is not None else -1)
                if not low:
                    continue
                slots += bin(low).count("1")
                upd = Update(w)                           # updateDependencyAndMaybeExecute for each, descending
                upd.for_each_waiting_on_id(lambda i, w=w, upd=upd: self._update_dep(w, upd, i, rcmd, snap), only)
                propagated += upd.propagated
                if upd.waiting_on != w.waiting_on:
                    dep_touched.add(o)
                cur[o] = self._commit(w, upd)
        except IllegalState:
            self.trace, self.prop_beyond_own = saved
            raise
        for txn, key, flags, until in releases or []:
            w = cur.get(order(txn))
            if w is None:
                ignored += 1
                continue
            upd = Update(w)
            if flags & 1:                                 # removeWaitingOnKeyAndMaybeExecute (:859-876)
                k = w.keys.index(int(key)) if int(key) in w.keys else -1
                if k >= 0 and upd.remove_waiting_on_key(k):
                    released += 1
                    key_touched.add(order(txn))
                else:
                    ignored += 1
            # the guarded updateExecuteAtLeast of CommandsForKey.java:1372-1381, 1476-1484
            if raw(until) != ZERO and awaits_only_deps(w.txn_id) and order(until) > order(upd.execute_at_least or ZERO):
                upd.update_execute_at_least(until)
            cur[order(txn)] = self._commit(w, upd)
        ready = [o for o in sorted(cur) if snap[o].is_waiting() and not cur[o].is_waiting()]
        for o in ready:
            d, k = o in dep_touched, o in key_touched
            self.ready_by["both" if d and k else "dep" if d else "key"] += 1
        n_changed = sum(bin(snap[o].waiting_on).count("1") - bin(cur[o].waiting_on).count("1") for o in cur)
        self.recs = cur
        index = {o: i for i, o in enumerate(sorted(cur))}
        self.stats = dict(notify_slots=slots, propagated=propagated, key_released=released, key_ignored=ignored, ready=len(ready))
        return dict(ready_rec=np.array([index[o] for o in ready], np.uint32), ready_txn=[cur[o].txn_id for o in ready],
                    ready_eal=[cur[o].execute_at_least or ZERO for o in ready], n_changed=n_changed)

    def erase(self, ids) -> int:
        n = 0
        for t in ids:
            n += self.recs.pop(order(t), None) is not None
        self.stats = dict(erased=n)
        return n

    def view(self) -> dict:
        """the columns of WaitingStore.view()"""
        ws = [self.recs[o] for o in sorted(self.recs)]
        col = lambda f, dt: np.array([f(w) for w in ws], dt)  # noqa: E731
        csum = lambda f: np.concatenate([[0], np.cumsum([f(w) for w in ws])]).astype(np.uint32)  # noqa: E731
        eal = [w.execute_at_least or ZERO for w in ws]
        deps = [t for w in ws for t in w.txn_ids]
        state, kw = [], []
        for w in ws:
            nd = len(w.txn_ids)
            for i in range(nd):
                state.append(WAITING if (w.waiting_on >> i) & 1 else
                             APPLIED_OR_INVALIDATED if w.applied is not None and (w.applied >> i) & 1 else NOT_WAITING)
            kw += [(w.waiting_on >> (nd + k)) & 1 for k in range(len(w.keys))]
        low = lambda w: w.waiting_on & ((1 << len(w.txn_ids)) - 1)  # noqa: E731
        return dict(
            msb=col(lambda w: w.txn_id[0], np.uint64), lsb=col(lambda w: w.txn_id[1], np.uint64), node=col(lambda w: w.txn_id[2], np.int32),
            xmsb=col(lambda w: w.execute_at[0], np.uint64), xlsb=col(lambda w: w.execute_at[1], np.uint64),
            xnode=col(lambda w: w.execute_at[2], np.int32),
            eal_msb=np.array([e[0] for e in eal], np.uint64), eal_lsb=np.array([e[1] for e in eal], np.uint64),
            eal_node=np.array([e[2] for e in eal], np.int32),
            flags=col(lambda w: (AWAITS_ONLY_DEPS if awaits_only_deps(w.txn_id) else 0) | (RANGE_DOMAIN if w.applied is not None else 0),
                      np.uint8),
            key_off=csum(lambda w: len(w.keys)), key=np.array([k for w in ws for k in w.keys], np.uint64),
            key_wait=np.array(kw, np.uint8), dep_off=csum(lambda w: len(w.txn_ids)),
            dmsb=np.array([t[0] for t in deps], np.uint64), dlsb=np.array([t[1] for t in deps], np.uint64),
            dnode=np.array([t[2] for t in deps], np.int32), dep_state=np.array(state, np.uint8),
            n_wait_dep=col(lambda w: bin(low(w)).count("1"), np.uint32),
            n_wait_key=col(lambda w: bin(w.waiting_on >> len(w.txn_ids)).count("1"), np.uint32),
            next_waiting_on=col(lambda w: w.next_waiting_on(), np.uint32))

    def bitsets(self) -> list:
        """per record the Java long[] words of (waitingOn, appliedOrInvalidated)"""
        def words(bits, n):
            out = [(bits >> (64 * i)) & ((1 << 64) - 1) for i in range((n + 63) // 64)]
            return [v - (1 << 64) if v >> 63 else v for v in out]
        return [(words(w.waiting_on, len(w.txn_ids) + len(w.keys)),
                 None if w.applied is None else words(w.applied, len(w.txn_ids)))
                for w in (self.recs[o] for o in sorted(self.recs))]


def rcmd_apply(rcmd: dict, upd: dict):
    """the (status, executeAt) a RangeCmdStore holds after upd (the last update of a TxnId wins; key-domain ids ignored)"""
    for i in range(len(upd["msb"])):
        t = (upd["msb"][i], upd["lsb"][i], upd["node"][i])
        if is_range_domain(t):
            rcmd[order(t)] = (int(upd["status"][i]), raw((upd["xmsb"][i], upd["xlsb"][i], upd["xnode"][i])))
    return rcmd
