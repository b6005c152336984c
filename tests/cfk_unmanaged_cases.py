"""Seeded cases for acc_cfk_register_unmanaged / acc_cfk_notify_unmanaged — TEST INFRASTRUCTURE.

family(seed) builds, over a handful of keys with TxnIds of their own (a store holds one status per TxnId):
  base      one batch of updates: per key an APPLIED prefix, a COMMITTED / STABLE middle (some executeAts bumped), an
            uncommitted tail;
  waiters   commands CommandsForKey does not manage (range-domain Read / SyncPoint / ExclusiveSyncPoint, key-domain
            EphemeralRead), each over some keys with deps = the key's entries below it (a few left out) plus unknown
            TxnIds no key holds (shared between waiters of a key), and over keys the store lacks;
  later     two more batches: the uncommitted entries and some of the unknown TxnIds commit, then everything applies;
  ranges    a RedundantBefore step for the end of the chain.
TxnId hlcs: entries 0 mod 4, bumped executeAts 2 mod 4, unknown ids 1 mod 4, waiters 3 mod 4.
run_model(case) walks the chain on the host model alone and asserts what every family must show; the GPU tests compare
the device against the same walk.
"""
from __future__ import annotations

import numpy as np

import cfk_cases as CC
import cfk_notify_cases as NC
import cfk_redundant_model as M
import cfk_unmanaged_model as UM

TK, HIST, PRE, ACC, COMMITTED, STABLE, APPLIED, INVALID = range(8)
READ, WRITE, EPHEMERAL_READ, SYNC_POINT, EXCLUSIVE_SYNC_POINT, LOCAL_ONLY = range(6)
UM_LANE_MAX = 16           # csrc/cfkunmanaged.hip: trimmed deps of a pair the lane tier walks by default
SEEDS = (3, 5, 8)          # family seeds (their conditions are asserted in test_cfk_unmanaged_model.py)
NEW_KEYS = (50, 105, 999)  # below, between and above the store's keys 100, 110, ...


def ts(hlc, kind=WRITE, node=1, domain=0):
    return NC._ts(hlc, (kind << 1) | domain, node)


class Waiters:
    """the CfkStore.register_unmanaged dict, waiter by waiter"""

    def __init__(self):
        self.s = NC._Stream()

    def add(self, tid, ex, per_key):
        """per_key: [(key code, [raw deps, sorted])], key codes ascending"""
        self.s.add(tid, ex, 0, sorted(per_key))

    def done(self):
        w = self.s.done()
        del w["status"], w["flags"]
        return w


def waiters_of(items):
    w = Waiters()
    for tid, ex, per_key in items:
        w.add(tid, tid if ex is None else ex, per_key)
    return w.done()


def family(seed, n_keys=8):
    rng = np.random.default_rng(seed)
    base, commit, apply_ = NC._Stream(), NC._Stream(), NC._Stream()
    ent, unknown = {}, {}      # key -> [(tid, executeAt, st0, st1)], key -> [unknown tid]
    hlc = 0
    for j in range(n_keys):
        code = 100 + 10 * j
        n = int(rng.integers(8, 16))
        rows, taken = [], set()
        for i in range(n):
            kind = int(rng.choice(NC.KINDS, p=[0.35, 0.45, 0.1, 0.1]))
            tid = ts(hlc + 4 * i + 4, kind, 1 + int(rng.integers(0, 3)))
            x = tid
            if rng.random() < 0.3:     # bumped past up to three higher TxnIds; no two entries of a key share an executeAt
                xh = hlc + 4 * i + 6 + 4 * int(rng.integers(0, 4))
                while xh in taken:
                    xh += 4
                taken.add(xh)
                x = ts(xh, 0, 1)
            p = i / n
            tail = p >= 0.85 and j % 3 == 0        # stays uncommitted through the commit batch
            st0 = APPLIED if p < 0.4 else (STABLE if rng.random() < 0.6 else COMMITTED) if p < 0.6 else PRE
            st1 = st0 if st0 != PRE or tail else (STABLE if rng.random() < 0.5 else COMMITTED)
            rows.append((tid, x, st0, st1))
        ent[code] = rows
        unknown[code] = [ts(hlc + 4 * (n // 2) + 1), ts(hlc + 4 * (n - 1) + 1)]
        hlc += 4 * n + 40
    top = hlc
    for code, rows in ent.items():
        for i, (tid, x, st0, st1) in enumerate(rows):
            deps = [r[0] for r in rows[:i]]
            base.add(tid, tid if st0 == PRE else x, st0, [(code, deps if st0 != PRE else [])])
            if st1 != st0:
                commit.add(tid, x, st1, [(code, deps)])
            apply_.add(tid, x, APPLIED, [(code, deps)])
        u = unknown[code][0]                        # the lower unknown id turns out to be a Write that commits, then applies
        below = [r[0] for r in rows if M.order(r[0]) < M.order(u)]
        commit.add(u, u, COMMITTED, [(code, below)])
        apply_.add(u, u, APPLIED, [(code, below)])
    w = Waiters()
    codes = sorted(ent)

    def deps_on(code, tid, p_drop, unk):
        d = [r[0] for r in ent[code] if M.order(r[0]) < M.order(tid) and rng.random() >= p_drop]
        d += [u for u in unk if M.order(u) < M.order(tid)]
        return sorted(d, key=M.order)

    # an ExclusiveSyncPoint above everything over every key and the keys the store lacks
    esp = ts(top + 3, EXCLUSIVE_SYNC_POINT, 1, 1)
    w.add(esp, esp, [(c, deps_on(c, esp, 0.0, unknown[c] if c % 20 == 0 else [])) for c in codes] +
          [(c, [ts(1, WRITE, 2), ts(5, WRITE, 2)]) for c in NEW_KEYS])
    # a SyncPoint that shares the unknown ids with it, and one new key
    sp = ts(top + 7, SYNC_POINT, 2, 1)
    w.add(sp, sp, [(c, deps_on(c, sp, 0.2, unknown[c])) for c in codes[::2]] + [(NEW_KEYS[1], [ts(5, WRITE, 2)])])
    # range reads and ephemeral reads inside the keys' id ranges: the executeAt filter matters, prefixes may be all applied
    for j, code in enumerate(codes):
        rows = ent[code]
        for frac, kind, dom in ((0.35, READ, 1), (0.55, EPHEMERAL_READ, 0), (0.75, READ, 1), (1.0, EPHEMERAL_READ, 0)):
            i = min(len(rows) - 1, int(frac * len(rows)))
            h = (rows[i][0][1] >> 16) + 3
            tid = ts(h, kind, 3, dom)
            x = tid if rng.random() < 0.7 else ts(h + 8, kind, 3, dom)
            w.add(tid, x, [(code, deps_on(code, tid, 0.1, unknown[code] if rng.random() < 0.3 else []))])
    # a waiter without deps, and one without keys
    w.add(ts(top + 11, READ, 1, 1), ts(top + 11, READ, 1, 1), [(codes[0], [])])
    w.add(ts(top + 15, SYNC_POINT, 1, 1), ts(top + 15, SYNC_POINT, 1, 1), [])
    # the RedundantBefore step: the first key past all its entries (it leaves the state, its records stay), the rest of
    # the lower half of the keys up to two thirds of their entries (an entry equal to the bound stays)
    half = codes[1:len(codes) // 2]
    ranges = M.ranges_of([(codes[0] - 1, codes[0], ts(top + 1))] + [(c - 1, c, ent[c][2 * len(ent[c]) // 3][0]) for c in half])
    return dict(seed=seed, base=base.done(), waiters=w.done(), later=[commit.done(), apply_.done()], ranges=ranges)


def run_model(case, oracle_apply):
    """The chain on the host model: register, the commit batch, notify, the apply batch, notify, RedundantBefore,
    notify. Returns the steps [(name, payload, state after, records after, events or register result)] and asserts the
    family's conditions. oracle_apply: oracle.cfk_apply."""
    state = oracle_apply(CC.empty_snapshot(), case["base"])
    st = UM.Store(state)
    steps = []
    reg = st.register(case["waiters"])
    state = st.state()
    steps.append(("register", case["waiters"], state, UM.comparable(st.records()), reg))
    events = []
    for upd in case["later"]:
        state = oracle_apply(state, upd)
        st.load(state)
        steps.append(("apply_deps", upd, state, UM.comparable(st.records()), None))
        ev = sorted(st.notify())
        events += ev
        steps.append(("notify", None, state, UM.comparable(st.records()), ev))
        again = st.notify()
        assert again == [], "a second notify with nothing changed emits no event"
    bm = M.BoundMap(1).add(case["ranges"])
    state = M.with_redundant_before(state, lambda k: M.NONE, bm.get)
    st.load(state)
    st.set_bounds(bm)
    steps.append(("redundant_before", case["ranges"], state, UM.comparable(st.records()), None))
    ev = sorted(st.notify())
    events += ev
    steps.append(("notify", None, state, UM.comparable(st.records()), ev))
    # what every family must show
    oc = reg["outcome"]
    assert all((oc == o).any() for o in (UM.READY, UM.PENDING_COMMIT, UM.PENDING_APPLY)), np.bincount(oc, minlength=3)
    kinds = {(k, f) for k, f, _, _, _ in events}
    assert {(UM.EV_TO_APPLY, 1), (UM.EV_RELEASE, 1), (UM.EV_RELEASE, 0)} <= kinds, kinds
    assert (UM.EV_TO_APPLY, 0) not in kinds       # a record only moves to APPLY by being re-evaluated
    before = set(int(c) for c in oracle_apply(CC.empty_snapshot(), case["base"])["key"])
    assert set(int(c) for c in steps[0][2]["key"]) - before, "at least one key is created"
    wt = case["waiters"]
    per = {}
    for i in range(len(wt["msb"])):
        for j in range(int(wt["key_off"][i]), int(wt["key_off"][i + 1])):
            if oc[j] == UM.READY:
                continue
            for d in range(int(wt["dep_off"][j]), int(wt["dep_off"][j + 1])):
                per.setdefault((int(wt["key"][j]), M.order((wt["dmsb"][d], wt["dlsb"][d], wt["dnode"][d]))), set()).add(i)
    held = {(int(steps[0][2]["key"][k]), M.order((steps[0][2]["emsb"][e], steps[0][2]["elsb"][e], steps[0][2]["enode"][e])))
            for k in range(len(steps[0][2]["key"])) for e in range(int(steps[0][2]["ent_off"][k]), int(steps[0][2]["ent_off"][k + 1]))
            if steps[0][2]["status"][e] == TK}
    assert any(len(ws) >= 2 for kt, ws in per.items() if kt in held), "a missing dep shared by two waiters"
    assert reg["n_inserted"] == len(steps[0][2]["status"]) - len(oracle_apply(CC.empty_snapshot(), case["base"])["status"])
    return steps


# ---------------------------------------------------------------- shapes for the tier and tile edges

def wide_case(dep_counts, n_entries=1100, absent_every=7):
    """One key (500) of n_entries APPLIED / COMMITTED / PREACCEPTED Writes, and one ExclusiveSyncPoint waiter per dep
    count on it: its deps are the first `count` of the ids 4, 6, 8, ... of which every hlc 0 mod 4 is an entry and every
    `absent_every`-th other one is absent (hlc 2 mod 4)."""
    s = NC._Stream()
    for i in range(n_entries):
        st = APPLIED if i % 3 == 0 else COMMITTED if i % 3 == 1 else PRE
        t = ts(4 * i + 4)
        s.add(t, t, st, [(500, [])])
    w = Waiters()
    for q, n in enumerate(dep_counts):
        pool = []
        i = 0
        while len(pool) < n:
            pool.append(ts(4 * i + 4))
            if i % absent_every == q % absent_every and len(pool) < n:
                pool.append(ts(4 * i + 6))
            i += 1
        tid = ts(4 * (n_entries + q) + 7, EXCLUSIVE_SYNC_POINT, 1, 1)
        w.add(tid, tid, [(500, pool)])
    return s.done(), w.done()
