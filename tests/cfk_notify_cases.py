"""Seeded CommandsForKey update streams with an execution frontier, for acc_cfk_notify — TEST INFRASTRUCTURE.

cfk_cases.cfk_case leaves most txns COMMITTED forever, which blocks every STABLE entry behind them: a literal notify
releases next to nothing on it. frontier_case instead applies txns roughly in executeAt order a short lag behind their
commit, so each key holds a long APPLIED prefix and a short live window of STABLE, COMMITTED and uncommitted entries;
deps witness most lower txns of a key and leave some out on purpose (a committing txn may leave out every txn that is
still uncommitted: those go to its missing[], and it is released past them); a few txns stay uncommitted for long and
null `next` behind them; about half of the executeAts are bumped, some past higher TxnIds, some onto one another.

conditions() states, on the host model alone, what every seed a GPU test uses must give; segments_case builds stores of
given segment lengths and bumped counts for the tier edges. All streams are in the CFK_UPD layout of oracle.py.
"""
from __future__ import annotations

import numpy as np

import cfk_notify_model as NM
from accord_amd import workload as W

TK, HIST, PRE, ACC, COMMITTED, STABLE, APPLIED, INVALID = range(8)
KINDS = np.array([0, 1, 3, 4])   # Read, Write, SyncPoint, ExclusiveSyncPoint
UPD_COLS = (("msb", np.uint64), ("lsb", np.uint64), ("node", np.int32), ("xmsb", np.uint64), ("xlsb", np.uint64),
            ("xnode", np.int32), ("status", np.uint8), ("flags", np.uint8))

# csrc/cfknotify.hip
NT_LANE_MAX = 16          # bumped entries of a key the lane tier ranks by default
NT_LANE_FORCE_MAX = 64    # ... when the lane tier is forced
NT_WAVE_MAX = 1024        # bumped entries of a key the wave tier holds in LDS
SCAN_TILE = 8192          # csrc/prims.hpp: u32 elements one block of the scan takes (a block chunk of the entry space)

SEEDS = (12, 17, 24)      # frontier_case seeds that meet conditions() after every batch (test_cfk_notify_model.py)
N_BATCHES = 5


def _ts(hlc, flags, node):
    return tuple(int(x) for x in W.encode_ts(1, hlc, flags, node))


def _order(t):
    return (t[0], t[1] & NM.IDENT, t[2])


class _Stream:
    def __init__(self):
        self.cols = {k: [] for k, _ in UPD_COLS}
        self.key_off, self.keys, self.dep_off, self.deps = [0], [], [0], []

    def add(self, tid, ex, status, per_key):
        """per_key: [(key code, [raw dep TxnIds, sorted])]"""
        for (k, _), v in zip(UPD_COLS, (tid[0], tid[1], tid[2], ex[0], ex[1], ex[2], status, 0)):
            self.cols[k].append(v)
        for code, deps in per_key:
            self.keys.append(code)
            self.deps.extend(deps)
            self.dep_off.append(len(self.deps))
        self.key_off.append(len(self.keys))

    def done(self):
        upd = {k: np.array(self.cols[k], dt) for k, dt in UPD_COLS}
        upd.update(key_off=np.array(self.key_off, np.uint32), key=np.array(self.keys, np.uint64),
                   dep_off=np.array(self.dep_off, np.uint32), dmsb=np.array([d[0] for d in self.deps], np.uint64),
                   dlsb=np.array([d[1] for d in self.deps], np.uint64), dnode=np.array([d[2] for d in self.deps], np.int32))
        return upd


def frontier_case(seed, n_txn=300, n_keys=12, keys_per=2, lag=12.0, p_bump=0.5, p_slow=0.1, p_invalid=0.03, p_omit=0.08,
                  p_omit_uncommitted=0.7, window=60):
    """One stream of updates, events in time order. Txn i (TxnId hlc 4 i + 4) is first seen at time i, commits a few
    txns later (a slow one: some 40 later), turns STABLE soon after and is APPLIED `lag` after the time its executeAt
    stands for, so the frontier moves in executeAt order."""
    rng = np.random.default_rng(seed)
    kind = rng.choice(KINDS, size=n_txn, p=[0.35, 0.45, 0.1, 0.1])
    tid = [_ts(4 * i + 4, int(kind[i]) << 1, 1 + int(rng.integers(0, 4))) for i in range(n_txn)]
    keys = [sorted(int(k) * 10 + 100 for k in rng.choice(n_keys, size=min(keys_per, n_keys), replace=False)) for _ in range(n_txn)]
    on_key = {}
    for i in range(n_txn):
        for k in keys[i]:
            on_key.setdefault(k, []).append(i)
    ex, t_commit, events = [], [], []
    for i in range(n_txn):
        x = tid[i]
        if rng.random() < p_bump:   # between two TxnIds, up to eight txns on; two bumps may meet on one executeAt
            x = _ts(4 * i + 4 + 2 + 4 * int(rng.integers(0, 8)), 0, 1 + int(rng.integers(0, 2)))
        ex.append(x)
        slow = rng.random() < p_slow
        tc = i + (rng.uniform(30, 50) if slow else rng.uniform(1, 5))
        t_commit.append(tc)
        events.append((float(i), i, PRE))
        if rng.random() < 0.5:
            events.append((i + rng.uniform(0.2, 0.9), i, ACC))
        if rng.random() < p_invalid:
            events.append((tc, i, INVALID))
            t_commit[-1] = float("inf")
            continue
        ts_ = tc + rng.uniform(0.1, 4)
        r = rng.random()
        if r < 0.15:
            events.append((tc, i, COMMITTED))                  # stays COMMITTED until it is applied
        else:
            if r < 0.6:
                events.append((tc, i, COMMITTED))
            events.append((ts_ if r < 0.6 else tc, i, STABLE))
        x_time = ((x[1] >> 16) - 4) / 4.0
        events.append((max(ts_, x_time + lag) + rng.uniform(0, 2), i, APPLIED))
    events.sort(key=lambda e: (e[0], e[1], e[2]))
    s = _Stream()
    for t, i, st in events:
        per_key = []
        dkb = _order(tid[i]) if st in (PRE, ACC) or ex[i] == tid[i] else _order(ex[i])
        omit_unc = rng.random() < p_omit_uncommitted
        for k in keys[i]:
            deps = []
            if st in (ACC, COMMITTED, STABLE, APPLIED):
                for j in on_key[k]:
                    if j == i or j < i - window or _order(tid[j]) >= dkb:
                        continue
                    uncommitted = t_commit[j] > t
                    if (omit_unc and uncommitted) or rng.random() < p_omit:
                        continue
                    deps.append(tid[j])
            per_key.append((k, deps))
        s.add(tid[i], tid[i] if st in (PRE, ACC, INVALID) else ex[i], st, per_key)
    return s.done()


def batches(upd, n=N_BATCHES):
    """the stream cut into n batches; the last cut leaves the final tenth of the events out, so every state a test sees
    has a live window"""
    import cfk_cases as CC
    total = len(upd["msb"]) * 9 // 10
    out, rest, done = [], upd, 0
    for i in range(n):
        cut = total * (i + 1) // n
        part, rest = CC.split_updates(rest, cut - done)
        done = cut
        out.append(part)
    return out


def conditions(state, m=None):
    """what a state a GPU test uses must show on the host model alone; returns the figures"""
    m = NM.model(state, with_view=False) if m is None else m
    st = state["status"]
    eo = state["ent_off"].astype(np.int64)
    n_rel = int((m["ev_kind"] == NM.RELEASE).sum())
    n_wait = int((m["ev_kind"] == NM.WAITING_TO_EXECUTE).sum())
    n_held = len(m["held"])
    stable = int((st == STABLE).sum())
    assert stable == n_rel + n_held
    ids = [NM.order(a, b, c) for a, b, c in zip(state["emsb"], state["elsb"], state["enode"])]
    xs = [NM.order(a, b, c) for a, b, c in zip(state["xmsb"], state["xlsb"], state["xnode"])]
    nulled = no_unc = past = 0
    for k in range(len(state["key"])):
        seg = range(int(eo[k]), int(eo[k + 1]))
        live = [e for e in seg if st[e] in (COMMITTED, STABLE)]
        unc = [e for e in seg if st[e] < COMMITTED]
        no_unc += not unc
        nulled += bool(live) and m["next"][k] == NM.NONE
        past += sum(any(ids[o] > ids[e] and xs[e] > ids[o] for o in seg) for e in live)
    rel = m["ev_kind"] == NM.RELEASE
    fig = dict(releases=n_rel, held=n_held, waiting=n_wait, events=n_rel + n_wait, stable=stable, keys_next_nulled=int(nulled),
               keys_no_uncommitted=int(no_unc), releases_past_missing=int((rel & (m["ev_missing"] > 0)).sum()),
               candidates_bumped_past=int(past))
    assert 4 * n_rel >= stable and 4 * n_held >= stable, fig
    assert 10 * n_wait >= n_rel + n_wait, fig
    assert nulled >= 1 and no_unc >= 1 and fig["releases_past_missing"] >= 1 and past >= 1, fig
    return fig


def segments_case(seed, shapes, p_stable=0.7):
    """One batch of updates that leaves key 100 + 10 j with shapes[j] = (entries, bumped, live) entries: the last `live`
    committed-class entries COMMITTED or STABLE and the rest APPLIED, `bumped` of the committed-class entries with an
    executeAt off their TxnId (up to eight TxnIds on, so runs cross and tie), and, where entries allow, three
    uncommitted entries among the live ones. Each live entry's deps hold most of the 12 ids below it."""
    rng = np.random.default_rng(seed)
    s = _Stream()
    base = 0     # every key has TxnIds of its own: a store holds one executeAt and status per TxnId
    for j, (n, nb, live) in enumerate(shapes):
        code = 100 + 10 * j
        kind = rng.choice(KINDS, size=n, p=[0.35, 0.45, 0.1, 0.1])
        tid = [_ts(4 * (base + i) + 4, int(kind[i]) << 1, 1 + int(rng.integers(0, 4))) for i in range(n)]
        n_unc = 3 if n >= live + 8 and live >= 4 else 0
        unc = set(int(x) for x in rng.choice(np.arange(n - live - n_unc, n), size=n_unc, replace=False)) if n_unc else set()
        com = [i for i in range(n) if i not in unc]
        assert nb <= len(com) and live <= len(com)
        bumped = set(int(x) for x in rng.choice(com, size=nb, replace=False))
        live_set = set(com[len(com) - live:])
        for i in range(n):
            if i in unc:
                s.add(tid[i], tid[i], PRE, [(code, [])])
                continue
            x = _ts(4 * (base + i) + 4 + 2 + 4 * int(rng.integers(0, 8)), 0, 1 + int(rng.integers(0, 2))) if i in bumped else tid[i]
            st = APPLIED if i not in live_set else (STABLE if rng.random() < p_stable else COMMITTED)
            deps = [tid[d] for d in range(max(0, i - 12), i) if rng.random() < (0.4 if d in unc else 0.9)] if i in live_set else []
            s.add(tid[i], x, st, [(code, deps)])
        base += n
    return s.done()


# ---------------------------------------------------------------- hand-written states and streams

def state_of(keys):
    """{key code: [(hlc, kind, status, executeAt hlc or None for the TxnId, [missing hlcs])]} (node 1, entries in hlc
    order) -> the key-major state layout; a missing hlc names the entry of that hlc on the same key"""
    cols = {k: [] for k in ("emsb", "elsb", "enode", "xmsb", "xlsb", "xnode", "status", "mmsb", "mlsb", "mnode")}
    key, ent_off, miss_off = [], [0], [0]
    for code in sorted(keys):
        rows = keys[code]
        ids = {h: _ts(h, kind << 1, 1) for h, kind, _, _, _ in rows}
        for h, kind, st, xh, miss in rows:
            t = ids[h]
            x = t if xh is None else _ts(xh, 0, 1)
            for k, v in zip(("emsb", "elsb", "enode", "xmsb", "xlsb", "xnode", "status"), t + x + (st,)):
                cols[k].append(v)
            for mh in miss:
                for k, v in zip(("mmsb", "mlsb", "mnode"), ids[mh]):
                    cols[k].append(v)
            miss_off.append(len(cols["mmsb"]))
        key.append(code)
        ent_off.append(len(cols["emsb"]))
    dt = dict(emsb=np.uint64, elsb=np.uint64, enode=np.int32, xmsb=np.uint64, xlsb=np.uint64, xnode=np.int32, status=np.uint8,
              mmsb=np.uint64, mlsb=np.uint64, mnode=np.int32)
    out = {k: np.array(v, dt[k]) for k, v in cols.items()}
    out.update(key=np.array(key, np.uint64), ent_off=np.array(ent_off, np.uint32), miss_off=np.array(miss_off, np.uint32))
    return out


def stream_of(steps):
    """[(hlc, kind, status, executeAt hlc or None, key code, [dep (hlc, kind)])] -> one batch of updates (node 1)"""
    s = _Stream()
    for h, kind, st, xh, code, deps in steps:
        t = _ts(h, kind << 1, 1)
        s.add(t, t if xh is None else _ts(xh, 0, 1), st, [(code, [_ts(dh, dk << 1, 1) for dh, dk in deps])])
    return s.done()


W_, R_, S_ = 1, 0, 3   # Kind ordinals: Write, Read, SyncPoint
A, B, C, D = 4, 8, 12, 16


def literal_abcd():
    """Writes A < B < C < D on key 500: A APPLIED, B STABLE at B missing [], C PREACCEPTED, D STABLE at D missing [C]
    (D's deps [A, B] leave C out). Worked from CommandsForKey.java:422-470, 1512-1635:
      committed[] = [A, B, D], minUncommitted = C, next = nextWrite = B (C > B's executeAt).
      B: uncommittedIndex = 2 (C); executeAt B inserts at 2, nothing backfilled; expect 0 == missing 0 -> RELEASE.
      D: executeAt D is txns[3], C is backfilled: writes = B + C = 2; missing [C], none below C: 1 -> held.
    Then B APPLIED: D: expect 1 (C) == missing 1 -> RELEASE; next = nextWrite = D, nulled since C < D's executeAt.
    Returns [(updates, the state after them, the expected rows)], rows = (min_uncommitted, next, next_write,
    [(entry, kind, pos)]) with entries as hlcs."""
    one = stream_of([(A, W_, APPLIED, None, 500, []), (B, W_, STABLE, None, 500, [(A, W_)]), (C, W_, PRE, None, 500, []),
                     (D, W_, STABLE, None, 500, [(A, W_), (B, W_)])])
    s1 = state_of({500: [(A, W_, APPLIED, None, []), (B, W_, STABLE, None, []), (C, W_, PRE, None, []), (D, W_, STABLE, None, [C])]})
    two = stream_of([(B, W_, APPLIED, None, 500, [(A, W_)])])
    s2 = state_of({500: [(A, W_, APPLIED, None, []), (B, W_, APPLIED, None, []), (C, W_, PRE, None, []), (D, W_, STABLE, None, [C])]})
    return [(one, s1, (C, B, B, [(B, NM.RELEASE, 1)])), (two, s2, (C, None, None, [(D, NM.RELEASE, 2)]))]


def literal_kinds():
    """Write W (hlc 4) COMMITTED, Read R (8) STABLE, SyncPoint S (12) STABLE on key 500, no missing, nothing
    uncommitted. Worked from :1512-1635:
      W at its TxnId: committed[] = [W, R, S]. W -> WAITING_TO_EXECUTE, writes 1; R expects writes = 1 != 0: held,
        reads 1; S expects syncs 0 + reads 1 + writes 1 = 2: held. next = nextWrite = W.
      W bumped to hlc 14 (past S): committed[] = [R, S, W]. R expects 0 -> RELEASE at 0; S expects reads 1: held;
        W -> WAITING_TO_EXECUTE at 2. next = R, nextWrite = W. Events in TxnId order: W, R.
    Returns [(updates from an empty store, the state after them, the expected rows)] as literal_abcd."""
    deps = [(8, R_, STABLE, None, 500, [(4, W_)]), (12, S_, STABLE, None, 500, [(4, W_), (8, R_)])]
    at = state_of({500: [(4, W_, COMMITTED, None, []), (8, R_, STABLE, None, []), (12, S_, STABLE, None, [])]})
    past = state_of({500: [(4, W_, COMMITTED, 14, []), (8, R_, STABLE, None, []), (12, S_, STABLE, None, [])]})
    return [(stream_of([(4, W_, COMMITTED, None, 500, [])] + deps), at, (None, 4, 4, [(4, NM.WAITING_TO_EXECUTE, 0)])),
            (stream_of([(4, W_, COMMITTED, 14, 500, [])] + deps), past,
             (None, 8, 4, [(4, NM.WAITING_TO_EXECUTE, 2), (8, NM.RELEASE, 0)]))]


def rows_as_hlc(state, m):
    """a one-key model / store result as literal_*'s rows"""
    h = lambda e: None if e == NM.NONE else int(state["elsb"][e]) >> 16  # noqa: E731
    return (h(m["min_uncommitted"][0]), h(m["next"][0]), h(m["next_write"][0]),
            [(h(e), int(k), int(p)) for e, k, p in zip(m["ev_entry"], m["ev_kind"], m["ev_pos"])])
