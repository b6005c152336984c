"""Seeded step sequences for the resident WaitingOn store — TEST INFRASTRUCTURE.

A chain is a list of steps over one RangeCmdStore and one WaitingStore:
  ("rcmd", upd)                         RangeCmdStore.update with status / executeAt columns
  ("register", waiters)                 WaitingStore.register
  ("notify", changed | None, releases)  WaitingStore.notify (changed: dict(msb, lsb, node); releases: dict of columns)
  ("erase", ids)                        WaitingStore.erase
Every sequence is legal for the library: waiters are unknown to the range-command store, and only records that have
stopped waiting become Applied there. A range-command update may move a command's status backwards: that is how a record
comes to remember a dep as applied (state 2) that a later waiter's own evaluation would leave waiting, the case
setAppliedAndPropagate exists for.

run_model(steps) replays a chain on waiting_model.Store and returns, per step, what the device must show after it.
"""
from __future__ import annotations

import functools

import numpy as np

import waiting_model as WM

SEEDS = (11, 12, 13)
READ, WRITE, EPHEMERAL_READ, SYNC_POINT, EXCLUSIVE_SYNC_POINT = 0, 1, 2, 3, 4
LATE = 50_000          # added to a TxnId's hlc for an executeAt after every waiter's
EDGE_DEPS = (0, 1, 15, 16, 17, 63, 64, 65, 128, 129)   # around WT_LANE_MAX = 16 and the 64-bit word


def tid(hlc, kind, range_domain, node=1):
    return (int(hlc), (int(kind) << 1) | int(bool(range_domain)), int(node))


def ts_cols(ids, names=("msb", "lsb", "node")):
    return {names[0]: np.array([t[0] for t in ids], np.uint64), names[1]: np.array([t[1] for t in ids], np.uint64),
            names[2]: np.array([t[2] for t in ids], np.int32)}


def rcmd_upd(rows):
    """rows: (TxnId, status, executeAt); one unit range per update"""
    ids = [r[0] for r in rows]
    n = len(rows)
    out = ts_cols(ids)
    out.update(ts_cols([r[2] for r in rows], ("xmsb", "xlsb", "xnode")))
    out.update(status=np.array([r[1] for r in rows], np.uint8), flags=np.zeros(n, np.uint8),
               rng_off=np.arange(n + 1, dtype=np.uint32), rng_start=np.array([2 * t[0] for t in ids], np.uint64),
               rng_end=np.array([2 * t[0] + 1 for t in ids], np.uint64))
    return out


def waiters_of(ws, with_wait=True):
    """ws: dicts(txn, x, keys, key_wait, deps, dep_wait); keys and deps are sorted here, their wait bytes with them"""
    out = ts_cols([w["txn"] for w in ws])
    out.update(ts_cols([w["x"] for w in ws], ("xmsb", "xlsb", "xnode")))
    key, kw, dep, dw, ko, do = [], [], [], [], [0], [0]
    for w in ws:
        ks = sorted(zip(w["keys"], w.get("key_wait") or [1] * len(w["keys"])))
        ds = sorted(zip([WM.order(d) for d in w["deps"]], w["deps"], w.get("dep_wait") or [1] * len(w["deps"])))
        key += [k for k, _ in ks]; kw += [b for _, b in ks]
        dep += [d for _, d, _ in ds]; dw += [b for _, _, b in ds]
        ko.append(len(key)); do.append(len(dep))
    out.update(key_off=np.array(ko, np.uint32), key=np.array(key, np.uint64), dep_off=np.array(do, np.uint32))
    out.update(ts_cols(dep, ("dmsb", "dlsb", "dnode")))
    if with_wait:
        out.update(key_wait=np.array(kw, np.uint8), dep_wait=np.array(dw, np.uint8))
    return out


def releases_of(pairs):
    """pairs: (txn, key, flags, until)"""
    out = ts_cols([p[0] for p in pairs])
    out.update(ts_cols([p[3] for p in pairs], ("until_msb", "until_lsb", "until_node")))
    out.update(key=np.array([p[1] for p in pairs], np.uint64), flags=np.array([p[2] for p in pairs], np.uint8))
    return out


def release_list(rel):
    if rel is None:
        return []
    return [((rel["msb"][i], rel["lsb"][i], rel["node"][i]), int(rel["key"][i]), int(rel["flags"][i]),
             (rel["until_msb"][i], rel["until_lsb"][i], rel["until_node"][i])) for i in range(len(rel["msb"]))]


def id_list(c):
    return None if c is None else [(c["msb"][i], c["lsb"][i], c["node"][i]) for i in range(len(c["msb"]))]


def late(t):
    return (t[0] + LATE, t[1], t[2])


def _waiter(rng, hlc, pool, n_dep, n_key=None):
    kind, dom = [(WRITE, 0), (READ, 1), (SYNC_POINT, 1), (EXCLUSIVE_SYNC_POINT, 1), (EPHEMERAL_READ, 0)][int(rng.integers(5))]
    t = tid(hlc, kind, dom, 1 + int(rng.integers(3)))
    x = t if rng.random() < 0.5 else (t[0] + int(rng.integers(1, 3000)), t[1], t[2])
    nk = int(rng.integers(0, 5)) if n_key is None else n_key
    keys = sorted(int(k) for k in rng.choice(64, size=nk, replace=False))
    deps = [pool[i] for i in rng.choice(len(pool), size=min(n_dep, len(pool)), replace=False)]
    return dict(txn=t, x=x, keys=keys, key_wait=[int(rng.random() < 0.9) for _ in keys], deps=deps,
                dep_wait=[int(rng.random() < 0.9) for _ in deps])


@functools.lru_cache(maxsize=None)
def chain(seed, scale=1.0):
    """rcmd, register (the records that finish at once among them), rcmd, register, notify, rcmd, notify(None), erase,
    rcmd, notify: about 300 records with 0 to about 130 deps"""
    rng = np.random.default_rng(seed)
    ne, nr, n1, n2 = int(170 * scale), int(40 * scale), int(110 * scale), int(150 * scale)
    E = [tid(1000 + 3 * i, [READ, SYNC_POINT, EXCLUSIVE_SYNC_POINT][i % 3], 1, 1 + i % 2) for i in range(ne)]
    R = [tid(3000 + 2 * i, READ, 1) for i in range(nr)]
    steps = []
    # -- the deps' first states: a sixth unknown, the rest spread over the status ordinals, some executing late
    st0 = {}
    for e in E:
        s = int(rng.choice([-1, 2, 4, 5, 6, 7, 8, 9, 9, 10, 10]))
        x = late(e) if rng.random() < 0.35 else e
        if s == 9 and rng.random() < 0.3:
            x = WM.ZERO          # Erased: executeAt unknown
        if s >= 0:
            st0[e] = (s, x)
    steps.append(("rcmd", rcmd_upd([(e, s, x) for e, (s, x) in st0.items()] + [(r, 5, r) for r in R])))
    done = [e for e, (s, x) in st0.items() if s >= 9 or (s >= 4 and x != WM.ZERO and x[0] > LATE)]
    hlc = iter(range(5000, 100_000, 7))
    # -- records that are finished as they register (Read, range domain: every dep truncated, invalidated or late)
    ws = [dict(txn=r, x=r, keys=[], deps=[done[i] for i in rng.choice(len(done), size=int(rng.integers(3, 40)), replace=False)])
          for r in R]
    ws += [_waiter(rng, next(hlc), E, int(rng.integers(0, 40))) for _ in range(n1)]
    ws.append(_waiter(rng, next(hlc), E, 0, n_key=2))          # ready through its keys alone, later
    ws[-1]["key_wait"] = [1, 1]
    order_ = rng.permutation(len(ws))
    steps.append(("register", waiters_of([ws[i] for i in order_])))
    first = list(ws)
    # -- the finished records become Applied; some deps move back below PreCommitted or to a late Stable, others advance
    rows = [(r, 8, r) for r in R]
    for e in E:
        p = rng.random()
        if p < 0.15:
            rows.append((e, 2, e))
        elif p < 0.25:
            rows.append((e, 5, late(e)))
        elif p < 0.35:
            rows.append((e, int(rng.choice([8, 9, 10])), e))
    steps.append(("rcmd", rcmd_upd(rows)))
    pool = E + R
    sizes = list(EDGE_DEPS) + [int(rng.integers(0, 131)) for _ in range(n2 - len(EDGE_DEPS))]
    ws2 = [_waiter(rng, next(hlc), pool, nd) for nd in sizes]
    for w in ws2[:len(EDGE_DEPS)]:                             # the edge sizes wait on everything, some on their Rs
        w["dep_wait"] = [1] * len(w["deps"])
    steps.append(("register", waiters_of([ws2[i] for i in rng.permutation(len(ws2))])))
    allw = first + ws2
    # -- a notify of some changed deps with release pairs: present, absent, duplicated, keys not held, untils
    def some_releases(frac):
        pairs = []
        for w in allw:
            for k in w["keys"]:
                if rng.random() < frac:
                    until = late(E[int(rng.integers(ne))]) if rng.random() < 0.3 else WM.ZERO
                    pairs.append((w["txn"], k, 1, until))
        pairs += pairs[:5]                                      # duplicates
        pairs += [(tid(999_000 + i, READ, 1), 3, 1, WM.ZERO) for i in range(3)]           # no record
        pairs += [(w["txn"], 1000 + i, 1, WM.ZERO) for i, w in enumerate(allw[:4])]       # a key the record lacks
        pairs += [(w["txn"], 0, 0, late(E[i])) for i, w in enumerate(allw[:40:4])]        # until alone
        return releases_of([pairs[i] for i in rng.permutation(len(pairs))])
    rows = [(e, int(rng.choice([5, 8, 9, 10])), e if rng.random() < 0.7 else late(e)) for e in E if rng.random() < 0.4]
    steps.append(("rcmd", rcmd_upd(rows)))
    chg = sorted({r[0] for r in rows[::2]} | set(R[::3]), key=WM.order)
    steps.append(("notify", ts_cols(chg), some_releases(0.3)))
    steps.append(("notify", None, some_releases(0.3)))
    # -- erase: some of everything, and ids the store does not hold
    gone = sorted([w["txn"] for w in allw if rng.random() < 0.25] + [tid(998_000 + i, READ, 1) for i in range(4)], key=WM.order)
    steps.append(("erase", ts_cols(gone)))
    # -- everything left is invalidated and released: every record stops waiting
    steps.append(("rcmd", rcmd_upd([(e, 10, e) for e in E])))
    every = [(w["txn"], k, 1, WM.ZERO) for w in allw for k in w["keys"]]
    steps.append(("notify", ts_cols(sorted(pool, key=WM.order)), releases_of(every)))
    return tuple(steps)


def run_model(steps, store=None, rcmd=None):
    """per step: dict(name, out, stats, view, error); the model store and rcmd dict are left after the last step"""
    store = WM.Store() if store is None else store
    rcmd = {} if rcmd is None else rcmd
    res = []
    for st in steps:
        out, err = None, None
        try:
            if st[0] == "rcmd":
                WM.rcmd_apply(rcmd, st[1])
                store.stats = {}
            elif st[0] == "register":
                out = store.register(st[1], rcmd)
            elif st[0] == "notify":
                out = store.notify(id_list(st[1]), release_list(st[2]), rcmd)
            else:
                store.erase(id_list(st[1]))
        except WM.IllegalState:
            err = "state"
        except WM.IllegalArgument:
            err = "arg"
        res.append(dict(name=st[0], out=out, stats=dict(store.stats), view=store.view(), error=err))
    return res, store, rcmd


@functools.lru_cache(maxsize=None)
def chain_model(seed):
    return run_model(chain(seed))


def literal_steps(range_waiter: bool):
    """hand-worked: one waiter W (hlc 500, executeAt hlc 600) over seven deps, one per step of evaluate(), and a record R
    (D4's) that remembers E as applied. test_waiting_model states the expected bytes."""
    E = tid(100, READ, 1)        # in R.dep at state 2; below PreCommitted for W: only the propagation clears it
    D0 = tid(110, READ, 1)       # absent from rcmd: step 0
    D0b = tid(120, READ, 1)      # status 3: step 0
    D2 = tid(130, READ, 1)       # Invalidated: step 2
    D3 = tid(140, READ, 1)       # Stable, executes late: step 3
    D4 = tid(150, READ, 1)       # Applied, with a record: step 4
    D5 = tid(160, READ, 1)       # Stable, executes before W: step 5
    W = tid(500, READ if range_waiter else WRITE, 1 if range_waiter else 0)
    steps = [("rcmd", rcmd_upd([(E, 10, E), (D4, 5, D4)])),
             ("register", waiters_of([dict(txn=D4, x=D4, keys=[], deps=[E])])),
             ("rcmd", rcmd_upd([(E, 2, E), (D0b, 3, D0b), (D2, 10, D2), (D3, 5, late(D3)), (D4, 8, D4), (D5, 5, D5)])),
             ("register", waiters_of([dict(txn=W, x=(600, W[1], W[2]), keys=[7, 9], deps=[E, D0, D0b, D2, D3, D4, D5])]))]
    return steps, dict(E=E, D0=D0, D0b=D0b, D2=D2, D3=D3, D4=D4, D5=D5, W=W)


def edge_case(n_deps, total_slots=None):
    """records of the given dep counts over one pool of Stable deps (every slot waits), padded by further records to
    total_slots dep slots; then the whole pool is invalidated"""
    pool = [tid(1000 + i, READ, 1) for i in range(max(max(n_deps, default=0), 130))]
    ws = [dict(txn=tid(5000 + i, READ if i % 2 else WRITE, i % 2), x=tid(5000 + i, READ, 1), keys=[i % 5], deps=pool[:n])
          for i, n in enumerate(n_deps)]
    if total_slots is not None:
        left, i = total_slots - sum(n_deps), len(ws)
        while left > 0:
            n = min(left, 130)
            ws.append(dict(txn=tid(5000 + i, READ, 1), x=tid(5000 + i, READ, 1), keys=[], deps=pool[:n]))
            left -= n
            i += 1
    return (("rcmd", rcmd_upd([(p, 5, p) for p in pool])), ("register", waiters_of(ws, with_wait=False)),
            ("rcmd", rcmd_upd([(p, 10, p) for p in pool]))), pool, ws
