"""Time acc_waiting_register / acc_waiting_notify / acc_waiting_erase per call at a stated store size:
python tools/waiting_time.py [n_records] [deps_per_record] [batch] [reps]

The store: n_records (default 200,000) range-domain waiters over a pool of n_records range commands the range-command
store holds Stable at their TxnIds, each waiter with deps_per_record (default 16) deps drawn below its own TxnId and two
keys; every slot waits. Per repetition, host clocks around calls that end synchronised, inputs as host arrays:
  (a) acc_waiting_register of `batch` (default 20,000) further waiters of the same shape (the table merged and the index
      re-sorted: linear in the store);
  (b) acc_waiting_notify after `batch` pool commands became Applied, with those as `changed` and one release pair per
      key of `batch` records (work proportional to the slots of the changed deps: wt.notify_slots);
  (b2) the same call again, when nothing waits on the changed deps any more;
  (c) acc_waiting_erase of the `batch` records whose keys (b) released (they still wait on deps: a truncation).
One untimed repetition on a fresh store warms every buffer; the figures are medians over `reps` (default 3) more.
Prints one JSON line with the times and, per call, the wt.* stats it sets (last repetition); no time is asserted."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cassandra-accord_amd")]


NOTIFY = ("wt.notify_slots", "wt.propagated", "wt.ready", "wt.key_released", "wt.key_ignored", "wt.notify_us")
SETS = dict(register=("wt.register_evaluated", "wt.register_us"), notify=NOTIFY, notify_again=NOTIFY, erase=("wt.erased", "wt.erase_us"))


def median(x):
    return sorted(x)[len(x) // 2]


def ids(hlc, kind=0):
    n = len(hlc)
    return dict(msb=np.asarray(hlc, np.uint64), lsb=np.full(n, (kind << 1) | 1, np.uint64), node=np.ones(n, np.int32))


def waiters(rng, first, n, pool, nd):
    """n waiters with hlc first.. above the pool, nd sorted unique deps each, two keys"""
    w = ids(np.arange(first, first + n))
    w.update(xmsb=w["msb"], xlsb=w["lsb"], xnode=w["node"])
    # nd distinct pool entries out of a window of 4 nd at a random place: sorted unique per waiter
    off = np.sort(np.argsort(rng.random((n, 4 * nd)), axis=1)[:, :nd], axis=1)
    dep = pool[off + rng.integers(0, len(pool) - 4 * nd, size=(n, 1))].reshape(-1)
    d = ids(dep)
    key = np.sort(rng.integers(0, 1 << 20, size=(n, 2), dtype=np.uint64) * 2 + np.arange(2, dtype=np.uint64), axis=1).reshape(-1)
    w.update(key_off=np.arange(0, 2 * n + 1, 2, dtype=np.uint32), key=key, dep_off=np.arange(0, nd * n + 1, nd, dtype=np.uint32),
             dmsb=d["msb"], dlsb=d["lsb"], dnode=d["node"])
    return w


def rcmd_rows(hlc, status):
    u = ids(hlc)
    n = len(hlc)
    u.update(xmsb=u["msb"], xlsb=u["lsb"], xnode=u["node"], status=np.full(n, status, np.uint8), flags=np.zeros(n, np.uint8),
             rng_off=np.arange(n + 1, dtype=np.uint32), rng_start=np.asarray(hlc, np.uint64) * 2,
             rng_end=np.asarray(hlc, np.uint64) * 2 + 1)
    return u


def main(n_rec=200_000, nd=16, batch=20_000, reps=3):
    from accord_amd.deps import Context, RangeCmdStore, WaitingStore
    rng = np.random.default_rng(0xACC0)
    pool = np.arange(1000, 1000 + n_rec, dtype=np.uint64)
    base = waiters(rng, 10_000_000, n_rec, pool, nd)
    more = waiters(rng, 20_000_000, batch, pool, nd)
    applied = np.sort(rng.choice(pool, size=batch, replace=False))
    pick = np.sort(rng.choice(n_rec, size=batch, replace=False))
    rel = dict(msb=np.repeat(base["msb"][pick], 2), lsb=np.repeat(base["lsb"][pick], 2), node=np.repeat(base["node"][pick], 2),
               key=base["key"].reshape(-1, 2)[pick].reshape(-1), flags=np.ones(2 * batch, np.uint8),
               until_msb=np.zeros(2 * batch, np.uint64), until_lsb=np.zeros(2 * batch, np.uint64),
               until_node=np.zeros(2 * batch, np.int32))
    times = dict(register=[], notify=[], notify_again=[], erase=[])
    stats = {}
    with Context(0) as ctx:
        for rep in range(reps + 1):
            rc = RangeCmdStore(ctx)
            ws = WaitingStore(ctx, rc)
            rc.update(rcmd_rows(pool, 5))
            ws.register(base)

            def clock(name, fn):
                ctx.sync()
                t0 = time.perf_counter()
                out = fn()
                ctx.sync()
                if rep:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                st = ctx.stats()
                stats[name] = {k: st[k] for k in ("wt.records", "wt.slots") + SETS[name]}
                return out

            clock("register", lambda: ws.register(more))
            rc.update(rcmd_rows(applied, 8))
            clock("notify", lambda: ws.notify(ids(applied), rel))
            clock("notify_again", lambda: ws.notify(ids(applied), None))
            clock("erase", lambda: ws.erase({k: base[k][pick] for k in ("msb", "lsb", "node")}))
            ws.close()
            rc.close()
    print(json.dumps(dict(n_records=n_rec, deps_per_record=nd, batch=batch, reps=reps,
                          ms={k: round(median(v), 3) for k, v in times.items()}, stats=stats)))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:5]))
