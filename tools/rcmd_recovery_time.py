"""Time acc_rcmd_map_reduce_full against the whole-table route: python tools/rcmd_recovery_time.py [batches] [reps]

The store: the first 1M txns of workload.rangedeps_batch(config 4's width mix, p_range = 1, one range each) as range
commands with state drawn as tests/recovery_cases.range_recovery_case draws it: a uniform Status ordinal, executeAt bumped
past the TxnId for 45%, ERASED for 5%, HAS_DEPS for 70%, and 0..8 deps each (half of them near neighbours in TxnId order,
three in ten any stored txn, the rest TxnIds of a node no txn has; half keys, seven in ten of those inside the command's own
range, half ranges), applied by one acc_rcmd_update_cmds. Then `batches` batches of 50K further commands of that workload.
Per batch the update is timed once through acc_rcmd_update_cmds and, on a second store fed the same ranges, through
acc_rcmd_update: the difference is the cost of carrying the state. Then 2,000 of the batch's txns are recovered over their
own ranges at the four BeginRecovery parameter sets (L.RECOVERY_SCANS), inputs resident in HBM.

Timed in one process, the routes alternating, one untimed call each per batch and then `reps` (>= 5) timed ones, every
call followed by a device synchronise (wall clock, no kernel events recorded); a batch's figure is the sum of its four scans:
  resident   acc_rcmd_map_reduce_full
  snapshot   acc_map_reduce_full_ranges over acc_rcmd_view + acc_rcmd_state_view, every column in HBM (ACC_MEM_DEVICE)
The copied-out results of both are decoded (range ids to (start, end), table indices to TxnIds) and must be equal per batch
and set. One more call of each route per batch with kernel events on gives the per-kernel split. Prints one JSON line."""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cassandra-accord_amd")]

FOREIGN_NODE = 30_000
IDENT = np.uint64(0xFFFFFFFFFFFF001E)


def draw_state(rb, rng):
    """state columns for every row of rb (hlc = row + 1, rows in TxnId order), vectorised"""
    from accord_amd import _lib as L
    from accord_amd import workload as W
    n = rb.n_txn
    i = np.arange(n, dtype=np.int64)
    tm, tl, tn = rb.keys.txn_msb, rb.keys.txn_lsb, rb.keys.txn_node
    status = rng.integers(0, 11, size=n).astype(np.uint8)
    bump = rng.random(n) < 0.45
    bm, bl, bn = W.encode_ts(np.ones(n), i + 1 + rng.integers(1, 40, size=n), np.zeros(n), 1 + rng.integers(0, 4, size=n))
    flags = (np.where(rng.random(n) < 0.05, L.ACC_RCMD_ERASED, 0) | np.where(rng.random(n) < 0.7, L.ACC_RCMD_HAS_DEPS, 0)).astype(np.uint8)
    cnt = rng.integers(0, 9, size=n)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    own = np.repeat(i, cnt)
    m = len(own)
    u = rng.random(m)
    tgt = np.where(u < 0.5, np.clip(own + rng.integers(-5, 25, size=m), 0, n - 1), rng.integers(0, n, size=m))
    foreign = u >= 0.8
    dm, dl = tm[tgt], tl[tgt]
    dn = np.where(foreign, FOREIGN_NODE, tn[tgt]).astype(np.int32)
    is_key = rng.random(m) < 0.5
    s0, e0 = rb.rng_start[own].astype(np.int64), rb.rng_end[own].astype(np.int64)
    inside = s0 + (rng.random(m) * (e0 - s0 + 1)).astype(np.int64)
    anywhere = rng.integers(0, 1 << 32, size=m)
    ds = np.where(is_key & (rng.random(m) < 0.7), inside, anywhere)
    de = np.where(is_key, 0, ds + rng.integers(1, 1 << 16, size=m))
    order = np.lexsort((dn, dl & IDENT, dm, own))                # per command by Timestamp.compareTo
    return dict(status=status, flags=flags, xm=np.where(bump, bm, tm).astype(np.uint64), xl=np.where(bump, bl, tl).astype(np.uint64),
                xn=np.where(bump, bn, tn).astype(np.int32), dep_off=off, dm=dm[order].astype(np.uint64), dl=dl[order].astype(np.uint64),
                dn=dn[order], ds=ds[order].astype(np.uint64), de=de[order].astype(np.uint64), dk=is_key[order].astype(np.uint8))


def decoded_digest(r, tm, tl, tn):
    """a RangeDeps result with range ids decoded to (start, end) and table indices to TxnIds"""
    hs = hashlib.blake2b(digest_size=8)
    for a in (r.arena_off, r.rd_off, r.u_off, r.arena, r.rng_start[r.range_id], r.rng_end[r.range_id], tm[r.dep_txn], tl[r.dep_txn],
              tn[r.dep_txn]):
        hs.update(np.ascontiguousarray(a).tobytes())
    return hs.hexdigest()


def main(n_batches=5, reps=5, n_init=1_000_000, batch=50_000, n_query=2_000, local=0):
    import torch
    from accord_amd import _lib as L
    from accord_amd import workload as W
    from accord_amd.deps import Context, device_array
    t0 = time.perf_counter()
    rb = W.rangedeps_batch(n_init + batch * n_batches, W.CONFIG_SEEDS["4"], p_range=1.0, status_model="preaccepted")
    assert rb.is_range().all() and rb.n_ranges == rb.n_txn
    tm, tl, tn = rb.keys.txn_msb, rb.keys.txn_lsb, rb.keys.txn_node
    rng = np.random.default_rng(0x5EED)
    st = draw_state(rb, rng)
    cuts = [0, n_init] + [n_init + batch * (b + 1) for b in range(n_batches)]
    dev = torch.device("cuda", local)
    keep = []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr()

    upds, plains, queries = [], [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        n = b - a
        d0, d1 = int(st["dep_off"][a]), int(st["dep_off"][b])
        ids = L.TsCols(up(tm[a:b]), up(tl[a:b]), up(tn[a:b]))
        cols = (up(np.arange(n + 1, dtype=np.uint32)), up(rb.rng_start[a:b]), up(rb.rng_end[a:b]))
        upds.append(L.RcmdCmdUpdates(n, L.ACC_MEM_DEVICE, n, ids, up(st["flags"][a:b]), *cols,
                                     L.TsCols(up(st["xm"][a:b]), up(st["xl"][a:b]), up(st["xn"][a:b])), up(st["status"][a:b]), d1 - d0,
                                     up((st["dep_off"][a:b + 1] - d0).astype(np.uint32)),
                                     L.TsCols(up(st["dm"][d0:d1]), up(st["dl"][d0:d1]), up(st["dn"][d0:d1])), up(st["ds"][d0:d1]),
                                     up(st["de"][d0:d1]), up(st["dk"][d0:d1])))
        plains.append(L.RcmdUpdates(n, L.ACC_MEM_DEVICE, n, ids, up(st["flags"][a:b] & np.uint8(L.ACC_RCMD_ERASED)), *cols))
        if a == 0:
            continue
        pick = a + np.sort(rng.choice(n, size=n_query, replace=False))
        q = dict(ids=L.TsCols(up(tm[pick]), up(tl[pick]), up(tn[pick])), zeros=up(np.zeros(n_query + 1, np.uint32)),
                 off=up(np.arange(n_query + 1, dtype=np.uint32)), rs=up(rb.rng_start[pick]), re=up(rb.rng_end[pick]),
                 isr=up(np.ones(n_query, np.uint8)), none=up(np.zeros(1, np.uint64)))
        queries.append(q)
    t_gen = time.perf_counter() - t0
    torch.cuda.synchronize()
    variants = ("resident", "snapshot")
    scans = list(L.RECOVERY_SCANS.items())
    ei = int(rb.end_inclusive)
    rows = []
    with Context(local, timing=True) as c:
        lib = c._lib
        h, hp = C.c_void_p(), C.c_void_p()
        c.check(lib.acc_rcmd_create(c.handle, ei, C.byref(h)))
        c.check(lib.acc_rcmd_create(c.handle, ei, C.byref(hp)))
        c.timing_filter(["-"])                                   # no launch carries this tag: nothing records events
        try:
            def timed(f):
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                return (time.perf_counter() - t) * 1e3

            def update(b):
                return (timed(lambda: c.check(lib.acc_rcmd_update_cmds(c.handle, h, C.byref(upds[b])))),
                        timed(lambda: c.check(lib.acc_rcmd_update(c.handle, hp, C.byref(plains[b])))))

            init_ms = update(0)
            view = L.RangedepsView()
            for b, q in enumerate(queries):
                upd_ms = update(b + 1)
                ust = c.stats()
                tv, sv = L.RcmdTable(), L.RcmdState()
                c.check(lib.acc_rcmd_view(c.handle, h, C.byref(tv)))
                c.check(lib.acc_rcmd_state_view(c.handle, h, C.byref(sv)))
                n = int(tv.n_cmd)
                assert n == cuts[b + 2] and int(sv.n_cmd) == n
                table = L.RangeCmdsIn(n, L.ACC_MEM_DEVICE, ei, tv.txn_id, sv.execute_at, sv.status, sv.flags, tv.rng_off, tv.rng_start,
                                      tv.rng_end, sv.dep_off, sv.dep_txn, sv.dep_start, sv.dep_end, sv.dep_is_key)
                g = lambda ptr, cnt, dt: device_array(c, ptr, cnt, dt)  # noqa: E731
                ids = (g(tv.txn_id.msb, n, np.uint64), g(tv.txn_id.lsb, n, np.uint64), g(tv.txn_id.node, n, np.int32))

                def scan(k, params):
                    sa, td, ts, after = params
                    fl = L.ACC_FULL_EXECUTES_AFTER if after else 0
                    if k == "resident":
                        ri = L.CfkRecoveryIn(n_query, L.ACC_MEM_DEVICE, 0, n_query, q["ids"], q["zeros"], q["none"], q["off"], q["rs"],
                                             q["re"], ei, sa, td, ts, fl, -1)
                        c.check(lib.acc_rcmd_map_reduce_full(c.handle, h, C.byref(ri), C.byref(view)))
                    else:
                        ri = L.RecoveryRangesIn(n_query, L.ACC_MEM_DEVICE, q["ids"], q["isr"], q["off"], q["rs"], q["re"], sa, td, ts, fl, -1)
                        c.check(lib.acc_map_reduce_full_ranges(c.handle, C.byref(table), C.byref(ri), C.byref(view)))

                times = {k: [] for k in variants}
                per_set = {k: {name: [] for name, _ in scans} for k in variants}
                hashes, found, rst = {}, {}, {}
                for rep in range(reps + 1):                      # round 0 warms both routes' buffers, untimed, and compares
                    for k in variants:
                        total = 0.0
                        for name, params in scans:
                            ms = timed(lambda: scan(k, params))
                            total += ms
                            if rep:
                                per_set[k][name].append(ms)
                                continue
                            r = c.copy_out_range(view)
                            hashes[k, name] = decoded_digest(r, *ids)
                            found[name] = int((np.diff(r.u_off.astype(np.int64)) > 0).sum())
                            if k == "resident":
                                rst[name] = {s: v for s, v in c.stats().items() if s.startswith("rcr.")}
                        if rep:
                            times[k].append(total)
                for name, _ in scans:
                    assert hashes["resident", name] == hashes["snapshot", name], f"batch {b}, {name}: the results differ"
                # where the time goes: one more call of each route with kernel events on
                split = {}
                for k in variants:
                    c.timing_filter(None)
                    c.timing_reset()
                    for name, params in scans:
                        scan(k, params)
                    torch.cuda.synchronize()
                    split[k] = {name: round(ms, 3) for name, (ms, _) in sorted(c.timing().items(), key=lambda kv: -kv[1][0])[:8]}
                    c.timing_filter(["-"])
                med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
                rows.append(dict(store_cmds=n, store_deps=int(sv.n_deps), queries=n_query, queries_with_rows=found,
                                 n_query_x_n_cmd=n_query * n, rcr=rst, hashes={name: hashes["resident", name] for name, _ in scans},
                                 update_cmds_ms=round(upd_ms[0], 3), update_plain_ms=round(upd_ms[1], 3),
                                 inserted=ust.get("rcmd.inserted", 0),
                                 ms={k: [round(x, 3) for x in sorted(v)] for k, v in times.items()},
                                 median_ms_per_set={k: {name: round(med(v), 3) for name, v in per_set[k].items()} for k in variants},
                                 kernel_ms_top8=split))
        finally:
            lib.acc_rcmd_destroy(h)
            lib.acc_rcmd_destroy(hp)
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    summary = {k: round(sum(med(r["ms"][k]) for r in rows) / len(rows), 3) for k in variants}
    claim = [med(r["ms"]["resident"]) < med(r["ms"]["snapshot"]) - (max(r["ms"]["snapshot"]) - min(r["ms"]["snapshot"])) for r in rows]
    return {"workload": f"workload.rangedeps_batch({(n_init + batch * n_batches) // 1000}K range txns x 1 range, config 4's widths) with "
                        f"drawn state: a {n_init // 1000}K-command device store, then {n_batches} batches of {batch // 1000}K commands; "
                        f"per batch {n_query} of its txns recovered over their own ranges at the four BeginRecovery sets (ms = their "
                        f"sum, median of {reps} per batch, mean over the batches)",
            "median_ms": summary, "results_equal": True,
            "resident_below_snapshot_by_more_than_its_spread": claim,
            "update_cmds_ms_median": round(med([r["update_cmds_ms"] for r in rows]), 3),
            "update_plain_ms_median": round(med([r["update_plain_ms"] for r in rows]), 3),
            "initial_update_ms": {"cmds": round(init_ms[0], 3), "plain": round(init_ms[1], 3)}, "per_batch": rows,
            "setup_gen_s": round(t_gen, 2)}


if __name__ == "__main__":
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    print(json.dumps(main(nb, max(reps, 5))), flush=True)
