"""Time acc_rcmd_partial_rangedeps beside acc_rcmd_rangedeps: python tools/rcmd_partial_time.py [batches] [reps]

The store and the queries are tools/rcmd_query_time.py's: the first 1M txns of workload.rangedeps_batch(config 4's width
mix, p_range = 1, one range each) as range commands, applied by one acc_rcmd_update; then `batches` batches of 100K new
txns, half range txns x 1 range, half key txns x 4 keys, the batch's range commands applied first (acc_rcmd_update, timed
once), then its 100K queries answered, inputs resident in HBM, executeAt = TxnId.
Before the first batch one acc_rcmd_redundant_before prunes the store: 40 ranges, each 1/80 of the key space with as much
between two of them, bounds alternating between the TxnIds a tenth and a twentieth into the initial store. The map
holds 40 intervals from then on; the commands below the bounds lose what the ranges cover.

Timed in one process after a warm-up round, the variants alternating, the median of `reps` (>= 5) calls per batch each,
every call followed by a device synchronise (wall clock, no kernel events recorded):
  plain    acc_rcmd_rangedeps
  warm     acc_rcmd_partial_rangedeps on an unchanged store: the union index is reused
  cold     acc_rcmd_partial_rangedeps as the first call after the map was touched: the same 40 ranges are given again
           before each call (untimed; every bound is absorbed and nothing is rewritten, but the index is rebuilt)
The share of the warm call spent collecting (pu_tinfo, pu_count, pu_collect, pu_records and the copy of the raw pairs is
not a kernel) comes from the ACC_OPT_TIMING events of one more warm call per batch. Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cassandra-accord_amd")]

FOREIGN_NODE = 30_000
KEYS_PER_TXN = 4
N_MARKS = 40
COLLECT = ("pu_tinfo", "pu_count", "pu_collect", "pu_records")


def main(n_batches=5, reps=5, n_init=1_000_000, batch=100_000, local=0):
    import torch
    from accord_amd import _lib as L
    from accord_amd import workload as W
    from accord_amd.deps import Context
    t0 = time.perf_counter()
    half = batch // 2
    rb = W.rangedeps_batch(n_init + half * n_batches, W.CONFIG_SEEDS["4"], p_range=1.0, status_model="preaccepted")
    assert rb.is_range().all() and rb.n_ranges == rb.n_txn
    tm, tl, tn = rb.keys.txn_msb, rb.keys.txn_lsb, rb.keys.txn_node
    rng = np.random.default_rng(0x5EED)
    cuts = [0, n_init] + [n_init + half * (b + 1) for b in range(n_batches)]
    dev = torch.device("cuda", local)
    keep = []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr()

    upds, queries = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        n = b - a
        upds.append(L.RcmdUpdates(n, L.ACC_MEM_DEVICE, n, L.TsCols(up(tm[a:b]), up(tl[a:b]), up(tn[a:b])), up(np.zeros(n, np.uint8)),
                                  up(np.arange(n + 1, dtype=np.uint32)), up(rb.rng_start[a:b]), up(rb.rng_end[a:b])))
        if a == 0:
            continue
        keys = np.sort(rng.integers(0, 1 << 32, size=(n, KEYS_PER_TXN), dtype=np.int64), axis=1)
        for j in range(1, KEYS_PER_TXN):
            keys[:, j] = np.maximum(keys[:, j], keys[:, j - 1] + 1)
        klsb = (tl[a:b] & np.uint64(0xFFFFFFFFFFFF0000)) | np.uint64(W.WRITE << 1)
        cat = lambda x, y, dt: np.concatenate([np.asarray(x, dt), np.asarray(y, dt)])  # noqa: E731
        queries.append(L.CfkMixedQueries(2 * n, L.ACC_MEM_DEVICE, n * KEYS_PER_TXN, n,
                                         L.TsCols(up(cat(tm[a:b], tm[a:b], np.uint64)), up(cat(tl[a:b], klsb, np.uint64)),
                                                  up(cat(tn[a:b], np.full(n, FOREIGN_NODE), np.int32))),
                                         L.TsCols(None, None, None), up(cat(np.zeros(n + 1), KEYS_PER_TXN * np.arange(1, n + 1), np.uint32)),
                                         up(keys.reshape(-1).astype(np.uint64)), up(cat(np.arange(n + 1), np.full(n, n), np.uint32)),
                                         up(rb.rng_start[a:b]), up(rb.rng_end[a:b]), int(rb.end_inclusive), 0))
    # the prune: 40 ranges over 1/80 of the key space each
    step = (1 << 32) // (2 * N_MARKS)
    ms_ = np.arange(N_MARKS, dtype=np.uint64) * np.uint64(2 * step) + np.uint64(1)
    me_ = ms_ + np.uint64(step)
    brow = np.where(np.arange(N_MARKS) % 2 == 0, n_init // 10, n_init // 20)
    marks = L.CfkRedundantIn(L.ACC_MEM_DEVICE, N_MARKS, int(rb.end_inclusive), up(ms_), up(me_),
                             L.TsCols(up(tm[brow]), up(tl[brow]), up(tn[brow])))
    t_gen = time.perf_counter() - t0
    torch.cuda.synchronize()
    variants = ("plain", "warm", "cold")
    rows = []
    with Context(local, timing=True) as c:
        lib = c._lib
        h = C.c_void_p()
        c.check(lib.acc_rcmd_create(c.handle, int(rb.end_inclusive), C.byref(h)))
        try:
            def timed(fn):
                t = time.perf_counter()
                c.check(fn())
                torch.cuda.synchronize()
                return (time.perf_counter() - t) * 1e3

            c.timing_filter(["-"])     # no launch carries this tag: no events but where asked for below
            init_ms = timed(lambda: lib.acc_rcmd_update(c.handle, h, C.byref(upds[0])))
            prune_ms = timed(lambda: lib.acc_rcmd_redundant_before(c.handle, h, C.byref(marks)))
            prune_st = c.stats()
            rv, pv = L.RangedepsView(), L.RcmdPartialView()
            for b, (ui, qi) in enumerate(zip(upds[1:], queries)):
                upd_ms = timed(lambda: lib.acc_rcmd_update(c.handle, h, C.byref(ui)))
                times = {k: [] for k in variants}
                call = dict(plain=lambda: lib.acc_rcmd_rangedeps(c.handle, h, C.byref(qi), C.byref(rv)),
                            warm=lambda: lib.acc_rcmd_partial_rangedeps(c.handle, h, C.byref(qi), C.byref(pv)))
                call["cold"] = call["warm"]
                for rep in range(reps + 1):                      # round 0 warms every variant's buffers, untimed
                    for k in variants:
                        if k == "cold":
                            c.check(lib.acc_rcmd_redundant_before(c.handle, h, C.byref(marks)))
                            torch.cuda.synchronize()
                        ms = timed(call[k])
                        if rep:
                            times[k].append(ms)
                st = c.stats()
                plain_deps, deps = int(rv.total_deps), int(pv.rd.total_deps)
                assert st["rcmd.partial_intervals"] > 0 and deps >= plain_deps
                # one warm call with kernel events: where its time goes
                c.timing_filter(None)
                c.timing_reset()
                c.check(call["warm"]())
                torch.cuda.synchronize()
                ev = c.timing()
                c.timing_filter(["-"])
                kms = sum(v for v, _ in ev.values())
                rows.append(dict(store_cmds=int(pv.n_cmd), union_ids=int(pv.n_ids), union_ranges=int(pv.rd.n_ranges),
                                 queries=int(qi.n_query), deps=deps, plain_deps=plain_deps,
                                 partial_intervals=st["rcmd.partial_intervals"], pairs_shared=st["rcmd.partial_pairs_shared"],
                                 raw_entries=st.get("rangedeps.raw_entries", 0), update_ms=round(upd_ms, 3),
                                 collect_kernel_ms=round(sum(ev.get(k, (0.0, 0))[0] for k in COLLECT), 3), kernel_ms=round(kms, 3),
                                 top_kernels_ms={k: round(v[0], 3) for k, v in sorted(ev.items(), key=lambda kv: -kv[1][0])[:8]},
                                 ms={k: [round(x, 3) for x in sorted(v)] for k, v in times.items()}))
        finally:
            lib.acc_rcmd_destroy(h)
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    mean = lambda xs: sum(xs) / len(xs)  # noqa: E731
    summary = {k: round(mean([med(r["ms"][k]) for r in rows]), 3) for k in variants}
    spread = {k: round(max(max(r["ms"][k]) / min(r["ms"][k]) for r in rows), 3) for k in variants}
    upd = med([r["update_ms"] for r in rows])
    build = summary["cold"] - summary["warm"]
    return {"workload": f"tools/rcmd_query_time.py's store ({n_init // 1000}K range commands) and queries ({n_batches} batches of "
                        f"{batch // 1000}K), after one acc_rcmd_redundant_before of {N_MARKS} ranges; median of {reps} per batch, mean "
                        f"over the batches",
            "median_ms": summary, "max_over_min_of_repeats": spread,
            "warm_over_plain": round(summary["warm"] / summary["plain"], 3),
            "cold_build_ms": round(build, 3), "update_ms_median": round(upd, 3), "cold_build_over_update": round(build / upd, 3),
            "collect_share_of_warm_kernel_time": round(mean([r["collect_kernel_ms"] / r["kernel_ms"] for r in rows]), 4),
            "initial_update_ms": round(init_ms, 3), "prune_ms": round(prune_ms, 3),
            "prune_cmds_cut": prune_st.get("rcmd.redundant_cmds_cut", 0), "prune_cmds_dropped": prune_st.get("rcmd.redundant_cmds_dropped", 0),
            "per_batch": rows, "setup_gen_s": round(t_gen, 2)}


if __name__ == "__main__":
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    print(json.dumps(main(nb, max(reps, 5))), flush=True)
