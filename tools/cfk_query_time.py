"""Time acc_cfk_keydeps at the bench's steady-state shape: python tools/cfk_query_time.py [uniform|zipf] [batches] [top]

The shape of bench.py's cfk_steady_leg: a device store of the first 1M txns of workload.cfk_update_stream(1.5M txns x 8
keys over 1M keys, dist), then `batches` batches of 100K new txns (plus the final statuses that fall due), inputs resident
in HBM. Per batch, after acc_cfk_apply_deps, acc_cfk_keydeps runs on the batch's new txns (workload.preaccept_queries,
each with the executeAt the batch leaves it with, as ReplicaStore.preaccept_batch(scan="new") passes them). Pass 1 times
the call (wall clock, synchronised, the median of 3 calls per batch, one untimed call on the initial store first to
warm the buffers); pass 2 replays it
on a fresh store with every kernel timed (ACC_OPT_TIMING) for the breakdown. Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cassandra-accord_amd")]


def main(dist="uniform", n_batches=5, top_n=10, n_init=1_000_000, batch=100_000, local=0, reps=3):
    import torch
    from accord_amd import _lib as L
    from accord_amd import workload as W
    from accord_amd.deps import Context, _execute_at_after
    t0 = time.perf_counter()
    u = W.cfk_update_stream(n_init + batch * n_batches, 8, 1_000_000, dist=dist)
    cuts = W.cfk_stream_cuts(u, n_init, batch, n_batches)
    parts = [W.cfk_slice(u, 0, cuts[0])] + [W.cfk_slice(u, cuts[b], cuts[b + 1]) for b in range(n_batches)]
    qs = [W.preaccept_queries(p) for p in parts[1:]]
    xs = [_execute_at_after(p, q) for p, q in zip(parts[1:], qs)]
    t_gen = time.perf_counter() - t0
    dev = torch.device("cuda", local)
    keep = []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr()

    upds, queries = [], []
    for p in parts:
        P = {k: up(v) for k, v in p.items()}
        upds.append(L.CfkUpdates(L.ACC_MEM_DEVICE, len(p["msb"]), len(p["key"]), len(p["dmsb"]),
                                 L.TsCols(P["msb"], P["lsb"], P["node"]), L.TsCols(P["xmsb"], P["xlsb"], P["xnode"]),
                                 P["status"], P["flags"], P["key_off"], P["key"], P["dep_off"],
                                 L.TsCols(P["dmsb"], P["dlsb"], P["dnode"])))
    for q, (xm, xl, xn) in zip(qs, xs):
        queries.append(L.CfkQueries(len(q["msb"]), L.ACC_MEM_DEVICE, len(q["part_start"]),
                                    L.TsCols(up(q["msb"]), up(q["lsb"]), up(q["node"])), L.TsCols(up(xm), up(xl), up(xn)),
                                    up(q["part_off"].astype(np.uint32)), up(q["part_start"].astype(np.uint64))))
    torch.cuda.synchronize()

    def run(timing):
        rows, tm = [], {}
        with Context(local, timing=timing) as c:
            lib = c._lib
            h = C.c_void_p()
            c.check(lib.acc_cfk_create(c.handle, C.byref(h)))
            try:
                kv = L.KeydepsView()
                c.check(lib.acc_cfk_apply_deps(c.handle, h, C.byref(upds[0])))
                c.check(lib.acc_cfk_keydeps(c.handle, h, C.byref(queries[0]), C.byref(kv)))   # warm the query's buffers
                torch.cuda.synchronize()
                for ui, qi in zip(upds[1:], queries):
                    c.check(lib.acc_cfk_apply_deps(c.handle, h, C.byref(ui)))
                    torch.cuda.synchronize()
                    times = []
                    for _ in range(1 if timing else reps):   # the call reads the store only: repeats see one state
                        c.timing_reset()
                        t = time.perf_counter()
                        c.check(lib.acc_cfk_keydeps(c.handle, h, C.byref(qi), C.byref(kv)))
                        torch.cuda.synchronize()
                        times.append((time.perf_counter() - t) * 1e3)
                    ms = sorted(times)[len(times) // 2]
                    st = c.stats()
                    v = L.BatchIn()
                    c.check(lib.acc_cfk_view(c.handle, h, C.byref(v)))
                    rows.append(dict(query_ms=ms, store_txns=int(v.n_txn), store_pairs=int(v.n_pairs), queries=int(qi.n_query),
                                     pairs=st.get("cfq.pairs", 0), chunks=st.get("cfq.chunks", 0), hits=st.get("cfq.hits", 0),
                                     sorted_hits=st.get("cfq.sorted_hits", 0), deps=int(kv.total_deps)))
                    if timing:
                        for k, (x, n) in c.timing().items():
                            a = tm.setdefault(k, [0.0, 0])
                            a[0] += x
                            a[1] += n
            finally:
                lib.acc_cfk_destroy(h)
        return rows, tm

    rows, _ = run(False)
    _, tm = run(True)
    nb = len(rows)
    per = [round(r["query_ms"], 3) for r in rows]
    top = sorted(tm.items(), key=lambda kv: -kv[1][0])[:top_n]
    return {"workload": f"workload.cfk_update_stream({(n_init + batch * n_batches) // 1000}K txns x 8 {dist} keys over 1M keys): "
                        f"a {n_init // 1000}K-txn device store, then {n_batches} batches of {batch // 1000}K new txns; per "
                        "batch acc_cfk_apply_deps, then acc_cfk_keydeps of the new txns against the resident store (timed)",
            "query_ms_per_batch": round(sum(per) / nb, 3), "per_batch_query_ms": per,
            "max_over_min": round(max(per) / min(per), 3),
            "per_batch": [{k: v for k, v in r.items() if k != "query_ms"} for r in rows],
            "kernel_ms_per_batch": round(sum(x[0] for x in tm.values()) / nb, 3),
            "top_kernels_ms_per_batch": {k: round(x[0] / nb, 3) for k, x in top},
            "setup_gen_s": round(t_gen, 2)}


if __name__ == "__main__":
    dist = sys.argv[1] if len(sys.argv) > 1 else "uniform"
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    top = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    print(json.dumps({dist: main(dist, nb, top)}), flush=True)
