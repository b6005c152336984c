"""Time acc_cfk_map_reduce_full at the bench's steady-state shape: python tools/cfk_recovery_time.py [uniform|zipf] [batches] [queries]

The store of tools/cfk_query_time.py: the first 1M txns of workload.cfk_update_stream(1.5M txns x 8 keys over 1M keys,
dist), then `batches` batches of 100K new txns, every input resident in HBM. After each acc_cfk_apply_deps one batch of
recovery queries runs: `queries` of the batch's new txns (evenly strided), each recovered on its own keys, at the four
BeginRecovery parameter sets (messages/BeginRecovery.java:334, 348, 365, 378), through two routes on the same store:

  resident  acc_cfk_map_reduce_full: the store's key-major segments and missing[] lists read in place
  snapshot  acc_map_reduce_full over acc_cfk_missing: the txn-major copy, re-ranked, re-sorted and re-segmented per call

The two alternate in one process (resident, snapshot, resident, ..), 5 timed calls each per batch and parameter set
after one untimed call each; reported per route: the median of 5, summed over the four sets, per batch. Their copied-out
results are compared once per batch and set and must be equal. A second pass on a fresh store replays the batches with
every kernel timed (ACC_OPT_TIMING) for the per-route breakdown, and times the first set once more with ANY_DEPS in
place of WITHOUT (the same window, kinds and statuses, no missing[] probe): cr_count + cr_emit of the two differ by what
the probes cost. Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cassandra-accord_amd")]

FIELDS = ("arena_off", "arena", "kd_off", "key_idx", "u_off", "dep_txn")


def main(dist="uniform", n_batches=5, n_rec=2000, n_init=1_000_000, batch=100_000, local=0, reps=5, top_n=8):
    import torch
    from accord_amd import _lib as L
    from accord_amd import workload as W
    from accord_amd.deps import Context
    t0 = time.perf_counter()
    u = W.cfk_update_stream(n_init + batch * n_batches, 8, 1_000_000, dist=dist)
    cuts = W.cfk_stream_cuts(u, n_init, batch, n_batches)
    parts = [W.cfk_slice(u, 0, cuts[0])] + [W.cfk_slice(u, cuts[b], cuts[b + 1]) for b in range(n_batches)]
    qs = []
    for p in parts[1:]:
        q = W.preaccept_queries(p)
        nq = len(q["msb"])
        pick = np.unique(np.linspace(0, nq - 1, min(n_rec, nq)).astype(np.int64))
        off = q["part_off"].astype(np.int64)
        per = off[pick + 1] - off[pick]
        idx = np.repeat(off[pick], per) + (np.arange(int(per.sum())) - np.repeat(np.cumsum(per) - per, per))
        qs.append(dict(msb=q["msb"][pick], lsb=q["lsb"][pick], node=q["node"][pick],
                       key_off=np.concatenate([[0], np.cumsum(per)]).astype(np.uint32),
                       key_code=q["part_start"][idx].astype(np.uint64)))
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
    for q in qs:
        nq = len(q["msb"])
        queries.append(dict(n=nq, pairs=len(q["key_code"]), ids=L.TsCols(up(q["msb"]), up(q["lsb"]), up(q["node"])),
                            key_off=up(q["key_off"]), key_code=up(q["key_code"]), rng_off=up(np.zeros(nq + 1, np.uint32))))
    torch.cuda.synchronize()
    scans = [(name,) + L.RECOVERY_SCANS[name] for name in L.RECOVERY_SCANS]
    probe_free = ("startedBeforeAnyDeps", L.ACC_STARTED_BEFORE, L.ACC_DEP_ANY, L.ACC_STATUS_IS_PROPOSED, True)

    def run(timing):
        rows, tm = [], {"resident": {}, "snapshot": {}, "resident_no_probe": {}}
        with Context(local, timing=timing) as c:
            lib = c._lib
            h = C.c_void_p()
            c.check(lib.acc_cfk_create(c.handle, C.byref(h)))
            kv = L.KeydepsView()

            def resident(q, sa, td, ts, after):
                ri = L.CfkRecoveryIn(q["n"], L.ACC_MEM_DEVICE, q["pairs"], 0, q["ids"], q["key_off"], q["key_code"], q["rng_off"],
                                     None, None, 1, sa, td, ts, L.ACC_FULL_EXECUTES_AFTER if after else 0, -1)
                c.check(lib.acc_cfk_map_reduce_full(c.handle, h, C.byref(ri), C.byref(kv)))

            def snapshot(q, sa, td, ts, after):
                bv = L.CfkBatchView()
                c.check(lib.acc_cfk_missing(c.handle, h, C.byref(bv)))
                ri = L.RecoveryIn(q["n"], L.ACC_MEM_DEVICE, q["ids"], q["key_off"], q["key_code"], bv.missing_off, bv.missing_txn,
                                  int(bv.n_missing), sa, td, ts, L.ACC_FULL_EXECUTES_AFTER if after else 0, -1)
                c.check(lib.acc_map_reduce_full(c.handle, C.byref(bv.batch), C.byref(ri), C.byref(kv)))

            routes = (("resident", resident), ("snapshot", snapshot))

            def timed(fn, q, scan, into=None):
                c.timing_reset()
                t = time.perf_counter()
                fn(q, *scan[1:])
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t) * 1e3
                if into is not None:
                    for k, (x, n) in c.timing().items():
                        a = into.setdefault(k, [0.0, 0])
                        a[0] += x
                        a[1] += n
                return ms

            try:
                c.check(lib.acc_cfk_apply_deps(c.handle, h, C.byref(upds[0])))
                for ui, q in zip(upds[1:], queries):
                    c.check(lib.acc_cfk_apply_deps(c.handle, h, C.byref(ui)))
                    torch.cuda.synchronize()
                    row = dict(queries=q["n"], pairs=q["pairs"], resident_ms=0.0, snapshot_ms=0.0, per_scan={})
                    for scan in scans:
                        outs = {}
                        for name, fn in routes:      # untimed: warms the route's buffers; the results are compared
                            fn(q, *scan[1:])
                            outs[name] = c.copy_out(kv, None)
                            if name == "resident":
                                st = c.stats()
                        for f in FIELDS:
                            if not np.array_equal(getattr(outs["resident"], f), getattr(outs["snapshot"], f)):
                                raise AssertionError(f"{scan[0]}: the routes differ in {f}")
                        if timing:
                            for name, fn in routes:
                                timed(fn, q, scan, tm[name])
                            continue
                        times = {name: [] for name, _ in routes}
                        for _ in range(reps):
                            for name, fn in routes:
                                times[name].append(timed(fn, q, scan))
                        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
                        row["resident_ms"] += med["resident"]
                        row["snapshot_ms"] += med["snapshot"]
                        row["per_scan"][scan[0]] = dict(resident_ms=round(med["resident"], 3), snapshot_ms=round(med["snapshot"], 3),
                                                        chunks=st.get("cfr.chunks", 0), hits=st.get("cfr.hits", 0),
                                                        sorted_hits=st.get("cfr.sorted_hits", 0))
                    if timing:
                        resident(q, *probe_free[1:])
                        timed(resident, q, probe_free, tm["resident_no_probe"])
                        first = {}
                        timed(resident, q, scans[0], first)
                        for k, v in first.items():
                            a = tm.setdefault("resident_first_scan", {}).setdefault(k, [0.0, 0])
                            a[0] += v[0]
                            a[1] += v[1]
                    v = L.BatchIn()
                    c.check(lib.acc_cfk_view(c.handle, h, C.byref(v)))
                    s = L.CfkSnap()
                    c.check(lib.acc_cfk_state(c.handle, h, C.byref(s)))
                    row.update(store_txns=int(v.n_txn), store_pairs=int(v.n_pairs), store_missing=int(s.n_missing))
                    rows.append(row)
            finally:
                lib.acc_cfk_destroy(h)
        return rows, tm

    rows, _ = run(False)
    _, tm = run(True)
    nb = len(rows)

    def top(d):
        return {k: round(x[0] / nb, 3) for k, x in sorted(d.items(), key=lambda kv: -kv[1][0])[:top_n]}

    res, snap = [round(r["resident_ms"], 3) for r in rows], [round(r["snapshot_ms"], 3) for r in rows]
    return {"workload": f"workload.cfk_update_stream({(n_init + batch * n_batches) // 1000}K txns x 8 {dist} keys over 1M keys): "
                        f"a {n_init // 1000}K-txn device store, then {n_batches} batches of {batch // 1000}K new txns; per batch "
                        f"acc_cfk_apply_deps, then {rows[0]['queries']} of the new txns recovered on their own keys at the four "
                        "BeginRecovery parameter sets (timed: the median of 5 per set and route, summed over the sets)",
            "resident_ms_per_batch": round(sum(res) / nb, 3), "snapshot_ms_per_batch": round(sum(snap) / nb, 3),
            "per_batch_resident_ms": res, "per_batch_snapshot_ms": snap,
            "per_batch": [{k: v for k, v in r.items() if k not in ("resident_ms", "snapshot_ms")} for r in rows],
            "resident_kernels_ms_per_batch": top(tm["resident"]), "snapshot_kernels_ms_per_batch": top(tm["snapshot"]),
            "resident_kernel_ms_per_batch": round(sum(x[0] for x in tm["resident"].values()) / nb, 3),
            "snapshot_kernel_ms_per_batch": round(sum(x[0] for x in tm["snapshot"].values()) / nb, 3),
            "first_scan_with_probes_ms_per_batch": top(tm.get("resident_first_scan", {})),
            "first_scan_without_probes_ms_per_batch": top(tm["resident_no_probe"]),
            "setup_gen_s": round(t_gen, 2)}


if __name__ == "__main__":
    dist = sys.argv[1] if len(sys.argv) > 1 else "uniform"
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    n_rec = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    print(json.dumps({dist: main(dist, nb, n_rec)}), flush=True)
