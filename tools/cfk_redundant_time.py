"""Time acc_cfk_redundant_before at the bench's steady-state shape: python tools/cfk_redundant_time.py [uniform|zipf] [reps]

The shape of bench.py's cfk_steady_leg: a device store of the first 1M txns of workload.cfk_update_stream(1.1M txns x 8
keys over 1M keys, dist), inputs resident in HBM. Per repetition, on a fresh store (a prune changes it):
  (b) acc_cfk_keydeps of the next batch's 100K new txns (workload.preaccept_queries) against the store, before the prune;
  a plain device-to-device copy of the store's 13 key-major columns (hipMemcpyAsync each, one synchronise): the yardstick;
  (a) one acc_cfk_redundant_before over every key with the store's median TxnId as the bound, which drops about half
      of the entries: wall clock (synchronised) and the stream time of its two halves (stats cfk.redundant_prune_us /
      cfk.redundant_view_us, the events acc_cfk_apply_deps uses for cfk.apply_us / cfk.view_us);
  (b) the same acc_cfk_keydeps after the prune.
One untimed repetition first warms every buffer; the figures are medians over `reps` (default 3) more. A last
repetition with every kernel timed (ACC_OPT_TIMING) gives the prune's kernel breakdown. Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cassandra-accord_amd")]

ENTRY_BYTES = 4 * 8 + 2 * 4 + 1 + 4     # TxnId / executeAt msb, lsb; their nodes; status; miss_off
MISSING_BYTES = 2 * 8 + 4
KEY_BYTES = 8 + 4


def median(x):
    return sorted(x)[len(x) // 2]


def main(dist="uniform", reps=3, n_init=1_000_000, batch=100_000, local=0):
    import torch
    from accord_amd import _lib as L
    from accord_amd import workload as W
    from accord_amd.deps import Context, _execute_at_after, device_array
    t0 = time.perf_counter()
    u = W.cfk_update_stream(n_init + batch, 8, 1_000_000, dist=dist)
    cuts = W.cfk_stream_cuts(u, n_init, batch, 1)
    init, nxt = W.cfk_slice(u, 0, cuts[0]), W.cfk_slice(u, cuts[0], cuts[1])
    q = W.preaccept_queries(nxt)
    xm, xl, xn = _execute_at_after(nxt, q)
    t_gen = time.perf_counter() - t0
    dev = torch.device("cuda", local)
    keep = []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr()

    P = {k: up(v) for k, v in init.items()}
    ui = L.CfkUpdates(L.ACC_MEM_DEVICE, len(init["msb"]), len(init["key"]), len(init["dmsb"]),
                      L.TsCols(P["msb"], P["lsb"], P["node"]), L.TsCols(P["xmsb"], P["xlsb"], P["xnode"]),
                      P["status"], P["flags"], P["key_off"], P["key"], P["dep_off"], L.TsCols(P["dmsb"], P["dlsb"], P["dnode"]))
    qi = L.CfkQueries(len(q["msb"]), L.ACC_MEM_DEVICE, len(q["part_start"]), L.TsCols(up(q["msb"]), up(q["lsb"]), up(q["node"])),
                      L.TsCols(up(xm), up(xl), up(xn)), up(q["part_off"].astype(np.uint32)), up(q["part_start"].astype(np.uint64)))
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    D2D = 3   # hipMemcpyDeviceToDevice

    def timed(f, n=3):
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return median(out)

    def one(timing):
        with Context(local, timing=timing) as c:
            lib = c._lib
            h = C.c_void_p()
            c.check(lib.acc_cfk_create(c.handle, C.byref(h)))
            try:
                kv, s, v = L.KeydepsView(), L.CfkSnap(), L.BatchIn()
                c.check(lib.acc_cfk_apply_deps(c.handle, h, C.byref(ui)))
                scan = lambda: c.check(lib.acc_cfk_keydeps(c.handle, h, C.byref(qi), C.byref(kv)))  # noqa: E731
                scan()                                                  # warm the query's buffers
                row = dict(keydeps_before_ms=timed(scan), deps_before=int(kv.total_deps))
                c.check(lib.acc_cfk_state(c.handle, h, C.byref(s)))
                c.check(lib.acc_cfk_view(c.handle, h, C.byref(v)))
                nk, ne, nm = int(s.n_keys), int(s.n_entries), int(s.n_missing)
                cols = [(s.key, nk * 8), (s.ent_off, (nk + 1) * 4), (s.txn_id.msb, ne * 8), (s.txn_id.lsb, ne * 8),
                        (s.txn_id.node, ne * 4), (s.execute_at.msb, ne * 8), (s.execute_at.lsb, ne * 8), (s.execute_at.node, ne * 4),
                        (s.status, ne), (s.miss_off, (ne + 1) * 4), (s.missing.msb, nm * 8), (s.missing.lsb, nm * 8),
                        (s.missing.node, nm * 4)]
                dst = [torch.empty(max(b, 1), dtype=torch.uint8, device=dev) for _, b in cols]

                def copy():
                    for (p, b), d in zip(cols, dst):
                        if b and hip.hipMemcpyAsync(d.data_ptr(), p, b, D2D, None):
                            raise RuntimeError("hipMemcpyAsync failed")
                copy()
                row.update(copy_ms=timed(copy), copy_bytes=sum(b for _, b in cols), keys=nk, entries=ne, missing=nm,
                           store_txns=int(v.n_txn))
                n = int(v.n_txn)
                mid = [device_array(c, p + (n // 2) * sz, 1, dt) for p, sz, dt in
                       ((v.txn_id.msb, 8, np.uint64), (v.txn_id.lsb, 8, np.uint64), (v.txn_id.node, 4, np.int32))]
                a = dict(rs=np.array([0], np.uint64), re=np.array([2 ** 64 - 1], np.uint64), bm=mid[0], bl=mid[1], bn=mid[2])
                ri = L.CfkRedundantIn(L.ACC_MEM_HOST, 1, 0, a["rs"].ctypes.data, a["re"].ctypes.data,
                                      L.TsCols(a["bm"].ctypes.data, a["bl"].ctypes.data, a["bn"].ctypes.data))
                c.timing_reset()
                torch.cuda.synchronize()
                t = time.perf_counter()
                c.check(lib.acc_cfk_redundant_before(c.handle, h, C.byref(ri)))
                torch.cuda.synchronize()
                row["redundant_before_ms"] = (time.perf_counter() - t) * 1e3
                st = c.stats()
                tm = c.timing() if timing else {}
                c.check(lib.acc_cfk_state(c.handle, h, C.byref(s)))
                c.check(lib.acc_cfk_view(c.handle, h, C.byref(v)))
                nk2, ne2, nm2 = int(s.n_keys), int(s.n_entries), int(s.n_missing)
                row.update(prune_ms=st["cfk.redundant_prune_us"] / 1e3, view_ms=st["cfk.redundant_view_us"] / 1e3,
                           keys_advanced=st["cfk.redundant_keys_advanced"], entries_dropped=st["cfk.redundant_entries_dropped"],
                           missing_dropped=st["cfk.redundant_missing_dropped"], keys_after=nk2, entries_after=ne2,
                           missing_after=nm2, store_txns_after=int(v.n_txn),
                           # the segmented copies read and write every surviving element once
                           prune_copy_bytes=2 * (nk2 * KEY_BYTES + ne2 * ENTRY_BYTES + nm2 * MISSING_BYTES))
                scan()
                row.update(keydeps_after_ms=timed(scan), deps_after=int(kv.total_deps))
                return row, tm
            finally:
                lib.acc_cfk_destroy(h)

    one(False)
    rows = [one(False)[0] for _ in range(reps)]
    _, tm = one(True)
    out = dict(rows[0])
    for k in ("keydeps_before_ms", "copy_ms", "redundant_before_ms", "prune_ms", "view_ms", "keydeps_after_ms"):
        out[k] = round(median([r[k] for r in rows]), 3)
        out[k + "_all"] = [round(r[k], 3) for r in rows]
    out["prune_over_copy"] = round(out["prune_ms"] / out["copy_ms"], 3)
    out["call_over_copy"] = round(out["redundant_before_ms"] / out["copy_ms"], 3)
    out["copy_GBps"] = round(2 * out["copy_bytes"] / out["copy_ms"] / 1e6, 1)
    out["kernels_ms"] = {k: round(x[0], 3) for k, x in sorted(tm.items(), key=lambda kv: -kv[1][0])[:14]}
    out["workload"] = (f"workload.cfk_update_stream({(n_init + batch) // 1000}K txns x 8 {dist} keys over 1M keys): a "
                       f"{n_init // 1000}K-txn device store; acc_cfk_redundant_before with the median TxnId over every key; "
                       f"acc_cfk_keydeps of the next {batch // 1000}K new txns before and after")
    out["setup_gen_s"] = round(t_gen, 2)
    return out


if __name__ == "__main__":
    dist = sys.argv[1] if len(sys.argv) > 1 else "uniform"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    print(json.dumps({dist: main(dist, reps)}), flush=True)
