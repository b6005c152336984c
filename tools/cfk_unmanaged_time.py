"""Time acc_cfk_register_unmanaged / acc_cfk_notify_unmanaged at the bench's steady-state shape:
python tools/cfk_unmanaged_time.py [uniform|zipf] [reps]

The shape of bench.py's cfk_steady_leg: a device store of the first 1M txns of workload.cfk_update_stream(1.1M txns x 8
keys over 1M keys, dist), inputs resident in HBM. Per repetition, on a fresh store, each a host clock around a call that
ends synchronised:
  (a) acc_cfk_register_unmanaged of one ExclusiveSyncPoint above every stored TxnId over every key of the store, its deps
      on a key = that key's entries (the waiter's key and dep arrays are the store's own acc_cfk_state columns, DEVICE
      memory): the sync-point shape, one pair per key;
  then the next batch of 100K txns applied (acc_cfk_apply_deps, untimed);
  (b) acc_cfk_notify_unmanaged over the keys that batch touched (sorted unique, resident in HBM), and (b2) the same call
      again, when nothing has changed;
  (c) the device-to-host copy of the acc_cfk_state columns alone (pinned destination, hipMemcpyAsync each, one
      synchronise): a floor under the only other route, a read-back followed by a host registerUnmanaged /
      notifyUnmanaged per key. It is the same build's copy, not a rival implementation.
One untimed repetition warms every buffer; the figures are medians over `reps` (default 3) more. A last repetition with
every kernel timed (ACC_OPT_TIMING) gives the per-kernel split of (a) and (b).
Prints one JSON line; no time or ratio is asserted."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cassandra-accord_amd")]


def median(x):
    return sorted(x)[len(x) // 2]


def main(dist="uniform", reps=3, n_init=1_000_000, batch=100_000, local=0):
    import torch
    from accord_amd import _lib as L
    from accord_amd import workload as W
    from accord_amd.deps import Context, device_array
    t0 = time.perf_counter()
    u = W.cfk_update_stream(n_init + batch, 8, 1_000_000, dist=dist)
    cuts = W.cfk_stream_cuts(u, n_init, batch, 1)
    init, nxt = W.cfk_slice(u, 0, cuts[0]), W.cfk_slice(u, cuts[0], cuts[1])
    touched = np.unique(np.asarray(nxt["key"], np.uint64))
    t_gen = time.perf_counter() - t0
    dev = torch.device("cuda", local)
    keep = []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr()

    def updates(part):
        P = {k: up(v) for k, v in part.items()}
        return L.CfkUpdates(L.ACC_MEM_DEVICE, len(part["msb"]), len(part["key"]), len(part["dmsb"]),
                            L.TsCols(P["msb"], P["lsb"], P["node"]), L.TsCols(P["xmsb"], P["xlsb"], P["xnode"]),
                            P["status"], P["flags"], P["key_off"], P["key"], P["dep_off"], L.TsCols(P["dmsb"], P["dlsb"], P["dnode"]))

    ui, un = updates(init), updates(nxt)
    ni_touched = L.CfkUnmanagedNotifyIn(L.ACC_MEM_DEVICE, len(touched), up(touched))
    # the ExclusiveSyncPoint: a range-domain TxnId above every TxnId of the stream
    w_msb = up(np.array([int(np.max(u["msb"])) + 1], np.uint64))
    w_lsb = up(np.array([(4 << 1) | 1], np.uint64))   # Kind ordinal 4 = ExclusiveSyncPoint, domain bit = Range
    w_node = up(np.array([1], np.int32))
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    D2H = 2   # hipMemcpyDeviceToHost

    def clock(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def one(c, timing):
        """one repetition on a fresh store: {register, notify, notify_again, copy: ms} and the counts"""
        lib = c._lib
        h = C.c_void_p()
        c.check(lib.acc_cfk_create(c.handle, C.byref(h)))
        try:
            c.check(lib.acc_cfk_apply_deps(c.handle, h, C.byref(ui)))
            s = L.CfkSnap()
            c.check(lib.acc_cfk_state(c.handle, h, C.byref(s)))
            nk, ne, nm = int(s.n_keys), int(s.n_entries), int(s.n_missing)
            key_off = up(np.array([0, nk], np.uint32))
            wi = L.CfkUnmanagedIn(L.ACC_MEM_DEVICE, 1, nk, ne, L.TsCols(w_msb, w_lsb, w_node), L.TsCols(w_msb, w_lsb, w_node),
                                  key_off, s.key, s.ent_off, s.txn_id, 0)
            wo, ev = L.CfkUnmanagedOut(), L.CfkUnmanagedEvents()
            row = dict(keys=nk, entries=ne, missing=nm, keys_touched=len(touched))
            ms = {}
            if timing:
                c.timing_reset()
            ms["register"] = clock(lambda: c.check(lib.acc_cfk_register_unmanaged(c.handle, h, C.byref(wi), C.byref(wo))))
            st = c.stats()
            row.update({"register_" + n: st["cfk.unmanaged_" + n] for n in ("pairs", "ready", "pending_commit", "pending_apply",
                                                                            "tk_inserted", "records")})
            if timing:
                c.sync()
                row["kernels_ms_register"] = {k: round(x[0], 3) for k, x in sorted(c.timing().items(), key=lambda kv: -kv[1][0])[:12]}
            c.check(lib.acc_cfk_apply_deps(c.handle, h, C.byref(un)))
            if timing:
                c.sync()
                c.timing_reset()
            ms["notify"] = clock(lambda: c.check(lib.acc_cfk_notify_unmanaged(c.handle, h, C.byref(ni_touched), C.byref(ev))))
            st = c.stats()
            row.update({"notify_" + n: st["cfk.unmanaged_" + n] for n in ("reevaluated", "released", "records")})
            row["notify_events"] = int(ev.n_events)
            if timing:
                c.sync()
                row["kernels_ms_notify"] = {k: round(x[0], 3) for k, x in sorted(c.timing().items(), key=lambda kv: -kv[1][0])[:12]}
            ms["notify_again"] = clock(lambda: c.check(lib.acc_cfk_notify_unmanaged(c.handle, h, C.byref(ni_touched), C.byref(ev))))
            row["notify_again_events"] = int(ev.n_events)
            c.check(lib.acc_cfk_state(c.handle, h, C.byref(s)))
            nk, ne, nm = int(s.n_keys), int(s.n_entries), int(s.n_missing)
            cols = [(s.key, nk * 8), (s.ent_off, (nk + 1) * 4), (s.txn_id.msb, ne * 8), (s.txn_id.lsb, ne * 8),
                    (s.txn_id.node, ne * 4), (s.execute_at.msb, ne * 8), (s.execute_at.lsb, ne * 8), (s.execute_at.node, ne * 4),
                    (s.status, ne), (s.miss_off, (ne + 1) * 4), (s.missing.msb, nm * 8), (s.missing.lsb, nm * 8),
                    (s.missing.node, nm * 4)]
            dst = [torch.empty(max(b, 1), dtype=torch.uint8).pin_memory() for _, b in cols]

            def copy():
                for (p, b), d in zip(cols, dst):
                    if b and hip.hipMemcpyAsync(d.data_ptr(), p, b, D2H, None):
                        raise RuntimeError("hipMemcpyAsync failed")
            copy()
            ms["copy"] = clock(copy)
            row["copy_bytes"] = sum(b for _, b in cols)
            return ms, row
        finally:
            lib.acc_cfk_destroy(h)

    out = {}
    with Context(local) as c:
        one(c, False)
        runs = [one(c, False) for _ in range(reps)]
    for k in runs[0][0]:
        out[k + "_ms"] = round(median([m[k] for m, _ in runs]), 3)
        out[k + "_ms_all"] = [round(m[k], 3) for m, _ in runs]
    out.update(runs[-1][1])
    with Context(local, timing=True) as c:
        _, row = one(c, True)
        out["kernels_ms_register"], out["kernels_ms_notify"] = row["kernels_ms_register"], row["kernels_ms_notify"]
    out["register_over_copy"] = round(out["register_ms"] / out["copy_ms"], 3)
    out["notify_over_copy"] = round(out["notify_ms"] / out["copy_ms"], 3)
    out["copy_GBps"] = round(out["copy_bytes"] / out["copy_ms"] / 1e6, 1)
    out["workload"] = (f"workload.cfk_update_stream({(n_init + batch) // 1000}K txns x 8 {dist} keys over 1M keys): a "
                       f"{n_init // 1000}K-txn device store; one ExclusiveSyncPoint registered over every key with deps = each "
                       f"key's entries; the next {batch // 1000}K-txn batch applied; acc_cfk_notify_unmanaged over the batch's "
                       f"keys; the device-to-host copy of the acc_cfk_state columns")
    out["setup_gen_s"] = round(t_gen, 2)
    return out


if __name__ == "__main__":
    dist = sys.argv[1] if len(sys.argv) > 1 else "uniform"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    print(json.dumps({dist: main(dist, reps)}), flush=True)
