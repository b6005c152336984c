"""Time acc_cfk_notify at the bench's steady-state shape: python tools/cfk_notify_time.py [uniform|zipf] [reps]

The shape of bench.py's cfk_steady_leg: a device store of the first 1M txns of workload.cfk_update_stream(1.1M txns x 8
keys over 1M keys, dist), then the next batch of 100K txns applied (acc_cfk_apply_deps), inputs resident in HBM. On the
store after the batch, each a host clock around a call that ends synchronised:
  (a) acc_cfk_notify over the keys the batch touched (sorted unique, resident in HBM);
  (b) acc_cfk_notify over every key (key_code NULL);
  (c) the device-to-host copy of the acc_cfk_state columns alone (pinned destination, hipMemcpyAsync each, one
      synchronise): a floor under the only other route to the same answer, a read-back followed by a host notify per key.
      It is the same build's copy, not a rival implementation.
One untimed call of each warms every buffer; the figures are medians over `reps` (default 5) more, (a), (b), (c)
alternating. A last pass with every kernel timed (ACC_OPT_TIMING) gives the per-kernel split of (a) and (b), after one untimed
comparison of every output array of (b) under the forced sort tier with the default tiers (sort_tier_equals_default).
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


def main(dist="uniform", reps=5, n_init=1_000_000, batch=100_000, local=0):
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
    ni_touched = L.CfkNotifyIn(L.ACC_MEM_DEVICE, len(touched), up(touched), 0)
    ni_all = L.CfkNotifyIn(L.ACC_MEM_DEVICE, 0, None, 0)
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

    def one(timing):
        with Context(local, timing=timing) as c:
            lib = c._lib
            h = C.c_void_p()
            c.check(lib.acc_cfk_create(c.handle, C.byref(h)))
            try:
                c.check(lib.acc_cfk_apply_deps(c.handle, h, C.byref(ui)))
                c.check(lib.acc_cfk_apply_deps(c.handle, h, C.byref(un)))
                s, nv = L.CfkSnap(), L.CfkNotifyView()
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

                def notify(ni):
                    return lambda: c.check(lib.acc_cfk_notify(c.handle, h, C.byref(ni), C.byref(nv)))
                calls = dict(touched=notify(ni_touched), all=notify(ni_all), copy=copy)
                row = dict(keys=nk, entries=ne, missing=nm, keys_touched=len(touched), copy_bytes=sum(b for _, b in cols))
                if timing:
                    # not a timing: the sort tier alone against the default tiers, every event of every key
                    got = []
                    for tier in (0, L.ACC_NOTIFY_TIER_SORT):
                        ni = L.CfkNotifyIn(L.ACC_MEM_DEVICE, 0, None, tier)
                        c.check(lib.acc_cfk_notify(c.handle, h, C.byref(ni), C.byref(nv)))
                        n, k = int(nv.n_events), int(nv.n_keys)
                        got.append([device_array(c, ptr, cnt, dt) for ptr, cnt, dt in (
                            (nv.ev_entry, n, np.uint32), (nv.ev_txn, n, np.uint32), (nv.ev_pos, n, np.uint32), (nv.ev_kind, n, np.uint8),
                            (nv.ev_off, k + 1, np.uint64), (nv.next, k, np.uint32), (nv.next_write, k, np.uint32),
                            (nv.min_uncommitted, k, np.uint32), (nv.rel_keys, int(nv.n_txn), np.uint32))])
                    row["sort_tier_equals_default"] = all(np.array_equal(x, y) for x, y in zip(*got))
                    row["sort_tier_sorted"] = c.stats()["cfk.notify_sorted"]
                    for name in ("touched", "all"):
                        calls[name]()
                        c.timing_reset()
                        calls[name]()
                        c.sync()
                        row["kernels_ms_" + name] = {k: round(x[0], 3) for k, x in sorted(c.timing().items(), key=lambda kv: -kv[1][0])[:16]}
                    return row
                for f in calls.values():
                    f()
                ms = {k: [] for k in calls}
                for _ in range(reps):
                    for k, f in calls.items():
                        ms[k].append(clock(f))
                        if k != "copy":
                            st = c.stats()
                            row.update({f"{k}_{n}": st["cfk.notify_" + n] for n in ("keys", "candidates", "releases", "sorted")})
                            row[f"{k}_events"] = int(nv.n_events)
                for k, v in ms.items():
                    row[k + "_ms"] = round(median(v), 3)
                    row[k + "_ms_all"] = [round(x, 3) for x in v]
                return row
            finally:
                lib.acc_cfk_destroy(h)

    out = one(False)
    out.update(one(True))
    out["touched_over_copy"] = round(out["touched_ms"] / out["copy_ms"], 3)
    out["all_over_copy"] = round(out["all_ms"] / out["copy_ms"], 3)
    out["copy_GBps"] = round(out["copy_bytes"] / out["copy_ms"] / 1e6, 1)
    out["workload"] = (f"workload.cfk_update_stream({(n_init + batch) // 1000}K txns x 8 {dist} keys over 1M keys): a "
                       f"{n_init // 1000}K-txn device store and the next {batch // 1000}K-txn batch applied; acc_cfk_notify over "
                       f"the batch's keys, over every key, and the device-to-host copy of the acc_cfk_state columns")
    out["setup_gen_s"] = round(t_gen, 2)
    return out


if __name__ == "__main__":
    dist = sys.argv[1] if len(sys.argv) > 1 else "uniform"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    print(json.dumps({dist: main(dist, reps)}), flush=True)
