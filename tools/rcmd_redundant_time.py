"""Time acc_rcmd_redundant_before on a large resident range-command store: python tools/rcmd_redundant_time.py [reps] [n_cmd]

A device store of n_cmd (default 1M) range commands with state: command i is a Write at hlc 1000 + i with two ranges of
up to 64 key codes at pseudo-random places of a 2^26 key space, a status and one dep; the columns are resident in HBM
(ACC_MEM_DEVICE). The prune takes 4,096 input ranges, each three quarters of its 2^14-wide stripe, all with the store's
median TxnId as the bound: the older half of the commands loses about three quarters of its ranges (most of those rows
leave, the rest are cut), the younger half stays. Per repetition, on a fresh store (a prune changes it):
  rangedeps of a fixed batch of 10,000 queries (half keys, half ranges) and acc_rcmd_update_cmds of a fixed batch of
  2,000 commands above every stored TxnId, each warm (applied once untimed, then the median of 3), before the prune;
  one acc_rcmd_redundant_before: wall clock (synchronised) and the stream time of its two halves (stats
  rcmd.redundant_prune_us / rcmd.redundant_index_us);
  the same rangedeps and update_cmds after the prune;
  the only way to the same store without the call: a fresh acc_rcmd fed the surviving table (device columns) by one
  acc_rcmd_update_cmds, wall clock.
One untimed repetition first warms every buffer; the figures are medians over `reps` (default 3) more. A last
repetition with every kernel timed (ACC_OPT_TIMING) gives the prune's kernel breakdown. It checks no result
(tests/test_rcmd_redundant_gpu.py does). Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cassandra-accord_amd")]

SPACE_BITS, STRIPE_BITS = 26, 14


def median(x):
    return sorted(x)[len(x) // 2]


def commands(n, hlc0, W):
    """n commands from hlc0 up, in TxnId order, as the RangeCmdStore.update dict with state columns"""
    i = np.arange(n, dtype=np.uint64)
    m, l, nd = W.encode_ts(1, i + np.uint64(hlc0), (W.WRITE << 1) | 1, np.ones(n, np.int32))
    a = (i * np.uint64(2654435761)) % np.uint64((1 << SPACE_BITS) - 400)
    w = np.uint64(1) + (i * np.uint64(40503)) % np.uint64(64)
    rs = np.stack([a, a + np.uint64(200)], 1).reshape(-1)
    re_ = rs + np.repeat(w, 2)
    dm, dl, dn = W.encode_ts(1, np.uint64(1) + i % np.uint64(997), W.WRITE << 1, np.ones(n, np.int32))
    return dict(msb=m, lsb=l, node=nd, flags=np.full(n, 2, np.uint8), rng_off=(2 * np.arange(n + 1)).astype(np.uint32),
                rng_start=rs, rng_end=re_, status=(i % np.uint64(9)).astype(np.uint8) + np.uint8(1), xmsb=m, xlsb=l, xnode=nd,
                dep_off=np.arange(n + 1, dtype=np.uint32), dep_msb=dm, dep_lsb=dl, dep_node=dn, dep_start=a, dep_end=np.zeros(n, np.uint64),
                dep_is_key=np.ones(n, np.uint8))


def main(reps=3, n_cmd=1_000_000, local=0):
    import torch
    from accord_amd import _lib as L
    from accord_amd import workload as W
    from accord_amd.deps import Context, RangeCmdStore, _mixed_queries_in
    assert L.ACC_RCMD_HAS_DEPS == 2
    dev = torch.device("cuda", local)
    keep = []

    def device_updates(u):
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in u.items()}
        keep.append(t)
        p = lambda k: t[k].data_ptr()  # noqa: E731
        return L.RcmdCmdUpdates(len(u["msb"]), L.ACC_MEM_DEVICE, len(u["rng_start"]), L.TsCols(p("msb"), p("lsb"), p("node")),
                                p("flags"), p("rng_off"), p("rng_start"), p("rng_end"), L.TsCols(p("xmsb"), p("xlsb"), p("xnode")),
                                p("status"), len(u["dep_msb"]), p("dep_off"), L.TsCols(p("dep_msb"), p("dep_lsb"), p("dep_node")),
                                p("dep_start"), p("dep_end"), p("dep_is_key"))

    full = commands(n_cmd, 1000, W)
    ui_full = device_updates(full)
    ui_small = device_updates(commands(2000, 1000 + n_cmd + 10, W))
    mid = n_cmd // 2
    nj = 1 << (SPACE_BITS - STRIPE_BITS)
    s0 = (np.arange(nj, dtype=np.uint64) << np.uint64(STRIPE_BITS))
    ranges = dict(rng_start=s0, rng_end=s0 + np.uint64(3 << (STRIPE_BITS - 2)), msb=np.full(nj, full["msb"][mid], np.uint64),
                  lsb=np.full(nj, full["lsb"][mid], np.uint64), node=np.full(nj, full["node"][mid], np.int32))
    rng = np.random.default_rng(1)
    nq = 10_000
    qm, ql, qn = W.encode_ts(1, np.uint64(1000 + n_cmd + 5000) + np.arange(nq, dtype=np.uint64),
                             (W.WRITE << 1) | (np.arange(nq, dtype=np.uint64) & np.uint64(1)), np.full(nq, 3, np.int32))
    at = rng.integers(0, (1 << SPACE_BITS) - 400, size=nq).astype(np.uint64)
    isr = (np.arange(nq) & 1).astype(bool)
    csum = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.uint32)  # noqa: E731
    q = dict(msb=qm, lsb=ql, node=qn, key_off=csum(~isr), key_code=at[~isr], rng_off=csum(isr), rng_start=at[isr],
             rng_end=at[isr] + np.uint64(300))
    torch.cuda.synchronize()

    def wall(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def one(timing):
        with Context(local, timing=timing) as c:
            lib = c._lib
            s = RangeCmdStore(c, 0)
            qi = _mixed_queries_in(q, 0, 0, keep)
            view = L.RangedepsView()
            query = lambda: c.check(lib.acc_rcmd_rangedeps(c.handle, s._h, C.byref(qi), C.byref(view)))  # noqa: E731
            small = lambda: c.check(lib.acc_rcmd_update_cmds(c.handle, s._h, C.byref(ui_small)))  # noqa: E731
            try:
                c.check(lib.acc_rcmd_update_cmds(c.handle, s._h, C.byref(ui_full)))
                query(); small()
                row = dict(rangedeps_before_ms=median([wall(query) for _ in range(3)]), deps_before=int(view.total_deps),
                           update_before_ms=median([wall(small) for _ in range(3)]))
                v = s.view()
                row.update(cmds=int(v.n_cmd), ranges=int(v.n_ranges), deps=int(s.state_view().n_deps))
                c.timing_reset()
                row["redundant_before_ms"] = wall(lambda: s.redundant_before(ranges))
                st = c.stats()
                tm = c.timing() if timing else {}
                row.update(prune_ms=st["rcmd.redundant_prune_us"] / 1e3, index_ms=st["rcmd.redundant_index_us"] / 1e3,
                           cmds_cut=st["rcmd.redundant_cmds_cut"], cmds_dropped=st["rcmd.redundant_cmds_dropped"],
                           ranges_after=st["rcmd.redundant_ranges_after"])
                query(); small()
                row.update(rangedeps_after_ms=median([wall(query) for _ in range(3)]), deps_after=int(view.total_deps),
                           update_after_ms=median([wall(small) for _ in range(3)]))
                # the surviving table without the 2,000 late commands would be the fairer input; they are 0.2% of it
                tab, sta = s.table(), s.state()
                surv = dict(msb=tab["msb"], lsb=tab["lsb"], node=tab["node"], flags=sta["flags"], rng_off=tab["rng_off"],
                            rng_start=tab["rng_start"], rng_end=tab["rng_end"], status=sta["status"], xmsb=sta["xmsb"], xlsb=sta["xlsb"],
                            xnode=sta["xnode"], **{k: sta[k] for k in ("dep_off", "dep_msb", "dep_lsb", "dep_node", "dep_start",
                                                                        "dep_end", "dep_is_key")})
                ui_surv = device_updates(surv)
                f = RangeCmdStore(c, 0)
                try:
                    row["rebuild_ms"] = wall(lambda: c.check(lib.acc_rcmd_update_cmds(c.handle, f._h, C.byref(ui_surv))))
                    row["cmds_after"] = int(f.view().n_cmd)
                finally:
                    f.close()
                    keep.pop()
                return row, tm
            finally:
                s.close()

    one(False)
    rows = [one(False)[0] for _ in range(reps)]
    _, tm = one(True)
    out = dict(rows[0])
    for k in ("redundant_before_ms", "prune_ms", "index_ms", "rebuild_ms", "update_before_ms", "update_after_ms",
              "rangedeps_before_ms", "rangedeps_after_ms"):
        out[k] = round(median([r[k] for r in rows]), 3)
        out[k + "_all"] = [round(r[k], 3) for r in rows]
    out["kernels_ms"] = {k: round(x[0], 3) for k, x in sorted(tm.items(), key=lambda kv: -kv[1][0])[:14]}
    out["workload"] = (f"{n_cmd // 1000}K range commands x 2 ranges x 1 dep in a device store; acc_rcmd_redundant_before of {nj} "
                       f"ranges with the median TxnId; acc_rcmd_update_cmds of 2,000 commands and acc_rcmd_rangedeps of {nq} queries "
                       f"before and after; a fresh store fed the surviving table")
    return out


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    n_cmd = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    print(json.dumps(main(reps, n_cmd)), flush=True)
