"""Time acc_rcmd_rangedeps against the whole-snapshot route: python tools/rcmd_query_time.py [batches] [reps]

The store: the first 1M txns of workload.rangedeps_batch(config 4's width mix, p_range = 1, one range each) as range
commands, applied by one acc_rcmd_update. Then `batches` batches of 100K new txns: half range txns x 1 range (the next rows
of that workload), half key txns x 4 keys (uniform over the key space, TxnIds beside the range txns' from a node no
stored txn has). Per batch the range txns' commands are applied first (acc_rcmd_update, timed once, with its split from
the ACC_OPT_TIMING events of that call), then the batch's 100K queries are answered, inputs resident in HBM, executeAt =
TxnId.

Timed in one process after a warm-up round, the variants alternating, the median of `reps` (>= 5) calls per batch each,
every call followed by a device synchronise (wall clock, no kernel events recorded):
  resident   acc_rcmd_rangedeps
  snapshot   what the library offered before: acc_rangedeps_batch over the table (acc_rcmd_view, every row PREACCEPTED,
             executeAt = TxnId) with the key queries appended, every column already in HBM and put together outside the
             timed window; the range queries are table rows there. It re-sorts the whole store and answers every row.
The query rows of both (per query its dictionary ids, deps as table indices and rangesToTxnIds) are hashed and must be
equal. Prints one JSON line."""
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
KEYS_PER_TXN = 4


def rows_digest(rows, offs_cols):
    """hash of the given rows of a CSR result: per (offsets, column) the rows' lengths and their elements in row order"""
    hs = hashlib.blake2b(digest_size=8)
    for off, col in offs_cols:
        start = off[rows].astype(np.int64)
        cnt = off[rows + 1].astype(np.int64) - start
        base = np.concatenate([[0], np.cumsum(cnt)])[:-1]
        idx = np.repeat(start - base, cnt) + np.arange(int(cnt.sum()), dtype=np.int64)
        hs.update(cnt.tobytes())
        hs.update(np.ascontiguousarray(col[idx]).tobytes())
    return hs.hexdigest()


def main(n_batches=5, reps=5, n_init=1_000_000, batch=100_000, local=0):
    import torch
    from accord_amd import _lib as L
    from accord_amd import workload as W
    from accord_amd.deps import Context, device_array
    t0 = time.perf_counter()
    half = batch // 2
    rb = W.rangedeps_batch(n_init + half * n_batches, W.CONFIG_SEEDS["4"], p_range=1.0, status_model="preaccepted")
    assert rb.is_range().all() and rb.n_ranges == rb.n_txn
    tm, tl, tn = rb.keys.txn_msb, rb.keys.txn_lsb, rb.keys.txn_node
    assert not np.any(tn == FOREIGN_NODE)
    rng = np.random.default_rng(0x5EED)
    cuts = [0, n_init] + [n_init + half * (b + 1) for b in range(n_batches)]
    dev = torch.device("cuda", local)
    keep = []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr()

    upds, queries, qrows = [], [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        n = b - a
        upds.append(L.RcmdUpdates(n, L.ACC_MEM_DEVICE, n, L.TsCols(up(tm[a:b]), up(tl[a:b]), up(tn[a:b])), up(np.zeros(n, np.uint8)),
                                  up(np.arange(n + 1, dtype=np.uint32)), up(rb.rng_start[a:b]), up(rb.rng_end[a:b])))
        if a == 0:
            continue
        # the batch's queries: its range txns, then as many key txns at the same times from a foreign node
        keys = np.sort(rng.integers(0, 1 << 32, size=(n, KEYS_PER_TXN), dtype=np.int64), axis=1)
        for j in range(1, KEYS_PER_TXN):
            keys[:, j] = np.maximum(keys[:, j], keys[:, j - 1] + 1)
        klsb = (tl[a:b] & np.uint64(0xFFFFFFFFFFFF0000)) | np.uint64(W.WRITE << 1)
        cat = lambda x, y, dt: np.concatenate([np.asarray(x, dt), np.asarray(y, dt)])  # noqa: E731
        q = dict(msb=cat(tm[a:b], tm[a:b], np.uint64), lsb=cat(tl[a:b], klsb, np.uint64),
                 node=cat(tn[a:b], np.full(n, FOREIGN_NODE), np.int32),
                 key_off=cat(np.zeros(n + 1), KEYS_PER_TXN * np.arange(1, n + 1), np.uint32), key=keys.reshape(-1).astype(np.uint64),
                 rng_off=cat(np.arange(n + 1), np.full(n, n), np.uint32))
        qrows.append(q)
        queries.append(L.CfkMixedQueries(2 * n, L.ACC_MEM_DEVICE, n * KEYS_PER_TXN, n, L.TsCols(up(q["msb"]), up(q["lsb"]), up(q["node"])),
                                         L.TsCols(None, None, None), up(q["key_off"]), up(q["key"]), up(q["rng_off"]),
                                         up(rb.rng_start[a:b]), up(rb.rng_end[a:b]), int(rb.end_inclusive), 0))
    t_gen = time.perf_counter() - t0
    torch.cuda.synchronize()
    variants = ("resident", "snapshot")
    rows = []
    with Context(local, timing=True) as c:
        lib = c._lib
        h = C.c_void_p()
        c.check(lib.acc_rcmd_create(c.handle, int(rb.end_inclusive), C.byref(h)))
        try:
            def update(ui):
                """one acc_rcmd_update: wall ms and the split of its kernel events"""
                c.timing_filter(None)
                c.timing_reset()
                t = time.perf_counter()
                c.check(lib.acc_rcmd_update(c.handle, h, C.byref(ui)))
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t) * 1e3
                split = dict(table_merge=0.0, index_rebuild=0.0, shared_scans=0.0)
                for name, (kms, _) in c.timing().items():
                    part = ("index_rebuild" if name.startswith(("rd_", "rs_rd")) else
                            "shared_scans" if name in ("scan", "iota") else "table_merge")
                    split[part] += kms
                c.timing_filter(["-"])     # no launch carries this tag: the queries below record no events
                return ms, {k: round(v, 3) for k, v in split.items()}, c.stats()

            init_ms, init_split, _ = update(upds[0])
            rv, sv = L.RangedepsView(), L.RangedepsView()
            for b, (ui, qi, q) in enumerate(zip(upds[1:], queries, qrows)):
                upd_ms, split, ust = update(ui)
                tv = L.RcmdTable()
                c.check(lib.acc_rcmd_view(c.handle, h, C.byref(tv)))
                n, R, nk = int(tv.n_cmd), int(tv.n_ranges), half
                assert n == cuts[b + 2] and R == n
                g = lambda ptr, cnt, dt: device_array(c, ptr, cnt, dt)  # noqa: E731
                mark = len(keep)
                cat = lambda x, y, dt: up(np.concatenate([np.asarray(x, dt), np.asarray(y, dt)]))  # noqa: E731
                ids = L.TsCols(cat(g(tv.txn_id.msb, n, np.uint64), q["msb"][half:], np.uint64),
                               cat(g(tv.txn_id.lsb, n, np.uint64), q["lsb"][half:], np.uint64),
                               cat(g(tv.txn_id.node, n, np.int32), q["node"][half:], np.int32))
                snap = L.RangeBatchIn(n + nk, L.ACC_MEM_DEVICE, nk * KEYS_PER_TXN, R, ids, ids, up(np.full(n + nk, W.PREACCEPTED, np.uint8)),
                                      cat(np.zeros(n), q["key_off"][half:], np.uint32), up(q["key"]),
                                      cat(g(tv.rng_off, n + 1, np.uint32), np.full(nk, R), np.uint32),
                                      up(g(tv.rng_start, R, np.uint64)), up(g(tv.rng_end, R, np.uint64)), int(rb.end_inclusive), 0)
                torch.cuda.synchronize()
                times = {k: [] for k in variants}
                hashes, qst = {}, {}
                for rep in range(reps + 1):                      # round 0 warms both variants' buffers, untimed
                    for k in variants:
                        t = time.perf_counter()
                        if k == "resident":
                            c.check(lib.acc_rcmd_rangedeps(c.handle, h, C.byref(qi), C.byref(rv)))
                        else:
                            c.check(lib.acc_rangedeps_batch(c.handle, C.byref(snap), C.byref(sv)))
                        torch.cuda.synchronize()
                        if rep:
                            times[k].append((time.perf_counter() - t) * 1e3)
                            continue
                        view = rv if k == "resident" else sv
                        r = c.copy_out_range(view)
                        # the batch's range txns are the table's last `half` rows; its key txns follow the table in the snapshot
                        qr = np.arange(2 * half) if k == "resident" else np.concatenate([np.arange(n - half, n), np.arange(n, n + nk)])
                        hashes[k] = rows_digest(qr, ((r.rd_off, r.range_id), (r.u_off, r.dep_txn), (r.arena_off, r.arena)))
                        hashes[k + "_dict"] = hashlib.blake2b(r.rng_start.tobytes() + r.rng_end.tobytes(), digest_size=8).hexdigest()
                        if k == "resident":
                            qst = c.stats()
                            deps = int(view.total_deps)
                assert hashes["resident"] == hashes["snapshot"], f"batch {b}: the query rows differ: {hashes}"
                assert hashes["resident_dict"] == hashes["snapshot_dict"], f"batch {b}: the dictionaries differ"
                del keep[mark:]
                rows.append(dict(store_cmds=n, stored_ranges=int(tv.n_dict), queries=int(qi.n_query), deps=deps,
                                 raw_entries=qst.get("rangedeps.raw_entries", 0), hash=hashes["resident"],
                                 update_ms=round(upd_ms, 3), update_split_kernel_ms=split, inserted=ust.get("rcmd.inserted", 0),
                                 ms={k: [round(x, 3) for x in sorted(v)] for k, v in times.items()}))
        finally:
            lib.acc_rcmd_destroy(h)
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    summary = {k: round(sum(med(r["ms"][k]) for r in rows) / len(rows), 3) for k in variants}
    spread = {k: round(max(max(r["ms"][k]) / min(r["ms"][k]) for r in rows), 3) for k in variants}
    splits = {k: round(med([r["update_split_kernel_ms"][k] for r in rows]), 3) for k in ("table_merge", "index_rebuild", "shared_scans")}
    return {"workload": f"workload.rangedeps_batch({(n_init + half * n_batches) // 1000}K range txns x 1 range, config 4's widths): a "
                        f"{n_init // 1000}K-command device store, then {n_batches} batches of {batch // 1000}K new txns (half range txns x 1 "
                        f"range, half key txns x {KEYS_PER_TXN} keys); per batch acc_rcmd_update of its range commands, then the "
                        f"batch's queries (timed, median of {reps} per batch, mean over the batches)",
            "median_ms": summary, "max_over_min_of_repeats": spread, "query_rows_equal": True,
            "update_ms_median": round(med([r["update_ms"] for r in rows]), 3), "update_split_kernel_ms_median": splits,
            "initial_update_ms": round(init_ms, 3), "initial_update_split_kernel_ms": init_split, "per_batch": rows,
            "setup_gen_s": round(t_gen, 2)}


if __name__ == "__main__":
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    print(json.dumps(main(nb, max(reps, 5))), flush=True)
