"""Time acc_cfk_keydeps_mixed at the bench's steady-state shape: python tools/cfk_range_query_time.py [uniform|zipf] [batches] [reps]

The store of tools/cfk_query_time.py: the first 1M txns of workload.cfk_update_stream(1M + batches x 100K txns x 8 keys
over 1M keys, dist), then `batches` batches of 100K new txns, inputs resident in HBM. Per batch, after
acc_cfk_apply_deps, one call answers the batch's new key queries plus 1,000 range queries (SyncPoints) of 1,000
consecutive covered store keys each, plus one range query (an ExclusiveSyncPoint) over the whole key space. The range
txns take the times of new txns of the batch from a node no stored txn has, so no stored executeAt ties with them.

Timed in one process after a warm-up call, the variants alternating, the median of `reps` (>= 5) calls per batch each,
every call followed by a device synchronise (wall clock):
  lane_<n>   acc_cfk_keydeps_mixed with lane_seg = n in 1, 8, 16, 32, 64, 256
  lane_none  acc_cfk_keydeps_mixed with lane_seg = ACC_CFQ_LANE_NONE (every pair on the wave-per-chunk path)
  snapshot   what the library offered before: acc_keydeps_mixed over the store's txn-major view with the range txns
             appended (every column resident in HBM, put together outside the timed window), which sorts and scans the
             whole store and answers every txn of it
Every acc_cfk_keydeps_mixed variant's copied-out arrays are hashed per batch and must be bit-equal; the range txns' rows
are also compared with the snapshot route's (range_rows_equal_snapshot). Prints one JSON line."""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cassandra-accord_amd")]

LANES = (1, 8, 16, 32, 64, 256)
N_RANGE, SPAN = 1_000, 1_000
FOREIGN_NODE = 30_000


def main(dist="uniform", n_batches=2, reps=5, n_init=1_000_000, batch=100_000, local=0):
    import torch
    from accord_amd import _lib as L
    from accord_amd import workload as W
    from accord_amd.deps import AccordError, Context, _execute_at_after, device_array
    t0 = time.perf_counter()
    u = W.cfk_update_stream(n_init + batch * n_batches, 8, 1_000_000, dist=dist)
    assert not np.any(u["node"] == FOREIGN_NODE) and not np.any(u["xnode"] == FOREIGN_NODE)
    cuts = W.cfk_stream_cuts(u, n_init, batch, n_batches)
    parts = [W.cfk_slice(u, 0, cuts[0])] + [W.cfk_slice(u, cuts[b], cuts[b + 1]) for b in range(n_batches)]
    qs = [W.preaccept_queries(p) for p in parts[1:]]
    xs = [_execute_at_after(p, q) for p, q in zip(parts[1:], qs)]
    ko = u["key_off"].astype(np.int64)
    rng = np.random.default_rng(0xC0FE)
    rqs = []
    for b, q in enumerate(qs):
        codes = np.unique(u["key"][:ko[cuts[b + 1]]])                  # the store's keys after batch b
        j0 = rng.integers(0, len(codes) - SPAN, size=N_RANGE)
        rs = np.concatenate([codes[j0] - np.uint64(1), [np.uint64(0)]])
        re_ = np.concatenate([codes[j0 + SPAN - 1], [codes[-1]]])       # (s, e]: exactly SPAN keys; the last one: every key
        assert codes[0] > 0
        pick = np.linspace(0, len(q["msb"]) - 1, N_RANGE + 1).astype(np.int64)
        kind = np.full(N_RANGE + 1, 3, np.uint64)                       # SyncPoint
        kind[-1] = 4                                                    # ExclusiveSyncPoint
        lsb = (q["lsb"][pick] & np.uint64(0xFFFFFFFFFFFF0000)) | (kind << np.uint64(1)) | np.uint64(1)
        rqs.append(dict(msb=q["msb"][pick], lsb=lsb, node=np.full(N_RANGE + 1, FOREIGN_NODE, np.int32), rng_start=rs, rng_end=re_))
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
    for q, (xm, xl, xn), r in zip(qs, xs, rqs):
        nk, nr = len(q["msb"]), N_RANGE + 1
        cat = lambda a, b, dt: np.concatenate([np.asarray(a, dt), np.asarray(b, dt)])  # noqa: E731
        koff = cat(q["part_off"], np.full(nr, q["part_off"][-1]), np.uint32)
        roff = cat(np.zeros(nk + 1), np.arange(1, nr + 1), np.uint32)
        queries.append(L.CfkMixedQueries(
            nk + nr, L.ACC_MEM_DEVICE, len(q["part_start"]), nr,
            L.TsCols(up(cat(q["msb"], r["msb"], np.uint64)), up(cat(q["lsb"], r["lsb"], np.uint64)), up(cat(q["node"], r["node"], np.int32))),
            L.TsCols(up(cat(xm, r["msb"], np.uint64)), up(cat(xl, r["lsb"], np.uint64)), up(cat(xn, r["node"], np.int32))),
            up(koff), up(q["part_start"].astype(np.uint64)), up(roff), up(r["rng_start"].astype(np.uint64)),
            up(r["rng_end"].astype(np.uint64)), 1, 0))
    torch.cuda.synchronize()
    variants = [f"lane_{n}" for n in LANES] + ["lane_none", "snapshot"]
    lane_of = dict({f"lane_{n}": n for n in LANES}, lane_none=L.ACC_CFQ_LANE_NONE)
    rows = []
    with Context(local) as c:
        lib = c._lib
        h = C.c_void_p()
        c.check(lib.acc_cfk_create(c.handle, C.byref(h)))
        try:
            kv = L.KeydepsView()

            def digest():
                hs = hashlib.blake2b(digest_size=8)
                nq = int(kv.n_txn)
                for ptr, n, dt in ((kv.arena_off, nq + 1, np.uint64), (kv.kd_off, nq + 1, np.uint64), (kv.u_off, nq + 1, np.uint64),
                                   (kv.arena, kv.total_arena, np.int32), (kv.key_idx, kv.total_keys, np.uint32),
                                   (kv.dep_txn, kv.total_deps, np.uint32), (kv.kd_key, kv.total_keys, np.uint64)):
                    hs.update(device_array(c, ptr, int(n), dt).tobytes())
                return hs.hexdigest()

            def last_rows(view, cnt):
                """the last cnt rows of a KeyDeps view, offsets rebased"""
                first = int(view.n_txn) - cnt
                out = []
                for off_ptr, cols in ((view.arena_off, ((view.arena, np.int32),)), (view.kd_off, ((view.key_idx, np.uint32), (view.kd_key, np.uint64))),
                                      (view.u_off, ((view.dep_txn, np.uint32),))):
                    off = device_array(c, off_ptr + 8 * first, cnt + 1, np.uint64)
                    out.append(off - off[0])
                    out += [device_array(c, ptr + int(off[0]) * np.dtype(dt).itemsize, int(off[-1] - off[0]), dt) for ptr, dt in cols]
                return out

            c.check(lib.acc_cfk_apply_deps(c.handle, h, C.byref(upds[0])))
            c.check(lib.acc_cfk_keydeps_mixed(c.handle, h, C.byref(queries[0]), C.byref(kv)))   # warm the query's buffers
            torch.cuda.synchronize()
            for b, (ui, qi, r) in enumerate(zip(upds[1:], queries, rqs)):
                c.check(lib.acc_cfk_apply_deps(c.handle, h, C.byref(ui)))
                torch.cuda.synchronize()
                # the snapshot route's input: the store's view + the range txns appended (PREACCEPTED, no keys)
                v = L.BatchIn()
                c.check(lib.acc_cfk_view(c.handle, h, C.byref(v)))
                n, P = int(v.n_txn), int(v.n_pairs)
                g = lambda ptr, cnt, dt: device_array(c, ptr, cnt, dt)  # noqa: E731
                nr = N_RANGE + 1
                cat = lambda a, b2, dt: up(np.concatenate([np.asarray(a, dt), np.asarray(b2, dt)]))  # noqa: E731
                mark = len(keep)
                snap = L.RangeBatchIn(
                    n + nr, L.ACC_MEM_DEVICE, P, nr,
                    L.TsCols(cat(g(v.txn_id.msb, n, np.uint64), r["msb"], np.uint64), cat(g(v.txn_id.lsb, n, np.uint64), r["lsb"], np.uint64),
                             cat(g(v.txn_id.node, n, np.int32), r["node"], np.int32)),
                    L.TsCols(cat(g(v.execute_at.msb, n, np.uint64), r["msb"], np.uint64),
                             cat(g(v.execute_at.lsb, n, np.uint64), r["lsb"], np.uint64),
                             cat(g(v.execute_at.node, n, np.int32), r["node"], np.int32)),
                    cat(g(v.status, n, np.uint8), np.full(nr, 2), np.uint8),
                    cat(g(v.key_off, n + 1, np.uint32), np.full(nr, P), np.uint32), up(g(v.key_code, P, np.uint64)),
                    cat(np.zeros(n + 1), np.arange(1, nr + 1), np.uint32), up(r["rng_start"].astype(np.uint64)),
                    up(r["rng_end"].astype(np.uint64)), 1, 0)
                torch.cuda.synchronize()
                times = {k: [] for k in variants}
                hashes, stats, err, same = {}, {}, None, None
                sv = L.KeydepsView()
                for rep in range(reps + 1):                      # round 0 warms every variant's buffers, untimed
                    for k in variants:
                        if k == "snapshot" and err:
                            continue
                        t = time.perf_counter()
                        if k == "snapshot":
                            try:
                                c.check(lib.acc_keydeps_mixed(c.handle, C.byref(snap), C.byref(sv)))
                            except AccordError as e:
                                err = f"{type(e).__name__}: {e}"
                                continue
                        else:
                            qi.lane_seg = lane_of[k]
                            c.check(lib.acc_cfk_keydeps_mixed(c.handle, h, C.byref(qi), C.byref(kv)))
                        torch.cuda.synchronize()
                        if rep:
                            times[k].append((time.perf_counter() - t) * 1e3)
                        elif k != "snapshot":
                            hashes[k] = digest()
                            stats[k] = c.stats()
                            if k == "lane_none":
                                mine = last_rows(kv, nr)
                        else:   # the range txns' rows: both routes index the store's view
                            same = all(np.array_equal(x, y) for x, y in zip(mine, last_rows(sv, nr)))
                assert len(set(hashes.values())) == 1, f"batch {b}: the variants' results differ: {hashes}"
                del keep[mark:]
                st = stats["lane_none"]
                row = dict(store_txns=n, store_pairs=P, queries=int(qi.n_query), pairs=st.get("cfq.pairs", 0),
                           range_pairs=st.get("cfq.range_pairs", 0), hits=st.get("cfq.hits", 0),
                           sorted_hits=st.get("cfq.sorted_hits", 0), deps=int(kv.total_deps), hash=hashes["lane_none"],
                           lane_pairs={k: stats[k].get("cfq.lane_pairs", 0) for k in variants if k.startswith("lane_") and k != "lane_none"},
                           chunks={k: stats[k].get("cfq.chunks", 0) for k in stats},
                           ms={k: [round(x, 3) for x in sorted(v2)] for k, v2 in times.items() if v2})
                row["range_rows_equal_snapshot"] = same
                if err:
                    row["snapshot_error"] = err
                rows.append(row)
        finally:
            lib.acc_cfk_destroy(h)
    med = lambda xs_: sorted(xs_)[len(xs_) // 2]  # noqa: E731
    summary = {k: round(sum(med(r["ms"][k]) for r in rows) / len(rows), 3) for k in variants if all(k in r["ms"] for r in rows)}
    spread = {k: round(max(max(r["ms"][k]) / min(r["ms"][k]) for r in rows), 3) for k in summary}
    return {"workload": f"workload.cfk_update_stream({(n_init + batch * n_batches) // 1000}K txns x 8 {dist} keys over 1M keys): "
                        f"a {n_init // 1000}K-txn device store, then {n_batches} batches of {batch // 1000}K new txns; per batch "
                        f"acc_cfk_apply_deps, then one call for the new txns' key queries + {N_RANGE} range queries of {SPAN} "
                        "consecutive covered keys + one range query over every key (timed, median of "
                        f"{reps} per batch, mean over the batches)",
            "median_ms": summary, "max_over_min_of_repeats": spread, "results_bit_equal": True,
            "range_rows_equal_snapshot": all(r["range_rows_equal_snapshot"] is True for r in rows), "per_batch": rows,
            "setup_gen_s": round(t_gen, 2)}


if __name__ == "__main__":
    dist = sys.argv[1] if len(sys.argv) > 1 else "uniform"
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    print(json.dumps({dist: main(dist, nb, max(reps, 5))}), flush=True)
