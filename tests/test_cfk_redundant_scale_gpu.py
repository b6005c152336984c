"""GPU parity for acc_cfk_redundant_before where test_cfk_redundant_gpu.py does not reach: stores of more keys, entries,
missing ids, update pairs and map intervals than one block or one scan tile holds; the scans reading a store that a
prune has just rewritten; ReplicaStore.mark_shard_redundant inside the replica loop; the order's edges (the signed node,
the msb, flag bits outside the identity); ACC_MEM_DEVICE inputs; two stores interleaved on one context.

Expected values come from the Python model (cfk_redundant_model.py) alternating with the C restatement of the update,
built and checked against their host conditions in cfk_redundant_cases.py. Every comparison is exact array equality."""
import ctypes as C

import numpy as np
import pytest

import cfk_cases as CC
import cfk_redundant_cases as RCS
import cfk_redundant_model as M
import oracle
import recovery_cases as RC
import test_cfk_query_gpu as KQ
import test_cfk_query_mixed_gpu as MX
import test_cfk_recovery_gpu as CR
import test_cfk_redundant_gpu as RG
from accord_amd import workload as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


def run_step(c, s, st, msg, do_apply=None, do_prune=None):
    """one step of a chain on the store, then exactly what test_cfk_redundant_gpu.run_chain asserts after it"""
    if st["op"] == "apply":
        (do_apply or s.apply_deps)(st["upd"])
        assert c.stats()["cfk.deps_trimmed"] == st["trimmed"], msg
    else:
        (do_prune or s.redundant_before)(st["ranges"])
        RG.assert_stats(c, st["counts"], msg)
        RG.assert_map(s, st["map"], msg)
    RG.assert_store(c, s, st["state"], msg)


def sample_queries(ob, idx, execute_at=True):
    """the store members idx with their keys (and their stored executeAts): KQ.member_queries of a subset"""
    idx = np.asarray(idx, np.int64)
    ko = ob.key_off.astype(np.int64)
    cnt = ko[idx + 1] - ko[idx]
    off = np.concatenate([[0], np.cumsum(cnt)])
    src = np.repeat(ko[idx], cnt) + (np.arange(int(off[-1])) - np.repeat(off[:-1], cnt))
    q = dict(msb=ob.txn_msb[idx], lsb=ob.txn_lsb[idx], node=ob.txn_node[idx], key_off=off.astype(np.uint32),
             key_code=ob.key_code[src])
    if execute_at:
        q.update(xmsb=ob.exe_msb[idx], xlsb=ob.exe_lsb[idx], xnode=ob.exe_node[idx])
    return q


def scans(s, state, seed, span, run, msg, n_sample=None):
    """the three scans and the whole-store scan on the store as it stands, against the oracle over `state`.
    span: a range over every key; run: a second range (over a key the prune removed, where it removed one);
    n_sample: query that many members (the first and the last among them) instead of all"""
    ob, mo, mt = CC.snap_as_batch(state)
    want = oracle.keydeps_batch(ob)
    if n_sample is None:
        KQ.assert_result(s.keydeps(KQ.member_queries(ob)), want, f"{msg} keydeps")
    else:
        idx = np.unique(np.linspace(0, ob.n_txn - 1, n_sample).astype(np.int64))
        assert idx[0] == 0 and idx[-1] == ob.n_txn - 1
        KQ.assert_result(s.keydeps(sample_queries(ob, idx)), KQ.rows(want, idx), f"{msg} keydeps of {len(idx)} members")
    KQ.assert_result(s.calculate_partial_deps(), want, f"{msg} whole-store scan")
    top = int(max(ob.txn_lsb.max(), ob.exe_lsb.max()) >> 16)
    items = [(MX.ts(top + 9, (4 << 1) | MX.RANGE, 2), None, [], [span]),
             (MX.ts(top + 11, (4 << 1) | MX.RANGE, 3), None, [], [run])]
    MX.assert_result(s.keydeps_mixed(MX.make_mixed(items), 1), MX.expect_mixed(ob, items, 1), f"{msg} mixed")
    q = CC.recovery_queries(ob, seed, 80)
    hits = 0
    for sa, td, tst in RC.ALL_TESTS:
        o = oracle.map_reduce_full(ob, mo, mt, q, sa, td, tst)
        CR.assert_same(s.map_reduce_full(q, sa, td, tst), o, f"{msg} recovery {(sa, td, tst)}")
        hits += len(o.dep_txn)
    assert hits > 0, msg


# ---------------------------------------------------------------- 1. + 2. past one scan tile, scans straight after a prune

@pytest.mark.parametrize("dist", ["uniform", "zipf"])
def test_multi_tile_chain(ctx, dist):
    """cfk_redundant_cases.scale_chain: 11.8K keys (uniform), 48K entries, 26K missing ids (zipf), 16K-20K update pairs
    and 360 / 600 map intervals: every per-key launch takes several blocks, every scan several tiles. After the first
    and the last prune the scans read the store before any update touches it."""
    from accord_amd.deps import CfkStore
    steps = RCS.scale_chain(dist)
    RCS.scale_conditions(steps, dist)
    scan_at = RCS.scale_scan_steps(steps)
    s = CfkStore(ctx)
    try:
        for i, st in enumerate(steps):
            msg = f"{dist} step {i} {st['op']}"
            run_step(ctx, s, st, msg)
            if i in scan_at:
                keys, before = st["state"]["key"], steps[i - 1]["state"]["key"]
                run = RCS.removed_key_run(before, keys)
                assert run is not None, "the prune removed no key"
                scans(s, st["state"], 11 + i, (int(before.min()) - 1, int(before.max())), run, msg, n_sample=500)
                RG.assert_store(ctx, s, st["state"], f"{msg} after the scans")
    finally:
        s.close()


SMALL = (7, "three")     # a chain of test_cfk_redundant_gpu.py; no state after one of its prunes holds an executeAt tie


def test_scans_directly_after_a_prune(ctx):
    from accord_amd.deps import CfkStore
    seed, variant = SMALL
    steps = RG.chain(seed, variant)
    RG.host_conditions(steps, variant)
    assert all(KQ.no_committed_ties(st["state"]) for st in steps if st["op"] == "prune"), "pick another chain"
    s = CfkStore(ctx)
    try:
        n = 0
        for i, st in enumerate(steps):
            msg = f"seed {seed} {variant} step {i} {st['op']}"
            run_step(ctx, s, st, msg)
            if st["op"] == "prune":
                keys = st["state"]["key"]
                run = RCS.removed_key_run(steps[i - 1]["state"]["key"], keys) or MX.cover(keys, 2, len(keys) - 2, 1)
                scans(s, st["state"], seed + i, (M.KEY_LO, M.KEY_HI), run, msg)
                n += 1
        assert n == M.N_BATCHES - 1
    finally:
        s.close()


# ---------------------------------------------------------------- 3. the replica loop

def test_replica_loop_with_mark_shard_redundant(ctx):
    """propose from MaxConflicts, apply, the new txns' KeyDeps in place, prune, BeginRecovery: batch after batch"""
    from accord_amd import _lib as L
    from accord_amd.deps import ReplicaStore
    case = RCS.replica_case()
    RCS.replica_conditions(case)
    u, cuts = case["u"], case["cuts"]
    ident = 0xFFFFFFFFFFFF001E
    rs = ReplicaStore(ctx)
    try:
        rs.preaccept_batch(case["init"], scan=False)
        edges = hits = 0
        for b, bt in enumerate(case["batches"]):
            part, a, p = bt["part"], bt["apply"], bt["prune"]
            q = W.preaccept_queries(part)
            assert len(q["msb"]) == RCS.REPLICA["batch"]
            r = rs.preaccept_batch(part, q, scan="new")
            # a prune does not touch MaxConflicts: the proposals are those over every earlier update
            om = oracle.max_conflicts(W.conflicts_updates(W.cfk_slice(u, 0, cuts[b])), q)
            for k in ("msb", "lsb", "node", "fast"):
                np.testing.assert_array_equal(r["propose"][k], om[k], err_msg=f"batch {b} propose {k}")
            assert ctx.stats()["cfk.deps_trimmed"] == a["trimmed"], f"batch {b}"
            ob = CC.snap_as_batch(a["state"])[0]
            index = {(int(m), int(l) & ident, int(nd)): t for t, (m, l, nd) in enumerate(zip(ob.txn_msb, ob.txn_lsb, ob.txn_node))}
            new = [index[(int(m), int(l) & ident, int(nd))] for m, l, nd in zip(q["msb"], q["lsb"], q["node"])]
            want = KQ.rows(oracle.keydeps_batch(ob, queries=new), new)
            KQ.assert_result(r["keydeps_new"], want, f"batch {b} keydeps_new")
            edges += len(want["dep_txn"])
            RG.assert_store(ctx, rs.cfk, a["state"], f"batch {b} applied")
            rs.mark_shard_redundant(p["ranges"])
            RG.assert_stats(ctx, p["counts"], f"batch {b} prune")
            RG.assert_map(rs.cfk, p["map"], f"batch {b} prune")
            RG.assert_store(ctx, rs.cfk, p["state"], f"batch {b} pruned")
            ob, mo, mt = CC.snap_as_batch(p["state"])
            rq = sample_queries(ob, np.unique(np.linspace(0, ob.n_txn - 1, 60).astype(np.int64)), execute_at=False)
            g = rs.begin_recovery(rq)
            for name, scan in rs._RECOVERY_NAMES.items():
                sa, td, tst, after = L.RECOVERY_SCANS[scan]
                o = oracle.map_reduce_full(ob, mo, mt, rq, sa, td, tst, exec_after=after)
                if name.startswith("has_"):
                    np.testing.assert_array_equal(g[name], np.diff(np.asarray(o.u_off).astype(np.int64)) > 0,
                                                  err_msg=f"batch {b} {name}")
                else:
                    CR.assert_same(g[name], o, f"batch {b} {name}")
                hits += len(o.dep_txn)
        assert edges and hits
    finally:
        rs.close()


# ---------------------------------------------------------------- 4. the order's edges

def test_order_edges(ctx):
    """cfk_redundant_cases.order_edges, worked by hand there: bounds equal to ids that differ in the signed node alone,
    in the msb alone, and in a flag bit the order does not read"""
    from accord_amd.deps import CfkStore
    s = CfkStore(ctx)
    try:
        m, state = M.BoundMap(1), CC.empty_snapshot()
        for i, (op, arg, want, n) in enumerate(RCS.order_edges()):
            msg = f"step {i} {op}"
            if op == "apply":
                state = RG.apply(ctx, s, state, m, arg, msg)
                assert ctx.stats()["cfk.deps_trimmed"] == n, msg
            else:
                view = s.view()
                ptrs = (view.txn_id.msb, view.key_off, view.key_code)
                state = RG.prune(ctx, s, state, m, arg, msg)
                RG.assert_stats(ctx, n, msg)
                if n["keys_advanced"] == 0:
                    view = s.view()
                    assert (view.txn_id.msb, view.key_off, view.key_code) == ptrs, "a tie with the stored bound rewrote the view"
            assert RCS.edge_names(state) == want, msg
            assert RCS.edge_names(s.state()) == want, msg
    finally:
        s.close()


# ---------------------------------------------------------------- 5. inputs in device memory

class DeviceInputs:
    """acc_cfk_redundant_before / acc_cfk_apply_deps through the C ABI with mem = ACC_MEM_DEVICE: the columns uploaded
    with torch; after the call every uploaded tensor must hold what was uploaded"""

    def __init__(self, c, s):
        self.c, self.s = c, s

    def call(self, cols, make, fn, msg):
        import torch
        dev = torch.device("cuda", self.c.device)
        t = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
        torch.cuda.synchronize()
        p = lambda k: t[k].data_ptr()  # noqa: E731
        self.c.check(fn(self.c.handle, self.s._h, C.byref(make(p))))
        self.c.sync()
        for k, v in cols.items():
            np.testing.assert_array_equal(t[k].cpu().numpy(), v, err_msg=f"{msg}: the call wrote into the caller's {k}")

    def prune(self, ranges, end_inclusive=1):
        from accord_amd import _lib as L
        cols = dict(rs=np.ascontiguousarray(ranges["rng_start"], dtype=np.uint64), re=np.ascontiguousarray(ranges["rng_end"], dtype=np.uint64),
                    bm=np.ascontiguousarray(ranges["msb"], dtype=np.uint64), bl=np.ascontiguousarray(ranges["lsb"], dtype=np.uint64),
                    bn=np.ascontiguousarray(ranges["node"], dtype=np.int32))
        make = lambda p: L.CfkRedundantIn(L.ACC_MEM_DEVICE, len(cols["rs"]), int(end_inclusive), p("rs"), p("re"),  # noqa: E731
                                          L.TsCols(p("bm"), p("bl"), p("bn")))
        self.call(cols, make, self.c._lib.acc_cfk_redundant_before, "redundant_before")

    def apply(self, upd):
        from accord_amd import _lib as L
        from accord_amd.deps import _cfk_updates_host
        b = _cfk_updates_host(upd)
        make = lambda p: L.CfkUpdates(L.ACC_MEM_DEVICE, len(b["msb"]), len(b["key"]), len(b["dmsb"]),  # noqa: E731
                                      L.TsCols(p("msb"), p("lsb"), p("node")), L.TsCols(p("xmsb"), p("xlsb"), p("xnode")),
                                      p("status"), p("flags"), p("key_off"), p("key"), p("dep_off"),
                                      L.TsCols(p("dmsb"), p("dlsb"), p("dnode")))
        self.call(b, make, self.c._lib.acc_cfk_apply_deps, "apply_deps")


def test_device_inputs_handmade(ctx):
    """the hand-made case with the map first, so its one batch arrives under bounds (deps trimmed), then a prune of
    the filled store and one more batch: a store fed device inputs beside one fed host inputs, both against the model"""
    from accord_amd.deps import CfkStore
    upd, ranges, _, _ = M.handmade()
    script = [("prune", ranges), ("apply", upd), ("prune", M.ranges_of([(M.KEY_LO, M.KEY_HI, M.ts(14))])),
              ("apply", M.updates_of([(M.ts(24), M.ACC, [100, 200, 300, 400], [M.ts(4), M.ts(12), M.ts(20)])]))]
    d, h = CfkStore(ctx), CfkStore(ctx)
    try:
        dev = DeviceInputs(ctx, d)
        m, state, trimmed = M.BoundMap(1), CC.empty_snapshot(), []
        for i, (op, arg) in enumerate(script):
            msg = f"step {i} {op}"
            step, state = (RCS.apply_step if op == "apply" else RCS.prune_step)(state, m, arg)
            trimmed.append(step.get("trimmed", 0))
            if i == 0:      # an empty store records the map: there is no state to read yet
                dev.prune(arg)
                RG.assert_map(d, step["map"], msg)
                h.redundant_before(arg)
                continue
            run_step(ctx, d, step, f"{msg} device inputs", dev.apply, dev.prune)
            run_step(ctx, h, step, f"{msg} host inputs")
        assert trimmed[1] > 0 and trimmed[3] > 0
    finally:
        d.close()
        h.close()


def test_device_inputs_chain(ctx):
    from accord_amd.deps import CfkStore
    steps = RG.chain(5, "three")
    RG.host_conditions(steps, "three")
    d, h = CfkStore(ctx), CfkStore(ctx)
    try:
        dev = DeviceInputs(ctx, d)
        for i, st in enumerate(steps):
            run_step(ctx, d, st, f"step {i} {st['op']} device inputs", dev.apply, dev.prune)
            run_step(ctx, h, st, f"step {i} {st['op']} host inputs")
    finally:
        d.close()
        h.close()


# ---------------------------------------------------------------- 6. two stores on one context

def test_two_stores_interleaved(ctx):
    """A: a chained case; B: the much smaller cfk_redundant_cases.small_script. Every call's results trade places
    with the calling store's arrays in the context's named buffers, so each store keeps receiving arrays the other
    one left: after every step both stores are compared with their models. A is closed first, B goes on."""
    from accord_amd.deps import CfkStore
    a_steps = RG.chain(7, "single")
    b_ops = RCS.small_script()
    order = []
    ia = ib = 0
    while ia < len(a_steps):                       # apply A, apply B, prune A, apply B, prune B, apply A, ...
        for who in "ABABBA":
            if who == "A" and ia < len(a_steps):
                order.append(("A", ia))
                ia += 1
            elif who == "B" and ib < len(b_ops) - 2:
                order.append(("B", ib))
                ib += 1
    assert ib == len(b_ops) - 2 and [b_ops[j][0] for j in (ib, ib + 1)] == ["apply", "prune"]
    A, B = CfkStore(ctx), CfkStore(ctx)
    try:
        mb, b_state, a_state = M.BoundMap(1), None, None

        def b_step(j, msg):
            op, arg = b_ops[j]
            prev = CC.empty_snapshot() if b_state is None else b_state
            return (RG.apply if op == "apply" else RG.prune)(ctx, B, prev, mb, arg, msg)

        for n, (who, j) in enumerate(order):
            msg = f"call {n}: {who} step {j}"
            if who == "A":
                run_step(ctx, A, a_steps[j], msg)
                a_state = a_steps[j]["state"]
            else:
                b_state = b_step(j, msg)
            if a_state is not None:
                RG.assert_store(ctx, A, a_state, f"{msg}: store A")
            if b_state is not None:
                RG.assert_store(ctx, B, b_state, f"{msg}: store B")
        A.close()
        for j in (ib, ib + 1):
            b_state = b_step(j, f"B step {j} after A closed")
        assert len(b_state["key"]) > 0
    finally:
        A.close()
        B.close()
