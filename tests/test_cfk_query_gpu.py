"""GPU parity for acc_cfk_keydeps (CfkStore.keydeps): PreAccept.calculatePartialDeps' key half for new txns against the
resident CommandsForKey store (messages/PreAccept.java:107-138, 245-265 -> local/CommandsForKey.java:614-650), scanned in
place. Expected values are the C restatement's KeyDeps (oracle.keydeps_batch) over the host restatement of the store's
txn-major view (cfk_cases.snap_as_batch of the chained oracle.cfk_apply state), whose txn indices are the store-view
indices the device result uses.

The tie rule: a (query, key) pair that sees two or more committed entries executing exactly at the query's executeAt
fails the call (the reference's bisection is not determined there), so the seeded cases below are asserted free of such
states (no_committed_ties) before the device is asked; the seeds were chosen for that on the host restatement alone."""
import numpy as np
import pytest

import cfk_cases as CC
import oracle
from accord_amd import workload as W

pytestmark = pytest.mark.gpu

FIELDS = ("arena_off", "kd_off", "u_off", "arena", "key_idx", "dep_txn")
WRITE = 1 << 1
SMALL_CAP = 11      # the one-wave build tier's hit cap in the contexts that exercise the cap boundary
CHUNK = 256         # the scan's work chunk (csrc/cfkquery.hip): prefixes around it and its multiples change the chunk count


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_cap1():
    from accord_amd.deps import Context
    c = Context(0, cfq_wave_cap=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_small_cap():
    from accord_amd.deps import Context
    c = Context(0, cfq_wave_cap=SMALL_CAP)
    yield c
    c.close()


def ts(hlc, flags=WRITE, node=1):
    return tuple(int(x) for x in W.encode_ts(1, hlc, flags, node))


def make_queries(items):
    """items: [(txn_id, execute_at or None, [key codes])] -> the CfkStore.keydeps queries dict"""
    qm, ql, qn, xm, xl, xn, ko, kc = [], [], [], [], [], [], [0], []
    for tid, ex, keys in items:
        ex = tid if ex is None else ex
        qm.append(tid[0]); ql.append(tid[1]); qn.append(tid[2])
        xm.append(ex[0]); xl.append(ex[1]); xn.append(ex[2])
        kc.extend(keys)
        ko.append(len(kc))
    return dict(msb=np.array(qm, np.uint64), lsb=np.array(ql, np.uint64), node=np.array(qn, np.int32),
                xmsb=np.array(xm, np.uint64), xlsb=np.array(xl, np.uint64), xnode=np.array(xn, np.int32),
                key_off=np.array(ko, np.uint32), key_code=np.array(kc, np.uint64))


def member_queries(ob):
    """every store member with its stored executeAt and its keys"""
    return dict(msb=ob.txn_msb, lsb=ob.txn_lsb, node=ob.txn_node, xmsb=ob.exe_msb, xlsb=ob.exe_lsb, xnode=ob.exe_node,
                key_off=ob.key_off, key_code=ob.key_code)


def with_query(ob, tid, ex, keys):
    """ob with the query appended as a PREACCEPTED entry (index ob.n_txn; the store indices stay as they are)"""
    ex = tid if ex is None else ex
    ap = lambda a, v, dt: np.append(np.asarray(a, dt), dt(v))  # noqa: E731
    return W.Batch(ap(ob.txn_msb, tid[0], np.uint64), ap(ob.txn_lsb, tid[1], np.uint64), ap(ob.txn_node, tid[2], np.int32),
                   ap(ob.exe_msb, ex[0], np.uint64), ap(ob.exe_lsb, ex[1], np.uint64), ap(ob.exe_node, ex[2], np.int32),
                   ap(ob.status, CC.PRE, np.uint8), ap(ob.key_off, int(ob.key_off[-1]) + len(keys), np.uint32),
                   np.concatenate([np.asarray(ob.key_code, np.uint64), np.array(keys, np.uint64)]))


def rows(res, idx):
    """the rows idx of a per-txn KeyDeps result as one result over len(idx) queries (the six FIELDS)"""
    out = {f: [] for f in ("arena", "key_idx", "dep_txn")}
    offs = {f: [0] for f in ("arena_off", "kd_off", "u_off")}
    for t in idx:
        k, d, a = res.txn(int(t))
        out["arena"].append(a); out["key_idx"].append(k); out["dep_txn"].append(d)
        offs["arena_off"].append(offs["arena_off"][-1] + len(a))
        offs["kd_off"].append(offs["kd_off"][-1] + len(k))
        offs["u_off"].append(offs["u_off"][-1] + len(d))
    r = {f: np.array(v, np.uint64) for f, v in offs.items()}
    for f, dt in (("arena", np.int32), ("key_idx", np.uint32), ("dep_txn", np.uint32)):
        r[f] = np.concatenate(out[f]).astype(dt) if out[f] else np.zeros(0, dt)
    return r


def expect_foreign(ob, items):
    """one query at a time: the oracle over ob + the query as a PREACCEPTED entry, queried alone"""
    parts = []
    for tid, ex, keys in items:
        o = oracle.keydeps_batch(with_query(ob, tid, ex, keys), queries=[ob.n_txn])
        parts.append(o.txn(ob.n_txn))
    class R:  # noqa: E306
        def txn(self, t):
            return parts[t]
    return rows(R(), range(len(items)))


def assert_result(g, want, msg):
    for f in FIELDS:
        np.testing.assert_array_equal(np.asarray(getattr(g, f)), np.asarray(want[f] if isinstance(want, dict) else getattr(want, f)),
                                      err_msg=f"{msg}: {f}")


def no_committed_ties(state):
    """no key holds two committed-class entries with one executeAt (the state the tie rule rejects)"""
    off = state["ent_off"].astype(np.int64)
    for k in range(len(state["key"])):
        seen = set()
        for e in range(off[k], off[k + 1]):
            if CC.COMMITTED <= int(state["status"][e]) <= CC.APPLIED:
                x = (int(state["xmsb"][e]), int(state["xlsb"][e]) & 0xFFFFFFFFFFFF001E, int(state["xnode"][e]))
                if x in seen:
                    return False
                seen.add(x)
    return True


# ---------------------------------------------------------------- 1. hand-worked

def test_handmade(ctx):
    from accord_amd.deps import CfkStore
    upd, _ = CC.handmade()
    first3, rest = CC.split_updates(upd, 3)
    s = CfkStore(ctx)
    try:
        s.apply_deps(first3)      # [A COMMITTED, B PREACCEPTED, C ACCEPTED]: nothing below M = A, A itself stays
        g = s.keydeps(make_queries([(ts(16), None, [500])]))
        np.testing.assert_array_equal(g.arena_off, [0, 4])
        np.testing.assert_array_equal(g.arena, [4, 0, 1, 2])
        np.testing.assert_array_equal(g.kd_off, [0, 1])
        np.testing.assert_array_equal(g.key_idx, [0])
        np.testing.assert_array_equal(g.u_off, [0, 3])
        np.testing.assert_array_equal(g.dep_txn, [0, 1, 2])
        s.apply_deps(rest)        # [A COMMITTED, B COMMITTED, C ACCEPTED]
        # hlc 16 on 500: M = B, A pruned -> [B, C]; hlc 6 on 500: prefix [A], M = A stays -> [A]; key 501: no CFK
        g = s.keydeps(make_queries([(ts(16), None, [500]), (ts(6), None, [500]), (ts(16), None, [501])]))
        np.testing.assert_array_equal(g.arena_off, [0, 3, 5, 5])
        np.testing.assert_array_equal(g.arena, [3, 0, 1, 2, 0])
        np.testing.assert_array_equal(g.kd_off, [0, 1, 2, 2])
        np.testing.assert_array_equal(g.key_idx, [0, 0])
        np.testing.assert_array_equal(g.u_off, [0, 2, 3, 3])
        np.testing.assert_array_equal(g.dep_txn, [1, 2, 0])
        np.testing.assert_array_equal(g.kd_key, [500, 500])
    finally:
        s.close()


# ---------------------------------------------------------------- 2. + 3. seeded stores, member and foreign queries

# cfk_case bumps executeAts within a narrow range, so most seeds commit two txns of one key at one executeAt, which the
# reference never does (executeAt is unique per command) and the tie rule rejects: of seeds 1..59 these three are the
# ones whose final state no_committed_ties accepts (found on the host restatement alone)
SEEDS = (22, 46, 54)


def foreign_items(ob, seed):
    rng = np.random.default_rng(seed ^ 0xF0)
    codes = np.unique(ob.key_code)
    items = []
    for i in range(20):
        hlc = 2 * int(rng.integers(0, 4 * ob.n_txn + 8)) + 1      # odd: no store TxnId or executeAt (all even)
        tid = ts(hlc, int(rng.choice(CC.KINDS)) << 1, 1 + int(rng.integers(0, 4)))
        ex = ts(hlc + 2 * int(rng.integers(1, 40)), 0, 1 + int(rng.integers(0, 4))) if i % 2 else None
        keys = sorted({7} | set(int(x) for x in rng.choice(codes, size=2, replace=False)))   # 7: no CFK
        items.append((tid, ex, keys))
    return items


@pytest.mark.parametrize("cap1", [False, True], ids=["default_cap", "cap1"])
@pytest.mark.parametrize("seed", SEEDS)
def test_member_and_foreign_queries(ctx, ctx_cap1, seed, cap1):
    from accord_amd.deps import CfkStore
    c = ctx_cap1 if cap1 else ctx
    upd = CC.cfk_case(seed, n_txn=200, n_keys=12, keys_per=3)
    n = len(upd["msb"])
    a, rest = CC.split_updates(upd, int(n * 0.4))
    b, d = CC.split_updates(rest, int(n * 0.7) - int(n * 0.4))
    s = CfkStore(c)
    try:
        o_state = CC.empty_snapshot()
        for step, part in enumerate((a, b, d)):
            s.apply_deps(part)
            o_state = oracle.cfk_apply(o_state, part)
            assert no_committed_ties(o_state), "seed holds an executeAt tie: pick another"
            ob = CC.snap_as_batch(o_state)[0]
            g = s.keydeps(member_queries(ob))
            assert_result(g, oracle.keydeps_batch(ob), f"seed {seed} slice {step} members")
            np.testing.assert_array_equal(g.kd_key, ob.key_code[(np.repeat(ob.key_off[:-1].astype(np.int64), np.diff(g.kd_off.astype(np.int64)))
                                                                  + g.key_idx.astype(np.int64))])
            items = foreign_items(ob, seed + step)
            g = s.keydeps(make_queries(items))
            assert_result(g, expect_foreign(ob, items), f"seed {seed} slice {step} foreign")
    finally:
        s.close()


# ---------------------------------------------------------------- 4. segment widths

def width_stream(L, tail):
    """L Writes at hlc 4, 8, .. on key 900, the first L - tail first seen COMMITTED (executeAt = TxnId), the last `tail`
    ACCEPTED; one more ACCEPTED Write above them on key 901 alone"""
    cols = {k: [] for k in ("msb", "lsb", "node", "xmsb", "xlsb", "xnode", "status", "flags")}
    for i in range(L + 1):
        m, l, nd = ts(4 * i + 4)
        st = CC.COMMITTED if i < L - tail else CC.ACC
        for k, v in zip(cols, (m, l, nd, m, l, nd, st, 0)):
            cols[k].append(v)
    upd = {k: np.array(v, dt) for (k, v), dt in zip(cols.items(), (np.uint64, np.uint64, np.int32, np.uint64, np.uint64,
                                                                  np.int32, np.uint8, np.uint8))}
    upd.update(key_off=np.arange(L + 2, dtype=np.uint32), key=np.array([900] * L + [901], np.uint64),
               dep_off=np.zeros(L + 2, np.uint32), dmsb=np.zeros(0, np.uint64), dlsb=np.zeros(0, np.uint64),
               dnode=np.zeros(0, np.int32))
    return upd


# 63 / 64 / 65 / 128 / 129: the lanes of a wave; CHUNK - 1 .. CHUNK + 1, 2 CHUNK + 1: one, two and three chunks per pair
# (the fold of the chunks' M); tail 300 of 513: M lies two chunks below the end and 301 hits sort in several LDS rounds
WIDTHS = [(63, 10), (64, 10), (65, 10), (128, 10), (129, 10), (CHUNK - 1, 10), (CHUNK, 10), (CHUNK + 1, 10),
          (2 * CHUNK + 1, 10), (2 * CHUNK + 1, 300)]


def width_items(L, tail):
    """the queries of test_segment_widths over width_stream(L, tail), and how many of them come before the three that
    read key 901 as well"""
    top = 4 * (L + 1) + 4
    inside = sorted({1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, L - tail - 1, L - tail, L - tail + 1, L - 1} & set(range(1, L)))
    items = [(ts(top + 5), None, [900])]                                   # above: the whole segment
    items += [(ts(4 * j + 4 + 1), None, [900]) for j in inside]            # inside: prefix of j + 1 entries
    items += [(ts(4 * j + 4, 0 << 1), None, [900]) for j in inside[:3]]    # a Read on a member's hlc (another TxnId)
    items += [(ts(1), None, [900])]                                        # below: nothing
    both = len(items)
    items += [(ts(top + 5), None, [900, 901]), (ts(top + 7), None, [901]), (ts(top + 9), None, [899, 900, 901, 902])]
    return items, both


@pytest.mark.parametrize("L,tail", WIDTHS)
def test_segment_widths(ctx, ctx_small_cap, L, tail):
    from accord_amd.deps import CfkStore
    upd = width_stream(L, tail)
    ob = CC.snap_as_batch(oracle.cfk_apply(CC.empty_snapshot(), upd))[0]
    items, both = width_items(L, tail)
    want = expect_foreign(ob, items)
    if tail == SMALL_CAP - 1:
        # above on 900: the last committed + the tail = SMALL_CAP hits (one-wave tier at the cap);
        # on 900 + 901: SMALL_CAP + 1 (the sorting tier)
        assert int(want["u_off"][1]) == SMALL_CAP
        assert int(want["u_off"][both + 1] - want["u_off"][both]) == SMALL_CAP + 1
    for c, name in ((ctx, "default cap"), (ctx_small_cap, "small cap")):
        s = CfkStore(c)
        try:
            s.apply_deps(upd)
            assert_result(s.keydeps(make_queries(items)), want, f"L {L} tail {tail} {name}")
            assert_result(s.keydeps(member_queries(ob)), oracle.keydeps_batch(ob), f"L {L} tail {tail} {name} members")
        finally:
            s.close()


# ---------------------------------------------------------------- 5. steady-state chain

@pytest.mark.parametrize("dist", ["uniform", "zipf"])
def test_steady_state_new_txns(ctx, dist):
    from accord_amd.deps import ReplicaStore
    u = W.cfk_update_stream(6_000, 4, 800, dist=dist, window=600)
    nb = 4
    cuts = W.cfk_stream_cuts(u, 3_000, 500, nb)
    rs = ReplicaStore(ctx)
    try:
        init = W.cfk_slice(u, 0, cuts[0])
        rs.preaccept_batch(init, scan=False)
        o_state = oracle.cfk_apply(CC.empty_snapshot(), init)
        edges = 0
        for b in range(nb):
            part = W.cfk_slice(u, cuts[b], cuts[b + 1])
            q = W.preaccept_queries(part)
            assert len(q["msb"]) == 500
            r = rs.preaccept_batch(part, q, scan="new")
            assert "keydeps" not in r
            o_state = oracle.cfk_apply(o_state, part)
            ob = CC.snap_as_batch(o_state)[0]
            index = {(int(m), int(l) & 0xFFFFFFFFFFFF001E, int(nd)): t
                     for t, (m, l, nd) in enumerate(zip(ob.txn_msb, ob.txn_lsb, ob.txn_node))}
            new = [index[(int(m), int(l) & 0xFFFFFFFFFFFF001E, int(nd))] for m, l, nd in zip(q["msb"], q["lsb"], q["node"])]
            want = rows(oracle.keydeps_batch(ob, queries=new), new)
            assert_result(r["keydeps_new"], want, f"{dist} batch {b}")
            edges += len(want["dep_txn"])
            # the query neither modified the store nor wrote into the buffers the next update adopts
            g_state = rs.cfk.state()
            for k in o_state:
                np.testing.assert_array_equal(np.asarray(g_state[k]), np.asarray(o_state[k]), err_msg=f"{dist} batch {b} state {k}")
        assert edges
    finally:
        rs.close()


# ---------------------------------------------------------------- 6. errors and edges

def test_errors_and_edges(ctx):
    from accord_amd.deps import CfkStore, IllegalArgumentException, IllegalStateException
    upd, _ = CC.handmade()
    s = CfkStore(ctx)
    empty = CfkStore(ctx)
    status_only = CfkStore(ctx)
    try:
        s.apply_deps(upd)
        good = make_queries([(ts(16), None, [500])])

        def check_good():
            g = s.keydeps(good)
            np.testing.assert_array_equal(g.arena, [3, 0, 1])
            np.testing.assert_array_equal(g.dep_txn, [1, 2])

        check_good()
        with pytest.raises(IllegalArgumentException):
            s.keydeps(make_queries([(ts(16), None, [500]), (ts(18), None, [501, 500])]))      # unsorted keys
        with pytest.raises(IllegalArgumentException):
            s.keydeps(make_queries([(ts(16), None, [500, 500])]))                              # duplicate keys
        with pytest.raises(IllegalArgumentException):
            s.keydeps(make_queries([(ts(16, WRITE | 1), None, [500])]))                        # range domain
        bad = dict(good, key_off=np.array([1, 1], np.uint32))
        with pytest.raises(IllegalArgumentException):
            s.keydeps(bad)                                                                     # offsets do not start at 0
        bad = make_queries([(ts(16), None, [500]), (ts(18), None, [500])])
        bad["key_off"] = np.array([0, 2, 1], np.uint32)
        with pytest.raises(IllegalArgumentException):
            s.keydeps(bad)                                                                     # offsets decrease
        check_good()

        b = W.keydeps_batch(50, 2, 10, 7, "uniform")
        status_only.update(b)
        with pytest.raises(IllegalStateException):
            status_only.keydeps(good)

        for st in (empty, s):
            g = st.keydeps(make_queries([]))                                                   # n_query = 0
            for f in ("arena_off", "kd_off", "u_off"):
                np.testing.assert_array_equal(getattr(g, f), [0])
            assert len(g.arena) == len(g.key_idx) == len(g.dep_txn) == 0
        g = empty.keydeps(make_queries([(ts(16), None, [500]), (ts(18), None, [])]))           # empty store
        for f in ("arena_off", "kd_off", "u_off"):
            np.testing.assert_array_equal(getattr(g, f), [0, 0, 0])
        g = s.keydeps(make_queries([(ts(16), None, []), (ts(16), None, [500]), (ts(18), None, [])]))   # queries without keys
        np.testing.assert_array_equal(g.arena_off, [0, 0, 3, 3])
        np.testing.assert_array_equal(g.arena, [3, 0, 1])
        np.testing.assert_array_equal(g.u_off, [0, 0, 2, 2])
        np.testing.assert_array_equal(g.dep_txn, [1, 2])
        g = s.keydeps(dict(msb=good["msb"], lsb=good["lsb"], node=good["node"], key_off=good["key_off"],
                           key_code=good["key_code"]))                                         # no executeAt columns
        np.testing.assert_array_equal(g.dep_txn, [1, 2])
        check_good()
    finally:
        s.close()
        empty.close()
        status_only.close()


def test_tie_rule(ctx):
    """two committed entries of one key executing at one timestamp: a query whose executeAt is that timestamp fails with
    IllegalStateException (the reference's bisection could land on either); any other query is answered"""
    from accord_amd.deps import CfkStore, IllegalStateException
    x = ts(20, 0, 1)
    cols = {k: [] for k in ("msb", "lsb", "node", "xmsb", "xlsb", "xnode", "status", "flags")}
    for h in (4, 8):
        m, l, nd = ts(h)
        for k, v in zip(cols, (m, l, nd, x[0], x[1], x[2], CC.COMMITTED, 0)):
            cols[k].append(v)
    upd = {k: np.array(v, dt) for (k, v), dt in zip(cols.items(), (np.uint64, np.uint64, np.int32, np.uint64, np.uint64,
                                                                  np.int32, np.uint8, np.uint8))}
    upd.update(key_off=np.array([0, 1, 2], np.uint32), key=np.array([500, 500], np.uint64), dep_off=np.zeros(3, np.uint32),
               dmsb=np.zeros(0, np.uint64), dlsb=np.zeros(0, np.uint64), dnode=np.zeros(0, np.int32))
    s = CfkStore(ctx)
    try:
        s.apply_deps(upd)
        with pytest.raises(IllegalStateException):
            s.keydeps(make_queries([(ts(12), x, [500])]))
        g = s.keydeps(make_queries([(ts(12), ts(22, 0, 1), [500])]))      # both execute below S at one M: neither pruned
        np.testing.assert_array_equal(g.dep_txn, [0, 1])
    finally:
        s.close()
