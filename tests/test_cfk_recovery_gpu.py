"""GPU parity for acc_cfk_map_reduce_full (CfkStore.map_reduce_full, ReplicaStore.begin_recovery): BeginRecovery's scans
(messages/BeginRecovery.java:330-380 -> CommandsForKey.mapReduceFull, local/CommandsForKey.java:553-612) answered from the
resident CommandsForKey store's key-major segments and missing[] lists in place.

Expected values come only from the C restatement: oracle.cfk_apply chained -> cfk_cases.snap_as_batch ->
oracle.map_reduce_full, whose txn indices are the store-view indices the device result uses. A range-domain query's
expected row is the oracle's row for the same testTxnId over the store keys its ranges cover, the cover computed here
from the state's keys. Every comparison is exact array equality."""
import functools

import numpy as np
import pytest

import cfk_cases as CC
import oracle
import recovery_cases as RC
import test_cfk_query_gpu as KQ
from accord_amd import _lib as L

pytestmark = pytest.mark.gpu

FIELDS = ("arena_off", "arena", "kd_off", "key_idx", "u_off", "dep_txn")
CHUNK = KQ.CHUNK
WAVES = 4                    # items (waves) per block of a sliced launch
DEFAULT_LIMIT = 1 << 23      # blocks per slice when wave_grid_max is 0
IDENT = 0xFFFFFFFFFFFF001E   # Timestamp.compareTo / equals read these lsb bits
BEFORE, AFTER, ANY = L.ACC_STARTED_BEFORE, L.ACC_STARTED_AFTER, L.ACC_STARTED_ANY
WITH, WITHOUT, ANY_DEPS = L.ACC_DEP_WITH, L.ACC_DEP_WITHOUT, L.ACC_DEP_ANY
ANY_STATUS, IS_PROPOSED, IS_STABLE = L.ACC_STATUS_ANY, L.ACC_STATUS_IS_PROPOSED, L.ACC_STATUS_IS_STABLE
MASK = (1 << 1) | (1 << 4)   # an explicit Kinds mask: Writes and ExclusiveSyncPoints
CASES = [(4, 160, 10), (6, 1500, 40)]


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


def tkey(m, l, n):
    return (int(m), int(l) & IDENT, int(n))


CUTS = (0.3, 0.55, 0.8)      # the three chained batches end here; the rest of the stream is a fourth, final batch


@functools.lru_cache(maxsize=None)
def chain(seed, n_txn, n_keys):
    """the lifecycle in chained batches: [(part, state after it, snap_as_batch(state))], computed once. The first three
    end inside the stream, where txns are still uncommitted and missing[] lists are populated; the fourth completes
    every lifecycle, which leaves every missing[] empty (committing removes a TxnId from all of them)."""
    upd = CC.cfk_case(seed, n_txn=n_txn, n_keys=n_keys)
    n = len(upd["msb"])
    out, state, rest, done = [], CC.empty_snapshot(), upd, 0
    for cut in [int(n * f) for f in CUTS] + [n]:
        part, rest = CC.split_updates(rest, cut - done)
        done = cut
        state = oracle.cfk_apply(state, part)
        out.append((part, state, CC.snap_as_batch(state)))
    return out


def assert_same(g, o, msg, fields=FIELDS):
    for f in fields:
        np.testing.assert_array_equal(np.asarray(getattr(g, f)), np.asarray(getattr(o, f)), err_msg=f"{msg}: {f}")


def make_queries(items):
    """items: [(test_txn_id, [key codes], [(start, end)])] -> the CfkStore.map_reduce_full dict"""
    qm, ql, qn, ko, kc, ro, rs, re_ = [], [], [], [0], [], [0], [], []
    for tid, keys, ranges in items:
        qm.append(tid[0]); ql.append(tid[1]); qn.append(tid[2])
        kc.extend(keys); ko.append(len(kc))
        rs.extend(a for a, _ in ranges); re_.extend(b for _, b in ranges); ro.append(len(rs))
    return dict(msb=np.array(qm, np.uint64), lsb=np.array(ql, np.uint64), node=np.array(qn, np.int32),
                key_off=np.array(ko, np.uint32), key_code=np.array(kc, np.uint64), rng_off=np.array(ro, np.uint32),
                rng_start=np.array(rs, np.uint64), rng_end=np.array(re_, np.uint64))


def covered(codes, ranges, end_inclusive):
    """the store keys the ranges cover, range by range: (s, e] or [s, e)"""
    out = []
    for a, b in ranges:
        out += [int(k) for k in codes if (a < k <= b if end_inclusive else a <= k < b)]
    return out


def as_key_queries(state, items, end_inclusive):
    """every item as the key query the oracle answers: a range item over its covered store keys"""
    codes = [int(k) for k in state["key"]]
    keys = [list(ks) if not rg else covered(codes, rg, end_inclusive) for _, ks, rg in items]
    q = make_queries([(tid, ks, []) for (tid, _, _), ks in zip(items, keys)])
    return {k: q[k] for k in ("msb", "lsb", "node", "key_off", "key_code")}


def expect_kd_key(o, okq):
    """kd_key the device reports: the code of every key with entries"""
    per = np.diff(np.asarray(o.kd_off).astype(np.int64))
    base = np.repeat(okq["key_off"][:-1].astype(np.int64), per)
    return okq["key_code"][base + np.asarray(o.key_idx).astype(np.int64)]


def windows(state, q, sa, td):
    """per (query, key) pair of key-domain queries: the window's length, by CommandsForKey.java:561-575 on the host"""
    off = state["ent_off"].astype(np.int64)
    seg = {int(k): [tkey(state["emsb"][e], state["elsb"][e], state["enode"][e]) for e in range(off[j], off[j + 1])]
           for j, k in enumerate(state["key"])}
    out = []
    for i in range(len(q["msb"])):
        X = tkey(q["msb"][i], q["lsb"][i], q["node"][i])
        for k in q["key_code"][int(q["key_off"][i]):int(q["key_off"][i + 1])]:
            ids = seg.get(int(k), [])
            pos = sum(1 for t in ids if t < X)
            known = pos < len(ids) and ids[pos] == X
            if not known and td == WITH:
                out.append(0)
            else:
                out.append(pos if sa == BEFORE else len(ids) - pos if sa == AFTER else len(ids))
    return np.array(out, np.int64)


def chunks_of(w):
    return -(-w // CHUNK)


# ---------------------------------------------------------------- a. generated lifecycles

# the seed of CC.recovery_queries per case seed, chosen on the host restatement alone so that the 120 queries hit both
# WITH and WITHOUT after each of the three chained batches (the larger case's missing[] lists are few and short)
QUERY_SEEDS = {4: 4, 6: 8}


def missing_queries(state, limit=24):
    """queries the generator rarely draws: X = a TxnId some entry's missing[] names, on that entry's key"""
    off = state["ent_off"].astype(np.int64)
    owner = np.repeat(np.arange(len(state["key"])), np.diff(off))
    mo = state["miss_off"].astype(np.int64)
    items = []
    for e in np.nonzero(np.diff(mo))[0][:limit]:
        j = int(mo[e]) + (int(e) % int(mo[e + 1] - mo[e]))
        items.append(((int(state["mmsb"][j]), int(state["mlsb"][j]), int(state["mnode"][j])), [int(state["key"][owner[e]])], []))
    q = make_queries(items)
    return {k: q[k] for k in ("msb", "lsb", "node", "key_off", "key_code")}


def concat_queries(a, b):
    out = {k: np.concatenate([a[k], b[k]]) for k in ("msb", "lsb", "node", "key_code")}
    out["key_off"] = np.concatenate([a["key_off"], b["key_off"][1:] + a["key_off"][-1]]).astype(np.uint32)
    return out


@pytest.mark.parametrize("seed,n_txn,n_keys", CASES)
def test_generated_lifecycles(ctx, seed, n_txn, n_keys):
    """Three chained batches that end inside the stream (CUTS), each followed by the 120 generated queries (plus up to
    24 that name a TxnId of some missing[]) under every TestStartedAt x TestDep x TestStatus, with the executeAt filter
    and with an explicit Kinds mask; then the rest of the stream, after which every lifecycle is complete and every
    missing[] is empty, under the 27 combinations once more."""
    from accord_amd.deps import CfkStore, cfk_map_reduce_full
    st = CfkStore(ctx)
    try:
        for step, (part, state, (b, mo, mt)) in enumerate(chain(seed, n_txn, n_keys)):
            q = CC.recovery_queries(b, QUERY_SEEDS[seed], 120)
            final = step == len(CUTS)
            if not final:
                # the case exercises the missing[] test: asserted on the oracle alone, before the device is asked
                assert len(state["mmsb"]) > 0 and len(mt) > 0
                ow = oracle.map_reduce_full(b, mo, mt, q, ANY, WITH, ANY_STATUS)
                owo = oracle.map_reduce_full(b, mo, mt, q, ANY, WITHOUT, ANY_STATUS)
                assert len(ow.dep_txn) > 0 and len(owo.dep_txn) > 0
                assert not (np.array_equal(ow.arena, owo.arena) and np.array_equal(ow.dep_txn, owo.dep_txn))
                q = concat_queries(q, missing_queries(state))
            else:
                assert len(state["mmsb"]) == 0
            st.apply_deps(part)
            before = st.state()
            hits = 0
            for kinds, after in ((-1, False), (-1, True), (MASK, False)) if not final else ((-1, False),):
                for sa, td, ts in RC.ALL_TESTS:
                    msg = f"seed {seed} batch {step} {(sa, td, ts)} kinds {kinds} after {after}"
                    o = oracle.map_reduce_full(b, mo, mt, q, sa, td, ts, test_kinds=kinds, exec_after=after)
                    g = st.map_reduce_full(q, sa, td, ts, test_kinds=kinds, executes_after=after)
                    assert_same(g, o, msg)
                    np.testing.assert_array_equal(g.kd_key, expect_kd_key(o, q), err_msg=msg)
                    r = cfk_map_reduce_full(ctx, st.missing_view(), q, sa, td, ts, test_kinds=kinds, executes_after=after)
                    assert_same(g, r, msg + " against acc_map_reduce_full over acc_cfk_missing")
                    hits += len(o.dep_txn)
            assert hits > 0
            after_state = st.state()
            for k in before:
                np.testing.assert_array_equal(after_state[k], before[k], err_msg=f"the scans modified the store: {k}")
    finally:
        st.close()


# ---------------------------------------------------------------- b. chunk boundaries

def boundary_items(Ln):
    """X at the first entry, entries 255 and 256, the last entry (members), one hlc below the first, between two
    entries and above the last (no members), each on key 900 (Ln entries at hlc 4, 8, ..) and its neighbour 901"""
    members = sorted({0, 255, 256, Ln - 1} & set(range(Ln)))
    hlcs = [4 * j + 4 for j in members] + [3, 4 * 100 + 4 + 1, 4 * (Ln + 1) + 4 + 5]
    return [(KQ.ts(h), [900, 901], []) for h in hlcs]


@pytest.mark.parametrize("Ln", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_chunk_boundaries(ctx, Ln):
    from accord_amd.deps import CfkStore
    upd = KQ.width_stream(Ln, 10)
    state = oracle.cfk_apply(CC.empty_snapshot(), upd)
    b, mo, mt = CC.snap_as_batch(state)
    items = boundary_items(Ln)
    q = make_queries(items)
    kq = as_key_queries(state, items, 1)
    seen = set()
    st = CfkStore(ctx)
    try:
        st.apply_deps(upd)
        for td in (ANY_DEPS, WITHOUT):
            for sa in (BEFORE, AFTER, ANY):
                w = windows(state, kq, sa, td)
                seen |= set(int(x) for x in w)
                o = oracle.map_reduce_full(b, mo, mt, kq, sa, td, ANY_STATUS)
                g = st.map_reduce_full(q, sa, td, ANY_STATUS)
                stt = ctx.stats()
                assert stt["cfr.pairs"] == len(w) and stt["cfr.chunks"] == int(chunks_of(w).sum()), f"L {Ln} {(sa, td)}: {stt}"
                assert stt["cfr.hits"] == len(o.arena) - len(o.key_idx)
                assert_same(g, o, f"L {Ln} {(sa, td)}")
        # empty windows, one-entry windows and windows ending exactly on a chunk edge all occurred
        assert 0 in seen and 1 in seen and (CHUNK in seen or Ln < CHUNK)
        if Ln > CHUNK:
            assert CHUNK + 1 in seen or Ln - CHUNK in seen
    finally:
        st.close()


# ---------------------------------------------------------------- c. long missing[]

N_OPEN = 72


def long_missing_stream():
    """N_OPEN PREACCEPTED Writes on key 700, then a STABLE Write whose deps name none of them (its missing[] holds them
    all), then a STABLE Write whose deps name every one"""
    cols = {k: [] for k in ("msb", "lsb", "node", "xmsb", "xlsb", "xnode", "status", "flags")}
    open_ids = [KQ.ts(4 * i + 4) for i in range(N_OPEN)]
    late = [KQ.ts(4 * N_OPEN + 40), KQ.ts(4 * N_OPEN + 44)]
    dep_off, dm, dl, dn = [0], [], [], []
    for tid, stt, deps in [(t, CC.PRE, []) for t in open_ids] + [(late[0], CC.STABLE, []), (late[1], CC.STABLE, open_ids)]:
        for k, v in zip(cols, (tid[0], tid[1], tid[2], tid[0], tid[1], tid[2], stt, 0)):
            cols[k].append(v)
        for d in deps:
            dm.append(d[0]); dl.append(d[1]); dn.append(d[2])
        dep_off.append(len(dm))
    n = N_OPEN + 2
    upd = {k: np.array(v, dt) for (k, v), dt in zip(cols.items(), (np.uint64, np.uint64, np.int32, np.uint64, np.uint64,
                                                                  np.int32, np.uint8, np.uint8))}
    upd.update(key_off=np.arange(n + 1, dtype=np.uint32), key=np.full(n, 700, np.uint64), dep_off=np.array(dep_off, np.uint32),
               dmsb=np.array(dm, np.uint64), dlsb=np.array(dl, np.uint64), dnode=np.array(dn, np.int32))
    return upd, open_ids


def test_long_missing(ctx):
    from accord_amd.deps import CfkStore
    upd, open_ids = long_missing_stream()
    state = oracle.cfk_apply(CC.empty_snapshot(), upd)
    per = np.diff(state["miss_off"].astype(np.int64))
    assert int(per[N_OPEN]) >= 70 and int(per[N_OPEN + 1]) == 0, "the first late entry misses every open txn, the second none"
    b, mo, mt = CC.snap_as_batch(state)
    items = [(open_ids[0], [700], []), (open_ids[N_OPEN // 2], [700], []), (open_ids[-1], [700], []),
             (KQ.ts(4 * 20 + 4 + 1), [700], [])]
    q = make_queries(items)
    kq = as_key_queries(state, items, 1)
    ow = oracle.map_reduce_full(b, mo, mt, kq, ANY, WITH, ANY_STATUS)
    owo = oracle.map_reduce_full(b, mo, mt, kq, ANY, WITHOUT, ANY_STATUS)
    # the oracle splits the two late entries: WITH sees the one that names X, WITHOUT the one that misses it
    np.testing.assert_array_equal(ow.dep_txn, [N_OPEN + 1] * 3)
    np.testing.assert_array_equal(owo.dep_txn, [N_OPEN] * 3)
    np.testing.assert_array_equal(ow.u_off, [0, 1, 2, 3, 3])
    st = CfkStore(ctx)
    try:
        st.apply_deps(upd)
        for sa in (BEFORE, AFTER, ANY):
            for td in (WITH, WITHOUT, ANY_DEPS):
                for ts in (ANY_STATUS, IS_STABLE):
                    o = oracle.map_reduce_full(b, mo, mt, kq, sa, td, ts)
                    assert_same(st.map_reduce_full(q, sa, td, ts), o, f"long missing {(sa, td, ts)}")
    finally:
        st.close()


# ---------------------------------------------------------------- d. range-domain queries

def range_items(b):
    """the (4, 160, 10) store holds keys 100, 110, .., 190"""
    member = lambda t, dom: (int(b.txn_msb[t]), int(b.txn_lsb[t]) | dom, int(b.txn_node[t]))  # noqa: E731
    foreign = KQ.ts(4 * 30 + 4 + 1, (1 << 1) | 1)       # a range-domain Write on an odd hlc: no store TxnId
    t0, t1 = b.n_txn // 3, 2 * b.n_txn // 3
    keys_of = lambda t: [int(k) for k in b.key_code[int(b.key_off[t]):int(b.key_off[t + 1])]]  # noqa: E731
    return [
        (member(t0, 1), [], [(101, 109)]),                       # covers no store key
        (member(t0, 1), [], [(109, 110)]),                       # (109, 110] covers 110, [109, 110) nothing
        (member(t0, 0), keys_of(t0), []),                        # a key query between them
        (member(t1, 1), [], [(95, 195)]),                        # every key
        (foreign, [], [(95, 195)]),
        (member(t1, 1), [], [(100, 120), (120, 140)]),           # touching ranges
        (foreign, [], [(105, 130)]),                             # ends exactly on a key
        (member(t1, 0), sorted(set(keys_of(t1)) | {7}), []),
        (member(t0, 1), [], [(110, 111), (150, 190)]),
        (foreign, [], []),                                       # no participants
    ], foreign


@pytest.mark.parametrize("end_inclusive", [1, 0], ids=["end_inclusive", "start_inclusive"])
def test_range_domain_queries(ctx, end_inclusive):
    from accord_amd.deps import CfkStore
    steps = chain(*CASES[0])[:len(CUTS)]          # the store after the third batch: missing[] lists are populated
    state, (b, mo, mt) = steps[-1][1], steps[-1][2]
    assert len(mt) > 0
    items, foreign = range_items(b)
    q = make_queries(items)
    kq = as_key_queries(state, items, end_inclusive)
    per = np.diff(kq["key_off"].astype(np.int64))
    assert per[0] == 0 and per[1] == (1 if end_inclusive else 0) and per[3] == 10
    assert per[6] == (3 if end_inclusive else 2) and per[5] == 4
    st = CfkStore(ctx)
    try:
        for part, _, _ in steps:
            st.apply_deps(part)
        for sa, td, ts in RC.ALL_TESTS:
            o = oracle.map_reduce_full(b, mo, mt, kq, sa, td, ts)
            g = st.map_reduce_full(q, sa, td, ts, end_inclusive=end_inclusive)
            assert_same(g, o, f"ranges {(sa, td, ts)}")
            np.testing.assert_array_equal(g.kd_key, expect_kd_key(o, kq), err_msg=f"kd_key {(sa, td, ts)}")
            assert ctx.stats()["cfr.range_pairs"] == int(per[[i for i, it in enumerate(items) if it[2]]].sum())
            u = np.asarray(g.u_off).astype(np.int64)
            if td == WITH:
                for i, it in enumerate(items):
                    if it[0] == foreign:
                        assert u[i + 1] == u[i], "WITH: a range txn that is no member of a key gets nothing from it"
            if (sa, td, ts) == (ANY, ANY_DEPS, ANY_STATUS):
                assert u[5] > u[4] and u[7] > u[6], "ANY_DEPS: the covered keys' entries"
    finally:
        st.close()


# ---------------------------------------------------------------- e. builder tiers

@pytest.mark.parametrize("cap", [1, KQ.SMALL_CAP])
def test_builder_tiers(ctx, cap):
    from accord_amd.deps import CfkStore, Context
    steps = chain(*CASES[1])[:len(CUTS)]
    _, state, (b, mo, mt) = steps[-1]
    q = concat_queries(CC.recovery_queries(b, QUERY_SEEDS[6], 120), missing_queries(state))
    with Context(0, cfq_wave_cap=cap) as c:
        st, ref = CfkStore(c), CfkStore(ctx)
        try:
            for part, _, _ in steps:
                st.apply_deps(part)
                ref.apply_deps(part)
            sorted_hits = 0
            for sa, td, ts in [(BEFORE, WITHOUT, IS_PROPOSED), (BEFORE, WITH, IS_STABLE), (AFTER, WITHOUT, IS_PROPOSED),
                               (ANY, WITHOUT, IS_STABLE), (ANY, ANY_DEPS, ANY_STATUS), (BEFORE, ANY_DEPS, ANY_STATUS)]:
                o = oracle.map_reduce_full(b, mo, mt, q, sa, td, ts)
                g = st.map_reduce_full(q, sa, td, ts)
                stt = c.stats()
                sorted_hits += stt["cfr.sorted_hits"]
                if (sa, td, ts) == (ANY, ANY_DEPS, ANY_STATUS):
                    assert 0 < stt["cfr.sorted_hits"] and (cap == 1 or stt["cfr.sorted_hits"] < stt["cfr.hits"])
                assert_same(g, o, f"cap {cap} {(sa, td, ts)}")
                assert_same(g, ref.map_reduce_full(q, sa, td, ts), f"cap {cap} {(sa, td, ts)} against the default cap",
                            FIELDS + ("kd_key",))
            assert sorted_hits > 0
        finally:
            st.close()
            ref.close()


# ---------------------------------------------------------------- f. sliced launches

def launches(n, limit):
    return -(-n // ((limit or DEFAULT_LIMIT) * WAVES))


def cfr_launches(stt, nq, limit):
    """cfr.wave_launches of one call from its other stats, the way test_wave_slices_gpu.cfq_launches does it for the
    KeyDeps scan: NC = cfr.chunks > 0 gives cr_count over NC; E = cfr.hits > 0 gives cr_emit over NC; E > G =
    cfr.sorted_hits gives cq_build_wave over the nq queries"""
    NC, E, G = stt["cfr.chunks"], stt["cfr.hits"], stt["cfr.sorted_hits"]
    return (launches(NC, limit) if NC else 0) + (launches(NC, limit) if E else 0) + (launches(nq, limit) if E > G else 0)


def test_sliced_launches(ctx):
    from accord_amd.deps import CfkStore, Context
    Ln = 2 * CHUNK + 1
    upd = KQ.width_stream(Ln, 10)
    state = oracle.cfk_apply(CC.empty_snapshot(), upd)
    b, mo, mt = CC.snap_as_batch(state)
    base = boundary_items(Ln)
    base_nc = int(chunks_of(windows(state, as_key_queries(state, base, 1), ANY, ANY_DEPS)).sum())
    fill = (-base_nc) % 24
    top = 4 * (Ln + 1) + 4
    items = base + [(KQ.ts(top + 21 + 2 * i), [901], []) for i in range(fill + 1)]     # one chunk each
    ctxs = {0: ctx}
    ctxs.update({lim: Context(0, wave_grid_max=lim) for lim in (1, 2, 3)})
    stores = {lim: CfkStore(c) for lim, c in ctxs.items()}
    try:
        for s in stores.values():
            s.apply_deps(upd)
        for drop, rem in ((1, 0), (0, 1)):
            its = items[:len(items) - drop]
            q = make_queries(its)
            kq = as_key_queries(state, its, 1)
            for sa, td in ((ANY, ANY_DEPS), (BEFORE, ANY_DEPS), (AFTER, WITHOUT)):
                NC = int(chunks_of(windows(state, kq, sa, td)).sum())
                if (sa, td) == (ANY, ANY_DEPS):
                    assert NC % 24 == rem and all(NC % (lim * WAVES) == rem for lim in (1, 2, 3))
                o = oracle.map_reduce_full(b, mo, mt, kq, sa, td, ANY_STATUS)
                for lim, c in ctxs.items():
                    g = stores[lim].map_reduce_full(q, sa, td, ANY_STATUS)
                    stt = c.stats()
                    assert stt["cfr.chunks"] == NC
                    assert stt["cfr.wave_launches"] == cfr_launches(stt, len(its), lim), f"{(sa, td)} limit {lim}: {stt}"
                    if lim == 0:
                        assert stt["cfr.wave_launches"] == (NC > 0) + (stt["cfr.hits"] > 0) + (stt["cfr.hits"] > stt["cfr.sorted_hits"])
                    elif (sa, td) == (ANY, ANY_DEPS):
                        # the last launch of the chunk kernels is full (rem 0) or holds one wave (rem 1)
                        assert launches(NC, lim) == NC // (lim * WAVES) + rem
                    assert_same(g, o, f"{(sa, td)} NC {NC} limit {lim}")
    finally:
        for s in stores.values():
            s.close()
        for lim in (1, 2, 3):
            ctxs[lim].close()


# ---------------------------------------------------------------- g. edges and errors

def assert_empty(g, nq):
    for f in ("arena_off", "kd_off", "u_off"):
        np.testing.assert_array_equal(getattr(g, f), [0] * (nq + 1))
    assert len(g.arena) == len(g.key_idx) == len(g.dep_txn) == 0


def test_edges_and_errors(ctx):
    from accord_amd import workload as W
    from accord_amd.deps import CfkStore, IllegalArgumentException, IllegalStateException
    upd, _ = CC.handmade()                      # [A COMMITTED, B COMMITTED, C ACCEPTED] on key 500
    s, empty, status_only = CfkStore(ctx), CfkStore(ctx), CfkStore(ctx)
    try:
        s.apply_deps(upd)
        state = oracle.cfk_apply(CC.empty_snapshot(), upd)
        b, mo, mt = CC.snap_as_batch(state)
        good_items = [(KQ.ts(8), [500], []), (KQ.ts(9, (1 << 1) | 1), [], [(400, 500)])]
        good = make_queries(good_items)
        want = oracle.map_reduce_full(b, mo, mt, as_key_queries(state, good_items, 1), ANY, ANY_DEPS, ANY_STATUS)
        assert len(want.dep_txn) == 6

        def check_good():
            assert_same(s.map_reduce_full(good, ANY, ANY_DEPS, ANY_STATUS), want, "a good call")

        def fails(exc, items, sa=ANY, td=ANY_DEPS, ts=ANY_STATUS, **kw):
            before = s.state()
            with pytest.raises(exc):
                s.map_reduce_full(items if isinstance(items, dict) else make_queries(items), sa, td, ts, **kw)
            check_good()
            after = s.state()
            for k in before:
                np.testing.assert_array_equal(after[k], before[k])

        check_good()
        fails(IllegalArgumentException, [(KQ.ts(8), [501, 500], [])])                        # unsorted keys
        fails(IllegalArgumentException, [(KQ.ts(8, (1 << 1) | 1), [500], [])])               # a range query listing keys
        fails(IllegalArgumentException, [(KQ.ts(8), [], [(400, 500)])])                      # a key query listing ranges
        fails(IllegalArgumentException, [(KQ.ts(8, (1 << 1) | 1), [], [(500, 500)])])        # start >= end
        fails(IllegalArgumentException, [(KQ.ts(8, (1 << 1) | 1), [], [(400, 500), (450, 600)])])   # overlapping ranges
        fails(IllegalArgumentException, good, sa=3)                                          # no such TestStartedAt
        fails(IllegalArgumentException, good, td=3)
        fails(IllegalArgumentException, good, ts=3)
        fails(IllegalArgumentException, good, end_inclusive=2)
        fails(IllegalArgumentException, dict(good, key_off=np.array([1, 1, 1], np.uint32)))  # offsets do not start at 0
        fails(IllegalArgumentException, [(KQ.ts(8, 6 << 1), [500], [])])                     # Kind.ofOrdinal
        fails(IllegalStateException, [(KQ.ts(8, 5 << 1), [500], [])])                        # LocalOnly: witnessedBy() throws
        # an unknown flags bit: the Python entry only ever sets ACC_FULL_EXECUTES_AFTER, so the struct is built here
        import ctypes as C
        a = {k: np.ascontiguousarray(v) for k, v in good.items()}
        p = lambda k: a[k].ctypes.data  # noqa: E731
        ri = L.CfkRecoveryIn(2, L.ACC_MEM_HOST, len(a["key_code"]), len(a["rng_start"]), L.TsCols(p("msb"), p("lsb"), p("node")),
                             p("key_off"), p("key_code"), p("rng_off"), p("rng_start"), p("rng_end"), 1, ANY, ANY_DEPS,
                             ANY_STATUS, 2, -1)
        with pytest.raises(IllegalArgumentException):
            ctx.check(ctx._lib.acc_cfk_map_reduce_full(ctx.handle, s._h, C.byref(ri), C.byref(L.KeydepsView())))
        check_good()
        # a LocalOnly X under an explicit Kinds mask is answered: witnessedBy() is never asked
        g = s.map_reduce_full(make_queries([(KQ.ts(8, 5 << 1), [500], [])]), ANY, ANY_DEPS, ANY_STATUS, test_kinds=1 << 1)
        assert len(g.dep_txn) == 3

        status_only.update(W.keydeps_batch(50, 2, 10, 7, "uniform"))
        with pytest.raises(IllegalStateException):
            status_only.map_reduce_full(good, ANY, ANY_DEPS, ANY_STATUS)
        check_good()

        for st in (empty, s):
            assert_empty(st.map_reduce_full(make_queries([]), ANY, ANY_DEPS, ANY_STATUS), 0)             # n_query == 0
        assert_empty(empty.map_reduce_full(good, ANY, ANY_DEPS, ANY_STATUS), 2)                          # an empty store
        assert_empty(s.map_reduce_full(make_queries([(KQ.ts(8), [], []), (KQ.ts(9, 3), [], [])]), ANY, ANY_DEPS, ANY_STATUS), 2)
        # rng_* left out of a batch of key-domain queries
        kq = {k: good[k] for k in ("msb", "lsb", "node")}
        kq.update(key_off=np.array([0, 1, 1], np.uint32), key_code=np.array([500], np.uint64))
        kq["lsb"] = kq["lsb"] & ~np.uint64(1)
        g = s.map_reduce_full(kq, ANY, ANY_DEPS, ANY_STATUS)
        np.testing.assert_array_equal(g.u_off, [0, 3, 3])
        check_good()
    finally:
        s.close()
        empty.close()
        status_only.close()


# ---------------------------------------------------------------- h. ReplicaStore.begin_recovery

def test_begin_recovery(ctx):
    from accord_amd.deps import ReplicaStore
    steps = chain(*CASES[0])
    rs = ReplicaStore(ctx)
    try:
        for step, (part, state, (b, mo, mt)) in enumerate(steps):
            rs.cfk.apply_deps(part)
            q = CC.recovery_queries(b, 40 + step, 120)
            r = rs.begin_recovery(q)
            assert sorted(r) == ["accepted_started_before_without", "has_accepted_started_after_without",
                                 "has_stable_executes_after_without", "stable_started_before_with"]
            # BeginRecovery.java:334-341, 348, 365, 378
            o = oracle.map_reduce_full(b, mo, mt, q, BEFORE, WITHOUT, IS_PROPOSED, exec_after=True)
            assert_same(r["accepted_started_before_without"], o, f"batch {step} :334")
            o = oracle.map_reduce_full(b, mo, mt, q, BEFORE, WITH, IS_STABLE)
            assert_same(r["stable_started_before_with"], o, f"batch {step} :348")
            o = oracle.map_reduce_full(b, mo, mt, q, AFTER, WITHOUT, IS_PROPOSED)
            np.testing.assert_array_equal(r["has_accepted_started_after_without"], np.diff(o.u_off.astype(np.int64)) > 0)
            o = oracle.map_reduce_full(b, mo, mt, q, ANY, WITHOUT, IS_STABLE)
            np.testing.assert_array_equal(r["has_stable_executes_after_without"], np.diff(o.u_off.astype(np.int64)) > 0)
            assert r["has_stable_executes_after_without"].dtype == np.bool_ and len(r["has_stable_executes_after_without"]) == 120
    finally:
        rs.close()
