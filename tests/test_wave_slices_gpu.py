"""GPU parity under sliced wave-per-item launches (csrc/ctx.hpp launch_waves). A wave-per-chunk launch over 2^26 chunks
asks for 2^32 work-items, more than a dispatch holds, so such launches go out in slices of at most acc_opts.wave_grid_max
blocks (default 2^23), each kernel being told its slice's first item. The default slice needs 2^25 items before a second
one starts; the contexts here lower the knob to 1, 2 and 3 blocks = 4, 8 and 12 items per launch, so a few thousand chunks
take hundreds of launches and every `first +`, the loop's step and the last slice's grid decide the result.

Every comparison is exact array equality with the C restatement, through the helpers of test_cfk_query_gpu,
test_cfk_query_mixed_gpu and recovery_cases. After every device call the launch counter the entry point publishes is
compared with the count worked out from the call's other stats (cfq_launches, recovery_launches below): a launcher that
ignored the knob, stepped by another amount or issued an empty trailing launch would miss it."""
import numpy as np
import pytest

import cfk_cases as CC
import oracle
import recovery_cases as RC
import test_cfk_query_gpu as KQ
import test_cfk_query_mixed_gpu as MQ
from accord_amd import _lib as L

pytestmark = pytest.mark.gpu

CHUNK = KQ.CHUNK
WAVES = 4                    # items (waves) per block of a sliced launch
DEFAULT_LIMIT = 1 << 23      # blocks per slice when the knob is 0
LIMITS = (0, 1, 2, 3)        # 0: the default
IDENTITY_LSB = 0xFFFFFFFFFFFF001E


@pytest.fixture(scope="module")
def ctxs():
    """limit -> context (0: the default)"""
    from accord_amd.deps import Context
    cs = {lim: Context(0, wave_grid_max=lim) for lim in LIMITS}
    yield cs
    for c in cs.values():
        c.close()


def per_slice(limit):
    return (limit or DEFAULT_LIMIT) * WAVES


def launches(n, limit):
    """launches of one sliced launch over n items"""
    return -(-n // per_slice(limit))


def cfq_launches(st, nq, limit):
    """cfq.wave_launches of one acc_cfk_keydeps / acc_cfk_keydeps_mixed call from its other stats (scan_located,
    csrc/cfkquery.hip): NC = cfq.chunks > 0 gives cq_max over NC, cq_fold over Qp = cfq.pairs and cq_count over NC;
    E = cfq.hits > 0 gives cq_emit over NC; E > G = cfq.sorted_hits gives cq_build_wave over the nq queries"""
    NC, Qp, E, G = st["cfq.chunks"], st["cfq.pairs"], st["cfq.hits"], st["cfq.sorted_hits"]
    n = 0
    if NC:
        n += 2 * launches(NC, limit) + launches(Qp, limit)
    if E:
        n += launches(NC, limit)
    if E > G:
        n += launches(nq, limit)
    return n


def recovery_launches(chunks, entries, limit):
    """recovery.wave_launches (recovery.range_wave_launches) of one call: NC = recovery.chunks (range_chunks) > 0 gives
    rc_count (rr_count) over NC; a call that emits anything, recovery.entries (range_entries) > 0, gives rc_emit (rr_emit)
    over NC again"""
    return (launches(chunks, limit) if chunks else 0) + (launches(chunks, limit) if entries else 0)


def check_cfq_launches(c, nq, limit, msg):
    st = c.stats()
    assert st["cfq.wave_launches"] == cfq_launches(st, nq, limit), f"{msg}: launches at limit {limit}, stats {st}"
    return st


# ---------------------------------------------------------------- a. acc_cfk_keydeps: chunk against slice boundaries

def pair_chunks(state, q):
    """chunks of every (query, key) pair of q, on the host: the pair's prefix = the entries of its key's segment with
    TxnId < the query's executeAt (Timestamp order), in CHUNK-entry chunks"""
    tkey = lambda m, l, n: (int(m), int(l) & IDENTITY_LSB, int(n))   # noqa: E731
    off = state["ent_off"].astype(np.int64)
    seg = {int(k): [tkey(state["emsb"][e], state["elsb"][e], state["enode"][e]) for e in range(off[j], off[j + 1])]
           for j, k in enumerate(state["key"])}
    out = []
    for i in range(len(q["msb"])):
        S = tkey(q["xmsb"][i], q["xlsb"][i], q["xnode"][i])
        for k in q["key_code"][int(q["key_off"][i]):int(q["key_off"][i + 1])]:
            w = sum(1 for t in seg.get(int(k), ()) if t < S)
            out.append(-(-w // CHUNK))
    return np.array(out, np.int64)


@pytest.mark.parametrize("tail", [10, 300])
def test_keydeps_chunk_and_slice_boundaries(ctxs, tail):
    """width_stream(2 CHUNK + 1, tail) under test_segment_widths' queries, followed by single-key queries on key 901 (one
    chunk each) that steer the chunk total: one call whose NC is a multiple of 24, so of every lowered slice size (no
    empty launch may follow), one with one query more (the last launch holds one wave). The placement the case is built
    for is asserted from the host's chunk arithmetic, which cfq.chunks and cfq.pairs pin to the device's."""
    from accord_amd.deps import CfkStore
    Ln = 2 * CHUNK + 1
    upd = KQ.width_stream(Ln, tail)
    state = oracle.cfk_apply(CC.empty_snapshot(), upd)
    ob = CC.snap_as_batch(state)[0]
    base, _ = KQ.width_items(Ln, tail)
    top = 4 * (Ln + 1) + 4
    base_nc = int(pair_chunks(state, KQ.make_queries(base)).sum())
    fill = (-base_nc) % 24
    items = base + [(KQ.ts(top + 21 + 2 * i), None, [901]) for i in range(fill + 1)]
    want_members = oracle.keydeps_batch(ob)
    stores = {lim: CfkStore(c) for lim, c in ctxs.items()}
    try:
        for s in stores.values():
            s.apply_deps(upd)
        for drop, rem in ((1, 0), (0, 1)):
            its = items[:len(items) - drop]
            q = KQ.make_queries(its)
            ch = pair_chunks(state, q)
            c_off = np.concatenate([[0], np.cumsum(ch)])
            NC = int(c_off[-1])
            assert NC % 24 == rem and all(NC % per_slice(lim) == rem for lim in (1, 2, 3))
            # at limit 1: a three-chunk pair whose chunks come from two launches, and a slice that ends where a pair ends
            assert any(ch[i] == 3 and c_off[i] // 4 != (c_off[i + 1] - 1) // 4 for i in range(len(ch)))
            assert any(ch[i] and ch[i - 1] and c_off[i] % 4 == 0 for i in range(1, len(ch)))
            want = KQ.expect_foreign(ob, its)
            for lim, c in ctxs.items():
                g = stores[lim].keydeps(q)
                st = check_cfq_launches(c, len(its), lim, f"tail {tail} foreign")
                assert st["cfq.chunks"] == NC and st["cfq.pairs"] == len(ch)
                KQ.assert_result(g, want, f"tail {tail} NC {NC} limit {lim}")
                if lim == 0:
                    # every sliced kernel ran, once each
                    assert st["cfq.hits"] > st["cfq.sorted_hits"] and st["cfq.wave_launches"] == 5
                else:
                    # the last launch of the chunk kernels is full (rem 0) or holds one wave (rem 1)
                    assert launches(NC, lim) == NC // per_slice(lim) + rem
        for lim, c in ctxs.items():
            g = stores[lim].keydeps(KQ.member_queries(ob))
            check_cfq_launches(c, ob.n_txn, lim, f"tail {tail} members")
            KQ.assert_result(g, want_members, f"tail {tail} members limit {lim}")
    finally:
        for s in stores.values():
            s.close()


# ---------------------------------------------------------------- b. the build tiers under slicing

def test_build_tiers_sliced():
    """test_member_and_foreign_queries, seed 22, with four queries per cq_build_wave launch and the one-wave tier capped
    at 11 hits: the wave tier runs in many slices beside the sorting tier"""
    from accord_amd.deps import CfkStore, Context
    seed = KQ.SEEDS[0]
    upd = CC.cfk_case(seed, n_txn=200, n_keys=12, keys_per=3)
    n = len(upd["msb"])
    a, rest = CC.split_updates(upd, int(n * 0.4))
    b, d = CC.split_updates(rest, int(n * 0.7) - int(n * 0.4))
    with Context(0, wave_grid_max=1, cfq_wave_cap=KQ.SMALL_CAP) as c:
        s = CfkStore(c)
        try:
            o_state = CC.empty_snapshot()
            for step, part in enumerate((a, b, d)):
                s.apply_deps(part)
                o_state = oracle.cfk_apply(o_state, part)
                assert KQ.no_committed_ties(o_state)
                ob = CC.snap_as_batch(o_state)[0]
                g = s.keydeps(KQ.member_queries(ob))
                st = check_cfq_launches(c, ob.n_txn, 1, f"slice {step} members")
                assert st["cfq.sorted_hits"] > 0 and st["cfq.hits"] > st["cfq.sorted_hits"], "both build tiers"
                assert launches(ob.n_txn, 1) > 10
                KQ.assert_result(g, oracle.keydeps_batch(ob), f"slice {step} members")
                items = KQ.foreign_items(ob, seed + step)
                g = s.keydeps(KQ.make_queries(items))
                check_cfq_launches(c, len(items), 1, f"slice {step} foreign")
                KQ.assert_result(g, KQ.expect_foreign(ob, items), f"slice {step} foreign")
        finally:
            s.close()


# ---------------------------------------------------------------- c. acc_cfk_keydeps_mixed

LANE_SEG_DEFAULT = 16        # what lane_seg = 0 stands for (csrc/cfkquery.hip)
NONE = L.ACC_CFQ_LANE_NONE


def lane_pairs(ob, items, end_inclusive, lane_seg):
    """the (range query, covered key) pairs the lane tier answers, on the host: the covered store keys whose whole
    segment holds at most lane_seg entries"""
    codes, seg_len = np.unique(ob.key_code, return_counts=True)
    n = 0
    for _, _, _, ranges in items:
        for a, b in ranges:
            cov = (codes > a) & (codes <= b) if end_inclusive else (codes >= a) & (codes < b)
            n += int(np.count_nonzero(cov & (seg_len <= lane_seg)))
    return n


def run_mixed(ctxs, stores, ob, items, want, end_inclusive, lane_segs, msg):
    """the call on the default context and on limits 1 and 3, per lane_seg; returns the lane tier's pairs per lane_seg.
    A lane-tier pair keeps one chunk slot, which the sliced chunk kernels see as empty."""
    q = MQ.make_mixed(items)
    seen = {}
    for lane_seg in lane_segs:
        lp = 0 if lane_seg == NONE else lane_pairs(ob, items, end_inclusive, lane_seg or LANE_SEG_DEFAULT)
        for lim in (0, 1, 3):
            g = stores[lim].keydeps_mixed(q, end_inclusive, lane_seg)
            st = check_cfq_launches(ctxs[lim], len(items), lim, f"{msg} lane_seg {lane_seg}")
            assert st["cfq.lane_pairs"] == lp and st["cfq.chunks"] >= lp, f"{msg} lane_seg {lane_seg} limit {lim}: {st}"
            MQ.assert_result(g, want, f"{msg} limit {lim} lane_seg {lane_seg}")
        seen[lane_seg] = lp
    return seen


@pytest.mark.parametrize("end_inclusive", [1, 0], ids=["end_inclusive", "start_inclusive"])
def test_mixed_seeded_sliced(ctxs, end_inclusive):
    """test_seeded_key_and_range_queries, seed 22, with and without the lane tier. Every key of this store holds more
    than the default lane_seg's 16 entries from the first slice on, so the default leaves the tier idle here (asserted
    against the host's count like every other run; the ladder store below is where the default engages it); lane_seg 64
    sends the shorter segments through it."""
    from accord_amd.deps import CfkStore
    seed = MQ.SEEDS[0]
    upd = CC.cfk_case(seed, n_txn=200, n_keys=12, keys_per=3)
    n = len(upd["msb"])
    a, rest = CC.split_updates(upd, int(n * 0.4))
    b, d = CC.split_updates(rest, int(n * 0.7) - int(n * 0.4))
    stores = {lim: CfkStore(ctxs[lim]) for lim in (0, 1, 3)}
    try:
        o_state = CC.empty_snapshot()
        wide = 0
        for step, part in enumerate((a, b, d)):
            for s in stores.values():
                s.apply_deps(part)
            o_state = oracle.cfk_apply(o_state, part)
            assert MQ.no_committed_ties(o_state)
            ob = CC.snap_as_batch(o_state)[0]
            items = MQ.interleave(MQ.foreign_items(ob, seed + step), MQ.foreign_range_items(ob, seed + step))
            seen = run_mixed(ctxs, stores, ob, items, MQ.expect_mixed(ob, items, end_inclusive), end_inclusive, (0, 64, NONE),
                             f"seed {seed} slice {step}")
            wide = max(wide, seen[64])
        assert wide > 0
    finally:
        for s in stores.values():
            s.close()


@pytest.mark.parametrize("end_inclusive", [1, 0], ids=["end_inclusive", "start_inclusive"])
def test_mixed_ladder_sliced(ctxs, end_inclusive):
    """test_segment_ladder's store: with the lane tier, the three shortest of a full range's thirteen segments are single empty
    chunk slots among the chunks of the others"""
    from accord_amd.deps import CfkStore
    upd, ob, items = MQ.ladder_case()
    want = MQ.expect_mixed(ob, items, end_inclusive)
    stores = {lim: CfkStore(ctxs[lim]) for lim in (0, 1, 3)}
    try:
        for s in stores.values():
            s.apply_deps(upd)
        seen = run_mixed(ctxs, stores, ob, items, want, end_inclusive, (0, NONE), "ladder")
        assert seen[0] > 0
    finally:
        for s in stores.values():
            s.close()


# ---------------------------------------------------------------- d. recovery, key and range

KEY_FIELDS = ("arena_off", "arena", "kd_off", "key_idx", "u_off", "dep_txn")
RANGE_FIELDS = ("rng_start", "rng_end", "arena_off", "arena", "rd_off", "range_id", "u_off", "dep_txn")


def test_recovery_hot_keys_sliced(ctxs):
    """test_recovery_hot_keys_multi_chunk's case and (sa, td, ts) triples: more than a thousand chunks, so hundreds of
    rc_count and rc_emit launches at limit 1. recovery.wave_launches = recovery_launches(recovery.chunks,
    recovery.entries, limit)."""
    b, mo, mt, q = RC.recovery_case(4, n=6000, keys_per=2, n_keys=5, n_query=200, p_missing=0.02)
    most = 0
    for sa, td, ts in [(0, 1, 1), (0, 0, 2), (1, 1, 1), (2, 1, 2), (2, 2, 0), (1, 2, 0)]:
        o = oracle.map_reduce_full(b, mo, mt, q, sa, td, ts)
        for lim in (0, 1, 3):
            g = ctxs[lim].map_reduce_full(b, mo, mt, q, sa, td, ts)
            st = ctxs[lim].stats()
            assert per_slice(3) < st["recovery.chunks"] < 10000
            most = max(most, st["recovery.chunks"])
            assert st["recovery.wave_launches"] == recovery_launches(st["recovery.chunks"], st["recovery.entries"], lim), \
                f"{(sa, td, ts)} limit {lim}: {st}"
            if lim == 0:
                assert st["recovery.wave_launches"] == 1 + (st["recovery.entries"] > 0)
            for f in KEY_FIELDS:
                np.testing.assert_array_equal(getattr(g, f), getattr(o, f), err_msg=f"{f} {(sa, td, ts)} limit {lim}")
    assert most > 1000


def test_range_recovery_sliced(ctxs):
    """test_range_recovery_all_tests, seed 1, every TestStartedAt x TestDep x TestStatus with and without the executeAt
    filter, four 64-command chunks per rr_count / rr_emit launch. recovery.range_wave_launches =
    recovery_launches(recovery.range_chunks, recovery.range_entries, limit)."""
    cmds, q = RC.range_recovery_case(1, n_cmd=400, n_query=300, end_inclusive=1)
    most, nonempty = 0, 0
    for sa, td, ts in RC.ALL_TESTS:
        for ea in (False, True):
            o = oracle.map_reduce_full_ranges(cmds, q, sa, td, ts, test_kinds=-1, exec_after=ea)
            for lim in (0, 1):
                g = ctxs[lim].map_reduce_full_ranges(cmds, q, sa, td, ts, test_kinds=-1, executes_after=ea)
                st = ctxs[lim].stats()
                assert st["recovery.range_wave_launches"] == \
                    recovery_launches(st["recovery.range_chunks"], st["recovery.range_entries"], lim), \
                    f"{(sa, td, ts, ea)} limit {lim}: {st}"
                assert st["recovery.range_chunks"] < 10000
                if lim == 0:
                    assert st["recovery.range_wave_launches"] == (st["recovery.range_chunks"] > 0) + (st["recovery.range_entries"] > 0)
                else:
                    most = max(most, st["recovery.range_chunks"])
                    nonempty += int(g.u_off[-1] > 0)
                for f in RANGE_FIELDS:
                    np.testing.assert_array_equal(np.asarray(getattr(g, f)).astype(np.int64), np.asarray(getattr(o, f)).astype(np.int64),
                                                  err_msg=f"{f} {(sa, td, ts, ea)} limit {lim}")
    assert most > per_slice(1), "no call read more chunks than one slice holds"
    assert nonempty > 40


# ---------------------------------------------------------------- f. the knob's edges

@pytest.mark.parametrize("knob", [(1 << 23) + 1, (1 << 32) - 1])
def test_knob_above_the_default_is_the_default(knob):
    from accord_amd.deps import CfkStore, Context
    upd = KQ.width_stream(CHUNK + 1, 10)
    ob = CC.snap_as_batch(oracle.cfk_apply(CC.empty_snapshot(), upd))[0]
    items, _ = KQ.width_items(CHUNK + 1, 10)
    with Context(0, wave_grid_max=knob) as c:
        s = CfkStore(c)
        try:
            s.apply_deps(upd)
            g = s.keydeps(KQ.make_queries(items))
            st = check_cfq_launches(c, len(items), 0, f"knob {knob}")
            assert st["cfq.wave_launches"] == 5, "cq_max, cq_fold, cq_count, cq_emit, cq_build_wave: one launch each"
            KQ.assert_result(g, KQ.expect_foreign(ob, items), f"knob {knob}")
        finally:
            s.close()
