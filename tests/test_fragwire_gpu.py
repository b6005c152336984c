"""The compact wire form of the KeyDeps fragments (csrc/fragwire.hip) in every form a message can take: slots as a
bitmap or a list, counts as u16 or u32, keys as u32 offsets or u64 codes, and the receiver's bookkeeping over sources
of different forms. Every case runs acc_shard_reduce (one: acc_partial_deps_reduce) over the host transport inside this
process (fragwire_harness.py), captures the messages and makes the harness's four comparisons: the independent model's
decode of each message against the explicit acc_shard_pack, the merged view against the single-store KeyDeps from the
oracle, the announced form against the form the reference streams call for, and the byte statistics. Each case also
states the form it was built to reach, so a case that misses its branch fails.

Also the argument and header checks that keep a bad n_global or a foreign message from reaching a kernel. No test
here hands the decoder a message whose body disagrees with a valid header: the body is checked on the device only."""
import functools

import numpy as np
import pytest

from accord_amd import workload as W

import fragwire_harness as H
import fragwire_model as M

pytestmark = pytest.mark.gpu

BITMAP, LIST, EMPTY = "bitmap", "list", "empty"


# ---------------------------------------------------------------- batches

def hand_batch(kind, status, keys, exe_after=None):
    """Txn i = TxnId hlc 2 (i + 1) of the given kind and status on the key codes keys[i] (ascending); executeAt =
    TxnId, or for the txns of exe_after {i: j} the odd hlc between the TxnIds of txns j and j + 1."""
    n = len(kind)
    i = np.arange(n, dtype=np.int64)
    kind = np.asarray(kind, dtype=np.int64)
    tm, tl, tn = W.encode_ts(np.ones(n), 2 * (i + 1), kind << 1, 1 + (i % 8))
    em, el, en = tm.copy(), tl.copy(), tn.copy()
    for a, j in (exe_after or {}).items():
        m, l, nd = W.encode_ts(np.ones(1), np.array([2 * (j + 1) + 1]), np.zeros(1), np.array([1000]))
        em[a], el[a], en[a] = m[0], l[0], nd[0]
    off = np.zeros(n + 1, np.uint32)
    np.cumsum([len(k) for k in keys], out=off[1:])
    code = np.array([c for k in keys for c in k], dtype=np.uint64)
    return W.Batch(tm, tl, tn, em, el, en, np.asarray(status, dtype=np.uint8), off, code, dict(n_txn=n))


@functools.lru_cache(maxsize=None)
def dense():
    import oracle
    b = W.keydeps_batch(20000, 8, 20000, 0xF4A6, "zipf", 0.99, status_model="model", window=2000)
    return b, oracle.keydeps_batch(b)


@functools.lru_cache(maxsize=None)
def small():
    import oracle
    b = W.keydeps_batch(3000, 6, 3000, 0xD15C, "zipf", 0.99, status_model="model", window=800)
    return b, oracle.keydeps_batch(b)


def run_one(b, gidx, n_global, queries=None):
    """World 1 over the loopback; the merged view expected from the oracle on the batch (queries: only for these
    txns, the others expected without deps)."""
    import oracle
    full = oracle.keydeps_batch(b, queries=queries)
    res = H.run_world([H.Store(b, gidx)], n_global)
    return res, full, [H.expected_home(full, b, gidx, n_global, 0, 1)]


# ---------------------------------------------------------------- dense

@pytest.mark.parametrize("store_local", [False, True])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_dense(world, store_local):
    """The suite's usual workload: bitmap slots, u16 counts, u32 key offsets on every message; world 1 sends more than
    8192 fragments to one destination (k_fe_dest's loop), and fragments start both below and above their own txn."""
    from accord_amd import sharded as S
    b, full = dense()
    bounds = S.even_split(b.key_code, world)
    stores = [H.Store(*S.store_batch(b, bounds, s)) if store_local else H.Store(S.shard_batch(b, bounds, s))
              for s in range(world)]
    res = H.run_world(stores, b.n_txn)
    expect = [S.home_result_from_full(full, b, r, world) for r in range(world)]
    for r in range(world):   # the placement-aware reference of the other cases is the same function here
        got = H.expected_home(full, b, None, b.n_txn, r, world)
        for f in H.MERGE_FIELDS:
            np.testing.assert_array_equal(got[f], expect[r][f], err_msg=f)
    forms, lens, signs = H.check_case(res, expect, f"dense world {world}")
    assert set(forms.values()) == {(BITMAP, False, False)}
    assert {-1, 1} <= signs, "first TxnIds on both sides of the fragment's txn"
    if world == 1:
        assert len(res.ref[0][0]["hdr"]) // 4 > 8192


# ---------------------------------------------------------------- slot list against bitmap

def test_slot_boundary():
    """n_global = 32 F: the bitmap is as long as the list and is kept; one more txn: the list is shorter."""
    b, full = small()
    gidx = np.arange(b.n_txn, dtype=np.uint32)
    rk = H.Rank(1, 0, H.loopback())
    try:
        ref = rk.load(H.Store(b, gidx))
        F = len(ref[0]["hdr"]) // 4
        assert 32 * F > b.n_txn
        for n_global, slots in ((32 * F, BITMAP), (32 * F + 1, LIST)):
            res = H.Result(1, n_global)
            res.ref[0], res.merged[0] = ref, rk.reduce(n_global)
            res.stats[0], res.msg = rk.ctx.stats(), {(0, d): m for d, m in rk.messages().items()}
            forms, _, _ = H.check_case(res, [H.expected_home(full, b, gidx, n_global, 0, 1)], f"n_global {n_global}")
            assert forms == {(0, 0): (slots, False, False)}
    finally:
        rk.close()


@pytest.mark.parametrize("rem", [0, 1, 31])
def test_bitmap_last_word(rem):
    """G mod 32 = 0, 1, 31 with a fragment in the last slot: the top used bit of the last bitmap word is set. The batch
    is placed at the end of the global txns, shifted so that their count has the remainder."""
    b, full = small()
    n_global = b.n_txn + (rem - b.n_txn) % 32
    gidx = (np.arange(b.n_txn) + (n_global - b.n_txn)).astype(np.uint32)
    res = H.run_world([H.Store(b, gidx)], n_global)
    assert int(res.ref[0][0]["hdr"][-4]) == n_global - 1 and n_global % 32 == rem
    forms, _, _ = H.check_case(res, [H.expected_home(full, b, gidx, n_global, 0, 1)], f"G {n_global}")
    assert forms == {(0, 0): (BITMAP, False, False)}


# ---------------------------------------------------------------- wide keys

def _two_key_batch(lo, hi):
    """Writes on lo, on hi, and on both: the message's keys span hi - lo; the last fragment has two keys."""
    keys = [[lo], [hi], [lo], [hi], [lo, hi], [lo, hi]]
    return hand_batch([W.WRITE] * 6, [W.PREACCEPTED] * 6, keys)


@pytest.mark.parametrize("slots", [BITMAP, LIST])
@pytest.mark.parametrize("lo,span,wide", [(1 << 31, 0xFFFFFFFF, False), (1 << 31, 1 << 32, True),
                                          ((1 << 63) - 5, (1 << 32) + 9, True)])
def test_wide_key(lo, span, wide, slots):
    """A key span of exactly 0xFFFFFFFF still fits u32 offsets, 2^32 does not; u64 codes on both sides of 2^63."""
    b = _two_key_batch(lo, lo + span)
    gidx = np.arange(b.n_txn, dtype=np.uint32)
    res, _, expect = run_one(b, gidx, b.n_txn if slots == BITMAP else 4096)
    forms, _, _ = H.check_case(res, expect, f"span {span:#x}")
    assert forms == {(0, 0): (slots, False, wide)}
    assert int(res.ref[0][0]["keys"].max()) - int(res.ref[0][0]["keys"].min()) == span


# ---------------------------------------------------------------- wide counts

HOT = 1 << 30


def _pad(n_pairs):
    """Ordinary conflicting txns: pairs of writes on a key of their own, the second depending on the first"""
    return [[HOT + 1000 + j // 2] for j in range(2 * n_pairs)]


def _closed_reads(R, n_pairs, two_keys):
    """R APPLIED reads of a hot key (two_keys: alternating between two keys 2^32 apart) and the txn that closes them,
    on every hot key, whose one fragment lists the R reads. For 65,535 TxnIds to fit u16 counts their varints must take
    65,535 bytes too, one each, so the first TxnId has to lie within 64 of the fragment's own txn: a closing write after
    the reads would spend three bytes on it (R + 2 in all, u32 counts from R = 65,534 on). So the closing txn is the
    first by TxnId, PREACCEPTED with an executeAt after the last read (its first TxnId is the next txn, one byte), and
    a sync point, not a write: it witnesses reads as a write does, but reads do not witness it and stay without deps.
    The largest of (nk, nv, bytes) is then exactly R. After them n_pairs pairs of padding writes."""
    hot = [HOT, HOT + (1 << 32)] if two_keys else [HOT]
    keys = [hot] + [[hot[i % len(hot)]] for i in range(R)] + _pad(n_pairs)
    kind = [W.SYNC_POINT] + [W.READ] * R + [W.WRITE] * (2 * n_pairs)
    status = [W.PREACCEPTED] + [W.APPLIED] * R + [W.PREACCEPTED] * (2 * n_pairs)
    return hand_batch(kind, status, keys, exe_after={0: R})


@pytest.mark.parametrize("slots", [LIST, BITMAP])
@pytest.mark.parametrize("R,two_keys", [(65535, False), (65536, False), (65535, True), (65536, True)])
def test_wide_count(R, two_keys, slots):
    """65,535 TxnIds in one fragment still fit u16 counts, 65,536 do not; with two keys the fragment carries a 2 x R
    key-bit matrix (131K bits) and, the keys lying 2^32 apart, u64 keys. List form: the fragment alone; bitmap form:
    padded with conflicting txns until the fragments are at least ceil(G / 32)."""
    n_pairs = 0 if slots == LIST else 2400
    b = _closed_reads(R, n_pairs, two_keys)
    # the oracle's scan of a hot key is quadratic in R: it is asked for every txn but the reads, whose groups are
    # expected empty (nothing they witness precedes them), which the merged view is then held to
    res, full, expect = run_one(b, None, b.n_txn, queries=np.r_[0, R + 1:b.n_txn])
    assert int(np.diff(full.u_off.astype(np.int64)).max()) == R
    hdr = res.ref[0][0]["hdr"].reshape(-1, 4)
    assert hdr[0].tolist() == [0, 2 if two_keys else 1, R, (2 if two_keys else 1) + R]
    assert len(hdr) == 1 + n_pairs and (slots == LIST or len(hdr) >= (b.n_txn + 31) // 32)
    forms, lens, signs = H.check_case(res, expect, f"R {R}")
    assert forms == {(0, 0): (slots, R > 65535, two_keys)}
    assert 1 in signs


@pytest.mark.parametrize("slots", [LIST, BITMAP])
def test_wide_count_by_bytes(slots):
    """40,000 reads closed by a PREACCEPTED write, the store's txns 129 global txns apart: every gap needs a two-byte
    varint, so nk and nv fit u16 and the TxnId bytes (80,000) do not. The bitmap form takes as many padding fragments
    as the 5.5M-slot bitmap has words."""
    R = 40000
    n_pairs = 0 if slots == LIST else 172100
    keys = _pad(n_pairs) + [[HOT]] * (R + 1)
    n = len(keys)
    b = hand_batch([W.WRITE] * (2 * n_pairs) + [W.READ] * R + [W.WRITE],
                   [W.PREACCEPTED] * (2 * n_pairs) + [W.APPLIED] * R + [W.PREACCEPTED], keys)
    gidx = np.concatenate([np.arange(2 * n_pairs), 2 * n_pairs + 129 * np.arange(R + 1)]).astype(np.uint32)
    n_global = int(gidx[-1]) + 1
    assert n_global <= 1 << 23
    res, full, expect = run_one(b, gidx, n_global, queries=np.r_[0:2 * n_pairs, n - 1])   # (as in test_wide_count)
    assert int(np.diff(full.u_off.astype(np.int64)).max()) == R
    hdr = res.ref[0][0]["hdr"].reshape(-1, 4)
    assert hdr[-1].tolist() == [n_global - 1, 1, R, 1 + R] and len(hdr) == 1 + n_pairs
    assert slots == LIST or len(hdr) >= (n_global + 31) // 32
    assert int(hdr[:, 1:3].max()) <= 65535
    forms, lens, _ = H.check_case(res, expect, "bytes only")
    assert forms == {(0, 0): (slots, True, False)}
    assert 2 in lens


# ---------------------------------------------------------------- varint widths

def test_varint_widths():
    """Writes on one key placed so that the gap codes are 127 | 128, 16383 | 16384 and 2097151 | 2097152 (one to four
    bytes), and pairs on other keys whose first value is 64 below and 64 above the fragment's txn (zigzag 127 | 128).
    Five-byte varints need gaps of 2^28 global txns, and acc_shard_pack allocates eight u64 arrays of n_global entries:
    gigabytes of scratch, so they stay untested."""
    codes = [127, 128, 16383, 16384, 2097151, 2097152]
    chain = np.concatenate([[0], np.cumsum(np.array(codes) + 1)]) + 1000
    place = {int(g): [HOT] for g in chain}
    place[int(chain[-1]) + 5] = [HOT]                  # the txn that lists the whole chain
    place[10], place[74] = [HOT + 1], [HOT + 1]        # 74 depends on 10: 64 below
    place[200], place[264] = [HOT + 2], [HOT + 2]      # 200 executes after 264 and depends on it: 64 above
    g = np.array(sorted(place), dtype=np.uint32)
    at = {int(x): i for i, x in enumerate(g)}
    b = hand_batch([W.WRITE] * len(g), [W.ACCEPTED if x == 200 else W.PREACCEPTED for x in g], [place[int(x)] for x in g],
                   exe_after={at[200]: at[264]})
    n_global = int(g[-1]) + 1
    assert 1 << 21 < n_global <= 1 << 23
    res, _, expect = run_one(b, g, n_global)
    forms, lens, signs = H.check_case(res, expect, "varint widths")
    assert forms == {(0, 0): (LIST, False, False)}
    ref = res.ref[0][0]
    hdr = ref["hdr"].reshape(-1, 4)
    assert hdr[-1].tolist()[:3] == [n_global - 1, 1, len(chain)]
    last = ref["vals"][-len(chain):].astype(np.int64)
    assert (np.diff(last) - 1).tolist() == codes
    _, delta = H.ref_varint_lens(ref)
    assert {-64, 64} <= set(delta.tolist())
    assert {1, 2, 3, 4} <= lens and 5 not in lens


# ---------------------------------------------------------------- sources of different forms at one receiver

STORE_SPAN = 1 << 20


def _stores_batch(counts, seed):
    """counts[s] writes on 16 keys of store s (keys [s, s + 1) * 2^20), interleaved in a seeded order: every write
    but the first of its key has a fragment. Returns (batch, bounds)."""
    world = len(counts)
    owner = np.repeat(np.arange(world), counts)
    owner = owner[np.argsort(W.stream(seed, 1, len(owner)), kind="stable")]
    seen = [0] * world
    keys = []
    for s in owner.tolist():
        keys.append([s * STORE_SPAN + 7 * (seen[s] % 16)])
        seen[s] += 1
    n = len(keys)
    b = hand_batch([W.WRITE] * n, [W.PREACCEPTED] * n, keys)
    return b, np.arange(world + 1, dtype=np.uint64) * np.uint64(STORE_SPAN)


@pytest.mark.parametrize("counts,order", [
    ((1500, 40), (BITMAP, LIST)),            # 24 fragments of store 1 against bitmaps of 25 words: a list wherever they go
    ((40, 1500), (LIST, BITMAP)),
    ((0, 1500), (EMPTY, BITMAP)),            # store 0 has no txn at all
    ((1500, 0, 30), (BITMAP, EMPTY, LIST)),  # 14 fragments against 17 words
    ((40, 48), (LIST, LIST)),                # padded to 4096 global txns below: no bitmap word at any receiver
    ((16, 16), (EMPTY, EMPTY)),              # one write per key: no txn has deps, F = 0 everywhere
])
def test_mixed_forms(counts, order):
    """Worlds 2 and 3, store-local batches with hand-set key bounds: the per-source forms at some receiver, in source
    order, are the ones the case names."""
    import oracle
    from accord_amd import sharded as S
    world = len(counts)
    b, bounds = _stores_batch(counts, 0xF0 + sum(counts))
    if order == (LIST, LIST):   # keyless txns up to 4096: G = 2048, lists of fewer than 64 slots
        n = b.n_txn
        b = hand_batch([W.WRITE] * 4096, [W.PREACCEPTED] * 4096,
                       [[int(b.key_code[i])] if i < n else [] for i in range(4096)])
    stores = [H.Store(*S.store_batch(b, bounds, s)) for s in range(world)]
    assert [st.batch.n_txn for st in stores] == list(counts)
    res = H.run_world(stores, b.n_txn)
    full = oracle.keydeps_batch(b)
    forms, _, _ = H.check_case(res, [S.home_result_from_full(full, b, r, world) for r in range(world)], str(order))
    seen = [tuple(forms[(s, d)][0] for s in range(world)) for d in range(world)]
    assert order in seen, seen
    assert all(f[1:] == (False, False) for f in forms.values())


# ---------------------------------------------------------------- acc_partial_deps_reduce

def test_partial_deps_reduce_key_half():
    """The key half of acc_partial_deps_reduce travels in the same wire form beside the range streams: world 1
    loopback over a mixed batch, its message cut out of the peer block by the announced size."""
    import torch
    import test_partial_reduce_gpu as P
    from accord_amd import _lib as L
    from accord_amd import sharded as S
    rb = P._batch(0x7D74, 6000)
    want_key, _ = P._expected(rb, 1, 0)
    sub, gidx = S.store_range_batch(rb, P._bounds(rb, 1), 0)
    keep = []

    def reduce(rk, store):
        rbi = rk.ctx.range_batch_in(sub, keep)
        rk.ctx.partial_deps_batch_raw(rbi)
        bi = L.BatchIn(rbi.n_txn, rbi.mem, rbi.n_pairs, rbi.txn_id, rbi.execute_at, rbi.status, rbi.key_off, rbi.key_code)
        g = torch.from_numpy(gidx.astype(np.int32))
        bufs, counts = S.shard_pack(rk.ctx, bi, 1, rk.dev, g)
        ref = [dict(hdr=bufs["hdr"].cpu().numpy().view(np.uint32), keys=bufs["keys"].cpu().numpy().view(np.uint64),
                    vals=bufs["vals"].cpu().numpy().view(np.uint32), k2v=bufs["k2v"].cpu().numpy())]
        rk.calls.clear()
        kv, rv = S.partial_deps_reduce(rk.ctx, rk.comm, rbi, rb.n_txn, gidx.astype(np.uint32))
        return ref, S.merged_to_host(rk.ctx, kv)

    res = H.run_world([None], rb.n_txn, reduce=reduce)
    assert len(res.msg[(0, 0)]) > M.HEADER_BYTES
    forms, _, _ = H.check_case(res, [want_key], "partial deps")
    assert forms == {(0, 0): (BITMAP, False, False)}


# ---------------------------------------------------------------- argument and header checks

def _good(rk, b, full, n_global, gidx):
    """A reduce that must succeed on rk, through the four comparisons"""
    res = H.Result(1, n_global)
    res.ref[0] = rk.load(H.Store(b, gidx))
    res.merged[0] = rk.reduce(n_global)
    res.stats[0], res.msg = rk.ctx.stats(), {(0, d): m for d, m in rk.messages().items()}
    return H.check_case(res, [H.expected_home(full, b, gidx, n_global, 0, 1)], "good reduce")


def test_n_global_below_placement():
    """A placement that reaches n_global is refused before anything is packed or sent (it used to write past the slot
    bitmap); one more global txn and the reduce passes."""
    from accord_amd.deps import IllegalArgumentException
    b, full = small()
    gidx = (3 * np.arange(b.n_txn) + 2).astype(np.uint32)
    last = int(gidx[-1])
    rk = H.Rank(1, 0, H.loopback())
    try:
        rk.load(H.Store(b, gidx))
        with pytest.raises(IllegalArgumentException):
            rk.reduce(last)
        assert rk.calls == []
        _good(rk, b, full, last + 1, gidx)
    finally:
        rk.close()


def test_n_global_below_placement_partial_deps():
    import test_partial_reduce_gpu as P
    from accord_amd import sharded as S
    from accord_amd.deps import Context, IllegalArgumentException
    rb = P._batch(0x7D75, 3000)
    sub, gidx = S.store_range_batch(rb, P._bounds(rb, 1), 0)
    assert int(gidx[-1]) + 1 == rb.n_txn, "the batch's last txn lies in the only store"
    calls = []
    with Context(0) as ctx:
        comm = S.Comm.host_fn(ctx, 1, 0, lambda send, sb, rb_: calls.append(len(send)) or send)
        keep = []
        rbi = ctx.range_batch_in(sub, keep)
        ctx.partial_deps_batch_raw(rbi)
        with pytest.raises(IllegalArgumentException):
            S.partial_deps_reduce(ctx, comm, rbi, int(gidx[-1]), gidx.astype(np.uint32))
        assert calls == []
        kv, _ = S.partial_deps_reduce(ctx, comm, rbi, int(gidx[-1]) + 1, gidx.astype(np.uint32))
        key = S.merged_to_host(ctx, kv)
        comm.close()
    assert len(calls) == 2
    want, _ = P._expected(rb, 1, 0)
    for f in H.MERGE_FIELDS:
        np.testing.assert_array_equal(key[f], want[f], err_msg=f)


def _word(msg, i, value):
    out = bytearray(msg)
    out[4 * i:4 * i + 4] = int(value).to_bytes(4, "little")
    return bytes(out)


def _header_word(i, change):
    """Tamper with header word i of the received message (the data exchange is call 1)"""
    def tamper(call, data):
        if call != 1:
            return data
        return _word(data, i, change(int.from_bytes(data[4 * i:4 * i + 4], "little")))
    return tamper


@pytest.mark.parametrize("name,tamper", [
    ("magic", _header_word(0, lambda v: v ^ 0x100)),
    ("unknown flag", _header_word(1, lambda v: v | 8)),
    ("count width flag", _header_word(1, lambda v: v ^ M.F_WIDE_CNT)),
    ("G", _header_word(3, lambda v: v + 1)),
    ("slot section size", _header_word(6, lambda v: v + 8)),
    ("short message", "short"),
    ("size differs from header", "longer"),
])
def test_header_rejected(name, tamper):
    """One header field wrong per case, or a lie in the size exchange: ACC_E_STATE from the host-side checks, before
    any kernel reads the message; the context then runs a good reduce."""
    from accord_amd.deps import IllegalStateException
    b, full = small()
    state = {"on": True, "calls": 0}

    def counted(_, data):
        call = state["calls"]
        state["calls"] += 1
        if not state["on"]:
            return data
        if tamper == "short":      # 56 bytes announced and delivered: shorter than a header
            return (56).to_bytes(8, "little") if call == 0 else data[:56]
        if tamper == "longer":     # 8 bytes more than the header accounts for (zeros, as padding would be)
            return (int.from_bytes(data, "little") + 8).to_bytes(8, "little") if call == 0 else data + bytes(8)
        return tamper(call, data)

    rk = H.Rank(1, 0, H.loopback(counted))
    try:
        rk.load(H.Store(b, None))
        with pytest.raises(IllegalStateException):
            rk.reduce(b.n_txn)
        assert state["calls"] == 2, "rejected on the received message, not earlier"
        state["on"] = False
        _good(rk, b, full, b.n_txn, None)
    finally:
        rk.close()
