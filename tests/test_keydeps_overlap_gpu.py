"""GPU parity of the CFK build's side lane: a TxnId-ordered batch whose pair sort packs its keys (modes 3, 4) runs the
sorted-batch dictionary beside the pair sort and makes the bumped committed (segment, executeAt) order from the txn
side (csrc/keydeps.hip: build_cfk, bc_from_txns). Every case compares all six result arrays with the oracle.

executeAts are built the way workload.keydeps_txn_columns builds them (bump <= 1000, exec node 1000 + i % 1024), so
no executeAt equals another timestamp and the batches take the run-based path.
"""
import numpy as np
import pytest

import rd_cases
from accord_amd import workload as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


def assert_same(gpu, orc, label=""):
    for name in ("arena_off", "kd_off", "u_off", "arena", "key_idx", "dep_txn"):
        np.testing.assert_array_equal(getattr(gpu, name), getattr(orc, name), err_msg=f"{label} {name}")


def with_columns(b, kind, status, bump, bump_by):
    """b's keys under TxnIds of the given kinds, statuses, and executeAt = TxnId + bump_by where bump is set."""
    n = b.n_txn
    i = np.arange(n, dtype=np.int64)
    kind = np.asarray(kind, dtype=np.int64)
    t_msb, t_lsb, t_node = W.encode_ts(np.ones(n), i + 1, kind << 1, 1 + (i % 8))
    e_msb, e_lsb, e_node = W.encode_ts(np.ones(n), i + 1 + np.asarray(bump_by, dtype=np.int64), np.zeros(n), 1000 + (i % 1024))
    return W.Batch(t_msb, t_lsb, t_node, np.where(bump, e_msb, t_msb).astype(np.uint64),
                   np.where(bump, e_lsb, t_lsb).astype(np.uint64), np.where(bump, e_node, t_node).astype(np.int32),
                   np.asarray(status, dtype=np.uint8), b.key_off, b.key_code)


def kinds_of(b):
    return ((b.txn_lsb >> np.uint64(1)) & np.uint64(7)).astype(np.int64)


def truncate_keys(b, counts):
    """Keep the first counts[t] keys of every txn (rows stay sorted and distinct)."""
    keep = np.concatenate([np.arange(int(b.key_off[t]), int(b.key_off[t]) + int(c)) for t, c in enumerate(counts)]
                          + [np.zeros(0, np.int64)]).astype(np.int64)
    b.key_code = b.key_code[keep]
    b.key_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return b


def nbc_of(b):
    """Entries of the bumped committed list: keys of txns that are committed, of a witnessed kind, executeAt != TxnId."""
    bumped = (b.txn_msb != b.exe_msb) | (b.txn_lsb != b.exe_lsb) | (b.txn_node != b.exe_node)
    com = (b.status >= W.COMMITTED) & (b.status <= W.APPLIED)
    cls = np.isin(kinds_of(b), [W.READ, W.WRITE, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT])
    return int(np.diff(b.key_off.astype(np.int64))[bumped & com & cls].sum())


def run_overlapped(ctx, b, o, label, want_nbc=None):
    if want_nbc is not None:
        assert nbc_of(b) == want_nbc
    g = ctx.calculate_partial_deps(b)
    st = ctx.stats()
    assert st["keydeps.build_overlap"] == 1 and st["keydeps.pair_sort_mode"] in (3, 4), st
    assert st["keydeps.path_replay"] == 0
    assert (st["keydeps.bc_sort_passes"] >= 1) == (nbc_of(b) > 0)
    assert g.total_edges == o.total_edges
    assert_same(g, o, label)


_CASES = {}


def case(name):
    """(batch, oracle result), built once and left unchanged."""
    import oracle
    if name in _CASES:
        return _CASES[name]
    if name == "heavy":
        # 3,000 txns x 4 keys over 40 keys, half of the committed txns bumped by up to 1000: executeAt order inside a
        # segment is far from TxnId order and many queries take M from the bumped list
        b = W.keydeps_batch(3000, 4, 40, 0xB0B, "uniform", status_model="model", window=600)
        rng = np.random.RandomState(5)
        com = (b.status >= W.COMMITTED) & (b.status <= W.APPLIED)
        b = with_columns(b, kinds_of(b), b.status, com & (rng.rand(b.n_txn) < 0.5), 1 + rng.randint(0, 1000, b.n_txn))
    elif name == "edges":
        # one batch with: bumped ACCEPTED txns, bumped committed EphemeralReads (no predicate witnesses them), bumped
        # committed txns without keys and empty txns generally, bumped committed SyncPoints of both kinds
        b = W.keydeps_batch(2500, 4, 60, 0xED6E, "uniform", status_model="model", window=700)
        rng = np.random.RandomState(9)
        n = b.n_txn
        kind = rng.choice([W.READ, W.WRITE, W.EPHEMERAL_READ, W.SYNC_POINT, W.EXCLUSIVE_SYNC_POINT], size=n,
                          p=[0.3, 0.35, 0.15, 0.1, 0.1])
        status = b.status.copy()
        bump = (status >= W.ACCEPTED) & (status <= W.APPLIED) & (rng.rand(n) < 0.4)
        counts = rng.choice([0, 1, 2, 3, 4], size=n, p=[0.15, 0.1, 0.15, 0.2, 0.4])
        b = truncate_keys(with_columns(b, kind, status, bump, 1 + rng.randint(0, 1000, n)), counts)
        com = (status >= W.COMMITTED) & (status <= W.APPLIED)
        assert (bump & (status == W.ACCEPTED)).sum() > 20
        assert (bump & com & (kind == W.EPHEMERAL_READ)).sum() > 20
        assert (bump & com & (counts == 0)).sum() > 20
        assert (bump & com & (kind == W.SYNC_POINT)).sum() > 10 and (bump & com & (kind == W.EXCLUSIVE_SYNC_POINT)).sum() > 10
    elif name == "preaccepted":
        b = W.keydeps_batch(1500, 4, 100, 0x9A, "uniform", status_model="preaccepted")
    elif name == "nobump":
        b = W.keydeps_batch(1500, 4, 100, 0x9B, "uniform", status_model="model", window=300)
        b = with_columns(b, kinds_of(b), b.status, np.zeros(b.n_txn, bool), np.ones(b.n_txn))
    elif name.startswith("nbc"):
        # exactly that many bumped committed entries: full 4-key txns and one txn cut to the remainder
        target = int(name[3:])
        b = W.keydeps_batch(1200, 4, 150, 0x1000 + target, "uniform", status_model="model", window=200)
        rng = np.random.RandomState(target)
        com = np.where((b.status >= W.COMMITTED) & (b.status <= W.APPLIED))[0]
        pick = rng.permutation(com)[:(target + 3) // 4]
        bump = np.zeros(b.n_txn, bool)
        bump[pick] = True
        counts = np.full(b.n_txn, 4)
        if target % 4:
            counts[pick[-1]] = target % 4
        b = truncate_keys(with_columns(b, kinds_of(b), b.status, bump, 1 + rng.randint(0, 1000, b.n_txn)), counts)
    elif name == "large":
        # more than 262,144 bumped committed entries: the sort's large tiles
        b = W.keydeps_batch(100_000, 8, 60_000, 0x1A26E, "uniform", status_model="model", window=2000)
        rng = np.random.RandomState(21)
        com = (b.status >= W.COMMITTED) & (b.status <= W.APPLIED)
        b = with_columns(b, kinds_of(b), b.status, com & (rng.rand(b.n_txn) < 0.5), 1 + rng.randint(0, 1000, b.n_txn))
        assert nbc_of(b) > 262_144
    elif name == "unsorted":
        b = case("heavy")[0].permuted(np.random.RandomState(13).permutation(3000))
    elif name == "ties":
        h = case("heavy")[0]
        b = W.Batch(*[a.copy() for a in (h.txn_msb, h.txn_lsb, h.txn_node, h.exe_msb, h.exe_lsb, h.exe_node, h.status,
                                         h.key_off, h.key_code)])
        com = np.where((b.status >= W.COMMITTED) & (b.status <= W.APPLIED))[0][:2]
        b.exe_msb[com] = b.exe_msb[com[0]]
        b.exe_lsb[com] = b.txn_lsb[com].max() + (np.uint64(7) << np.uint64(16))
        b.exe_node[com] = 77
    else:
        raise KeyError(name)
    _CASES[name] = (b, oracle.keydeps_batch(b))
    return _CASES[name]


def test_heavy_bumping_on_few_keys(ctx):
    b, o = case("heavy")
    run_overlapped(ctx, b, o, "heavy")


def test_predicate_edges(ctx):
    b, o = case("edges")
    run_overlapped(ctx, b, o, "edges")


@pytest.mark.parametrize("name", ["preaccepted", "nobump"])
def test_no_bumped_committed(ctx, name):
    b, o = case(name)
    run_overlapped(ctx, b, o, name, want_nbc=0)


@pytest.mark.parametrize("target", [1, 1023, 1024, 1025])
def test_bumped_committed_sizes(ctx, target):
    """One entry, and one small-sort tile of 1,024 entries +- 1."""
    b, o = case(f"nbc{target}")
    run_overlapped(ctx, b, o, f"nbc {target}", want_nbc=target)


def test_large_tile_sort(ctx):
    b, o = case("large")
    run_overlapped(ctx, b, o, "large")


def test_context_reuse():
    """Large, small, large on one context (the side lane's status words and their parity, the shared g words), then the
    fallback (an unsorted batch), the replay path (an executeAt tie), a RangeDeps call, and the first batch again."""
    import oracle
    from accord_amd.deps import Context
    large, small = case("large"), case("nbc1025")
    with Context(0) as c:
        for rnd, (b, o) in enumerate([large, small, large, case("heavy")]):
            run_overlapped(c, b, o, f"reuse round {rnd}")
        b, o = case("unsorted")
        g = c.calculate_partial_deps(b)
        assert c.stats()["keydeps.build_overlap"] == 0 and c.stats()["keydeps.pair_sort_mode"] == 1
        assert_same(g, o, "unsorted")
        b, o = case("ties")
        g = c.calculate_partial_deps(b)
        assert c.stats()["keydeps.path_replay"] == 1
        assert_same(g, o, "ties")
        rb = rd_cases.dense(200, n=2000, end_inclusive=1, ranges_per_txn=1)
        gr, orr = c.calculate_partial_range_deps(rb), oracle.rangedeps_batch(rb)
        assert orr.total_edges > 0
        for name in ("rng_start", "rng_end", "arena_off", "arena", "rd_off", "range_id", "u_off", "dep_txn"):
            np.testing.assert_array_equal(getattr(gr, name), getattr(orr, name), err_msg=f"rangedeps {name}")
        run_overlapped(c, large[0], large[1], "reuse: first batch again")
        run_overlapped(c, small[0], small[1], "reuse: small again")
