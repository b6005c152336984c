"""GPU parity of KeyDeps with the lean stream pass enqueued ahead of the size read-back.

From a context's second call on, keydeps_runs enqueues the lean stream pass behind the copy of the sizes and waits for
that copy on an event; the side-stream kernels rest on the same event. The pass is handed the capacity of the arena the
context holds and leaves without a store when the batch's P + E is beyond it; the host then grows the arena and runs
the pass in its old place (keydeps.stream_ahead_redo). Context(no_stream_ahead=True) forces the old order. The two txn
lists (big txns, stream txns with a run record) come from one packed flag word per txn, scanned beside the sizes.
Every result is compared with the oracle in all six arrays; the batches follow tests/test_write_phase_gpu.py.

Only a leading share of the pass goes ahead (ACC_AHEAD_DIV, keydeps.hip); the rest follows behind the side-stream
launches from a txn offset that is a multiple of the tile, so every batch here crosses that seam. The count pass ahead
of the build's read-back (keydeps.count_ahead) is not built, so nothing here covers it.

Of the two one-list cases the generator yields "run-record stream txns but no big txn" (a prefix of a uniform batch);
it does not yield "big txns but no run-record stream txn" at this size: a pair passes 15 entries (a run record) long
before a txn's pairs sum past 128 entries, so every batch with a big txn holds run-record stream txns before it.
"""
import numpy as np
import pytest

from accord_amd import workload as W

pytestmark = pytest.mark.gpu

FIELDS = ("arena_off", "kd_off", "u_off", "arena", "key_idx", "dep_txn")


def assert_same(gpu, ref, label=""):
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(gpu, f), getattr(ref, f), err_msg=f"{label} {f}")


def entries(o):
    """Dependency entries per txn, from the oracle's offsets (arena = one header int per key with deps + the entries)."""
    return np.diff(o.arena_off.astype(np.int64)) - np.diff(o.kd_off.astype(np.int64))


def prefix(b, n):
    """The batch's first n txns."""
    p = int(b.key_off[n])
    return W.Batch(b.txn_msb[:n].copy(), b.txn_lsb[:n].copy(), b.txn_node[:n].copy(), b.exe_msb[:n].copy(),
                   b.exe_lsb[:n].copy(), b.exe_node[:n].copy(), b.status[:n].copy(), b.key_off[:n + 1].copy(),
                   b.key_code[:p].copy(), dict(b.meta))


def _zipf():
    return W.keydeps_batch(8_000, 8, 200, 0xA12, "zipf", 0.99, status_model="model", window=2600)


def _sparse():
    """The same n and P, keys uniform over 2^20: a few entries per txn, no big txn, no run record."""
    return W.keydeps_batch(8_000, 8, 1 << 20, 0xA16, "uniform", status_model="model", window=2600)


def _runs_only():
    """The txns of test_write_phase_gpu's runs_uniform batch ahead of its first big txn (txn 5,963)."""
    return prefix(W.keydeps_batch(6_000, 4, 100, 0xA13, "uniform", status_model="model", window=600), 5_963)


_BUILD = dict(zipf=_zipf, sparse=_sparse, runs_only=_runs_only)
_CASES = {}


def case(name):
    """(batch, oracle result), built once and shared (never modified by a test)."""
    if name not in _CASES:
        import oracle
        b = _BUILD[name]()
        _CASES[name] = (b, oracle.keydeps_batch(b))
    return _CASES[name]


def call(ctx, name, label):
    b, o = case(name)
    g = ctx.calculate_partial_deps(b)
    st = ctx.stats()
    assert_same(g, o, f"{name} {label} vs oracle")
    return g, st


def test_all_three_classes_twice_then_forced():
    from accord_amd.deps import Context
    with Context(0) as c:
        g1, st1 = call(c, "zipf", "first call")
        assert st1["keydeps.big_path_txns"] > 0 and st1["keydeps.stream_run_txns"] > 0
        assert st1["keydeps.stream_txns"] > st1["keydeps.stream_run_txns"]   # plain stream txns
        assert st1["keydeps.stream_ahead"] == 0 and st1["keydeps.stream_ahead_redo"] == 0   # no arena yet
        g2, st2 = call(c, "zipf", "second call")
        assert st2["keydeps.stream_ahead"] == 1 and st2["keydeps.stream_ahead_redo"] == 0
        for k in ("keydeps.big_path_txns", "keydeps.stream_run_txns", "keydeps.stream_txns", "keydeps.window_txns"):
            assert st2[k] == st1[k], k
    with Context(0, no_stream_ahead=True) as c:
        call(c, "zipf", "forced, first call")
        g3, st3 = call(c, "zipf", "forced, second call")
        assert st3["keydeps.stream_ahead"] == 0 and st3["keydeps.stream_ahead_redo"] == 0
    assert_same(g3, g2, "forced order vs ahead")


def test_arena_growth_trips_the_guard_once():
    from accord_amd.deps import Context
    (bs, os_), (bz, oz) = case("sparse"), case("zipf")
    assert bs.n_txn == bz.n_txn and bs.n_pairs == bz.n_pairs
    need_s = bs.n_pairs + int(entries(os_).sum())
    need_z = bz.n_pairs + int(entries(oz).sum())
    # a buffer is allocated with half its size as headroom: the second batch's arena is beyond the first call's
    assert 2 * need_z > 3 * need_s
    with Context(0) as c:
        _, st = call(c, "sparse", "first call")
        assert st["keydeps.stream_ahead"] == 0 and st["keydeps.stream_ahead_redo"] == 0
        _, st = call(c, "zipf", "grown")
        assert st["keydeps.stream_ahead_redo"] == 1
        assert st["keydeps.stream_ahead"] == 0   # the pass ran in its old place, on the grown arena
        _, st = call(c, "zipf", "repeat")
        assert st["keydeps.stream_ahead"] == 1 and st["keydeps.stream_ahead_redo"] == 0
        # a smaller batch on the larger arena
        _, st = call(c, "sparse", "smaller again")
        assert st["keydeps.stream_ahead"] == 1 and st["keydeps.stream_ahead_redo"] == 0


def test_no_big_and_no_run_txns():
    from accord_amd.deps import Context
    with Context(0) as c:
        call(c, "sparse", "first call")
        _, st = call(c, "sparse", "second call")
    assert st["keydeps.stream_ahead"] == 1
    assert st["keydeps.big_path_txns"] == 0 and st["keydeps.stream_run_txns"] == 0
    assert st["keydeps.stream_txns"] == case("sparse")[0].n_txn


def test_run_txns_without_big_txns():
    from accord_amd.deps import Context
    b, o = case("runs_only")
    assert int((entries(o) > 128).sum()) == 0
    with Context(0) as c:
        call(c, "runs_only", "first call")
        _, st = call(c, "runs_only", "second call")
    assert st["keydeps.stream_ahead"] == 1
    assert st["keydeps.big_path_txns"] == 0 and st["keydeps.stream_run_txns"] > 0


def test_sparse_compaction_on_the_fast_path():
    """A mixed key / range batch sets cb.opts.sparse (the TxnId compaction over the txns with TxnIds only): its key
    part on a warm context, with the oracle's mixed KeyDeps."""
    import oracle
    import rd_cases
    from accord_amd.deps import Context
    rb = rd_cases.dense(301, n=4000, end_inclusive=1, ranges_per_txn=2)
    o = oracle.keydeps_mixed(rb)
    with Context(0) as c:
        c.calculate_partial_key_deps_mixed(rb)
        g = c.calculate_partial_key_deps_mixed(rb)
        st = c.stats()
    assert st["keydeps.stream_ahead"] == 1
    for f in FIELDS + ("kd_key",):
        np.testing.assert_array_equal(getattr(g, f), getattr(o, f), err_msg=f"mixed {f}")


def test_timing_context():
    from accord_amd.deps import Context
    with Context(0, timing=True) as c:
        call(c, "zipf", "timing, first call")
        c.timing_reset()
        _, st = call(c, "zipf", "timing, second call")
        tm = c.timing()
    assert st["keydeps.stream_ahead"] == 1
    for tag in ("v3_stream", "v3_route", "v2_count"):
        assert tag in tm and tm[tag][1] >= 1, tag
