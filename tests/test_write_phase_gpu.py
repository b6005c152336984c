"""GPU parity of the KeyDeps write phase with few blocks and long per-block lists.

The window tier (k_v2_write_win) is a persistent grid, one txn per block at a time, and stages the next list item's
records and offsets while it works on the current txn. Context(tier_grid_max=), bits 16..31 of acc_opts.flags, caps
that grid, so a few thousand big txns give every block many iterations: list longer than the grid, one block walking the whole list, a list length that
the grid does not divide, a list shorter than the grid, a txn passed on to the sorting tier in the middle of a block's
list, sparse spans between dense ones. Every txn's three arrays are compared with the oracle on the full batch and,
where the window tier runs, with the sorting tiers alone. The RUNS stream pass (stream txns with a run record) gets its
own batches.
"""
import numpy as np
import pytest

from accord_amd import workload as W

pytestmark = pytest.mark.gpu

HOT = 1 << 30   # a key outside every sampled key space


def assert_same(gpu, orc, label=""):
    for f in ("arena_off", "kd_off", "u_off", "arena", "key_idx", "dep_txn"):
        np.testing.assert_array_equal(getattr(gpu, f), getattr(orc, f), err_msg=f"{label} {f}")


def entries(o):
    """Dependency entries per txn, from the oracle's offsets (arena = one header int per key with deps + the entries)."""
    return np.diff(o.arena_off.astype(np.int64)) - np.diff(o.kd_off.astype(np.int64))


def prefix(b, n):
    """The batch's first n txns."""
    p = int(b.key_off[n])
    return W.Batch(b.txn_msb[:n].copy(), b.txn_lsb[:n].copy(), b.txn_node[:n].copy(), b.exe_msb[:n].copy(),
                   b.exe_lsb[:n].copy(), b.exe_node[:n].copy(), b.status[:n].copy(), b.key_off[:n + 1].copy(),
                   b.key_code[:p].copy(), dict(b.meta))


def with_key_counts(b, counts):
    """The batch with txn t keeping its first counts[t] keys."""
    keep = np.concatenate([np.arange(int(b.key_off[t]), int(b.key_off[t]) + int(c)) for t, c in enumerate(counts)])
    b.key_code = b.key_code[keep.astype(np.int64)]
    b.key_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return b


def put_key(b, idx, key):
    """Key `key` in place of the first key of the txns idx (a txn's keys stay sorted)."""
    code = W.int_key_code(np.array([key]))[0]
    for t in idx:
        lo, hi = int(b.key_off[t]), int(b.key_off[t + 1])
        b.key_code[lo] = code
        b.key_code[lo:hi] = np.sort(b.key_code[lo:hi])


def set_kind(b, idx, kind, status):
    b.txn_lsb[idx] = (b.txn_lsb[idx] & ~np.uint64(0xE)) | np.uint64(kind << 1)
    b.exe_msb[idx], b.exe_lsb[idx], b.exe_node[idx] = b.txn_msb[idx], b.txn_lsb[idx], b.txn_node[idx]
    b.status[idx] = status


_CASES = {}


def case(name):
    """(batch, oracle result), built once and shared (never modified by a test)."""
    if name not in _CASES:
        import oracle
        b = _BUILD[name]()
        _CASES[name] = (b, oracle.keydeps_batch(b))
    return _CASES[name]


def _win_uniform():
    return W.keydeps_batch(12_000, 4, 60, 0xA11, "uniform", status_model="model", window=3000)


def _win_zipf():
    return W.keydeps_batch(8_000, 8, 200, 0xA12, "zipf", 0.99, status_model="model", window=2600)


def _one_big():
    """The first 9,376 txns of _win_uniform: only the last txns of the uncommitted window reach 128 entries, here
    exactly one (asserted by its test): a window-tier list of one."""
    return prefix(_win_uniform(), 9_376)


def _few_big():
    """... and the first 9,440: a handful of big txns, a list shorter than a grid cap of 64."""
    return prefix(_win_uniform(), 9_440)


def _pass_on():
    """A window batch with a hot key of APPLIED Reads in its first 12,000 txns closed by three PREACCEPTED Writes near
    the end: 1,200 of each Write's entries lie more than 16,384 ranks below it, more than the window tier's list below
    its span holds, so the tier passes the txn on to the sorting tier and goes on with its list."""
    b = W.keydeps_batch(30_000, 4, 60, 0xA15, "uniform", status_model="model", window=3000)
    hot = np.arange(0, 12_000, 10)
    put_key(b, hot, HOT)
    set_kind(b, hot, W.READ, W.APPLIED)
    last = np.array([28_500, 29_200, 29_900])
    put_key(b, last, HOT)
    set_kind(b, last, W.WRITE, W.PREACCEPTED)
    return b


SPARSE_T = np.array([9_400, 9_900, 10_400, 10_900, 11_400, 11_900])


def _sparse_dense():
    """_win_uniform with a cold key: 160 APPLIED Reads spread over the first 8,000 txns and six single-key PREACCEPTED
    Writes in the window. A Write's ~160 entries span ~10,000 ranks (fewer than one entry per 16 ranks): the window
    tier's sorted-list-only path, between the dense txns of the same block."""
    b = _win_uniform()
    counts = np.full(b.n_txn, 4)
    counts[SPARSE_T] = 1
    b = with_key_counts(b, counts)
    cold = np.arange(0, 8_000, 50)
    put_key(b, cold, HOT)
    set_kind(b, cold, W.READ, W.APPLIED)
    put_key(b, SPARSE_T, HOT)
    set_kind(b, SPARSE_T, W.WRITE, W.PREACCEPTED)
    return b


def _win16():
    return W.keydeps_batch(10_000, 12, 3_000, 0xB23, "zipf", 0.99, status_model="model", window=2500)


def _runs_zipf():
    return W.keydeps_batch(6_000, 8, 400, 0xA14, "zipf", 0.99, status_model="model", window=500)


def _runs_uniform():
    return W.keydeps_batch(6_000, 4, 100, 0xA13, "uniform", status_model="model", window=600)


def _runs_ragged():
    """_runs_zipf with 0-8 keys per txn: groups with fewer than 16 active lanes, waves whose groups differ in run keys."""
    b = _runs_zipf()
    return with_key_counts(b, np.random.RandomState(5).randint(0, 9, size=b.n_txn))


_BUILD = dict(win_uniform=_win_uniform, win_zipf=_win_zipf, one_big=_one_big, few_big=_few_big, pass_on=_pass_on,
              sparse_dense=_sparse_dense, win16=_win16, runs_zipf=_runs_zipf, runs_uniform=_runs_uniform,
              runs_ragged=_runs_ragged)

_SORTED = {}


def sorting_tiers(name):
    """The batch through the sorting tiers alone (no window tier), once per case."""
    if name not in _SORTED:
        from accord_amd.deps import Context
        with Context(0, no_window_tier=True) as c:
            _SORTED[name] = c.calculate_partial_deps(case(name)[0])
    return _SORTED[name]


def run(name, tier_grid_max):
    from accord_amd.deps import Context
    b, o = case(name)
    with Context(0, tier_grid_max=tier_grid_max) as c:
        g = c.calculate_partial_deps(b)
        st = c.stats()
    assert_same(g, o, f"{name} grid {tier_grid_max} vs oracle")
    return g, st


@pytest.mark.parametrize("tier_grid_max", [0, 1, 3])
@pytest.mark.parametrize("name", ["win_uniform", "win_zipf"])
def test_window_many_iterations_per_block(name, tier_grid_max):
    """List longer than the grid (0: the default cap), one block walking the whole list (1), a list length the grid does
    not divide (3)."""
    g, st = run(name, tier_grid_max)
    assert st["keydeps.window_txns"] > 0
    if name == "win_zipf" and tier_grid_max == 3:
        assert st["keydeps.window_txns"] % 3 != 0
    assert_same(g, sorting_tiers(name), f"{name} grid {tier_grid_max} vs sorting tiers")


def test_window_list_of_one():
    b, o = case("one_big")
    assert int((entries(o) > 128).sum()) == 1
    g, st = run("one_big", 0)
    assert st["keydeps.window_txns"] == 1
    assert_same(g, sorting_tiers("one_big"), "list of one vs sorting tiers")


@pytest.mark.parametrize("tier_grid_max", [0, 64])
def test_window_list_shorter_than_grid_cap(tier_grid_max):
    nbig = int((entries(case("few_big")[1]) > 128).sum())
    assert 2 <= nbig < 64
    g, st = run("few_big", tier_grid_max)
    assert st["keydeps.window_txns"] == nbig
    assert_same(g, sorting_tiers("few_big"), "short list vs sorting tiers")


def test_window_pass_on_inside_a_blocks_list():
    """The passed-on txns sit in the middle of the one block's list: the txns after them must be exact (the staged
    buffers rotate on the pass-on path too)."""
    g, st = run("pass_on", 1)
    assert st["keydeps.window_txns"] > 0
    assert st["keydeps.big_txns"] + st["keydeps.huge_txns"] > 0
    assert_same(g, sorting_tiers("pass_on"), "pass-on vs sorting tiers")


def test_window_sparse_between_dense_spans():
    b, o = case("sparse_dense")
    e = entries(o)
    for t in SPARSE_T:
        deps = o.dep_txn[int(o.u_off[t]):int(o.u_off[t + 1])]
        # big (window tier), within the list below the span, fewer than one entry per 16 ranks below executeAt
        assert 128 < e[t] <= 1024 and int(t) - int(deps.min()) > 16 * int(e[t])
    assert int((e[SPARSE_T[0]:] > 128).sum()) > 10 * len(SPARSE_T)   # dense window txns around them
    g, st = run("sparse_dense", 1)
    assert st["keydeps.window_txns"] > 0
    assert_same(g, sorting_tiers("sparse_dense"), "sparse / dense vs sorting tiers")


@pytest.mark.parametrize("tier_grid_max", [0, 1])
def test_window_16_key_instance(tier_grid_max):
    g, st = run("win16", tier_grid_max)
    assert st["keydeps.window_txns"] > 0
    assert_same(g, sorting_tiers("win16"), f"12 keys grid {tier_grid_max} vs sorting tiers")


@pytest.mark.parametrize("name", ["runs_zipf", "runs_uniform", "runs_ragged"])
def test_stream_pass_with_run_records(name):
    g, st = run(name, 0)
    assert st["keydeps.stream_run_txns"] > 0
