"""The device fold of the range-command store (k_rc_fold, csrc/rcmd.hip: Ranges.with replayed per command over its
updates in array order) against the independent model of tests/ranges_model.py. No expected value here comes from the
library: the tables are built from ranges_model.fold, and every comparison is exact equality on every field of the
table and on the dictionary.

Each case runs on small integer points and on points spread over the u64 space (2^32 - 1, 2^32, 2^63 - 1, 2^63,
2^64 - 1 among them: the unsigned compares of the device code).
  1. stored (+) update, exhaustive: every ordered pair of the 233 Ranges over seven points as one command each;
  2. the same pairs inside one batch, a command's two updates 54,289 rows apart (the stable rank keeps array order);
  3. folds of three and of four operands, as one batch and with the first operands stored. A command's first operand
     meets no with() (ranges == null), so a chain of three with() results, which is what brings the first scratch
     buffer back into use while the second is read, takes four operands: the triples pin two-step paths, the
     quadruples the three-step ones. The paths are asserted from the model;
  4. long lists (1, 63, 64, 65, 300 ranges a side) on dense points, five-update groups, and neighbouring rows of fully
     interleaved lists whose result fills its scratch exactly;
  5. acc_rcmd_update with ACC_MEM_DEVICE inputs: a store rebuilt from another store's device view."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ranges_model as M
from accord_amd import _lib as L
from accord_amd import workload as W
from accord_amd.deps import RangeCmdStore

pytestmark = pytest.mark.gpu

ERASED = L.ACC_RCMD_ERASED
TABLE_FIELDS = ("msb", "lsb", "node", "flags", "rng_off", "rng_start", "rng_end", "dict_start", "dict_end")
POINT_MAPS = {"small": tuple(range(7)), "wide": M.WIDE_POINTS}


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- building updates and expected tables with numpy

class Pool:
    """A list of Ranges flattened into columns; gather(sel) lays the chosen ones out as update rows."""

    def __init__(self, lists):
        self.lists = lists
        self.len = np.array([len(r) for r in lists], np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.len)]).astype(np.int64)
        self.s = np.array([s for r in lists for s, _ in r], np.uint64)
        self.e = np.array([e for r in lists for _, e in r], np.uint64)

    def gather(self, sel):
        sel = np.asarray(sel, np.int64)
        cnt = self.len[sel]
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        idx = np.repeat(self.off[sel] - off[:-1], cnt) + np.arange(int(off[-1]), dtype=np.int64)
        return off.astype(np.uint32), self.s[idx], self.e[idx]


def txn_ids(n):
    """n range-domain Write TxnIds in ascending order: command c is table row c"""
    return W.encode_ts(np.ones(n), np.arange(1, n + 1), np.full(n, (W.WRITE << 1) | 1), np.ones(n))


def update_rows(ids, cmd, pool, sel, flags=None):
    """row r: an update of command cmd[r] with the Ranges pool.lists[sel[r]]"""
    cmd = np.asarray(cmd, np.int64)
    off, s, e = pool.gather(sel)
    return dict(msb=ids[0][cmd], lsb=ids[1][cmd], node=ids[2][cmd],
                flags=np.zeros(len(cmd), np.uint8) if flags is None else np.asarray(flags, np.uint8),
                rng_off=off, rng_start=s, rng_end=e)


def expected_table(ids, results):
    """results[c] = (erased, ranges or None) of command c, every command of ids present"""
    n = len(results)
    rows = [r if r and not er else [] for er, r in results]
    flat = [p for r in rows for p in r]
    live = sorted(set(flat))
    return dict(msb=ids[0][:n], lsb=ids[1][:n], node=ids[2][:n],
                flags=np.array([ERASED if er else 0 for er, _ in results], np.uint8),
                rng_off=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32),
                rng_start=np.array([s for s, _ in flat], np.uint64), rng_end=np.array([e for _, e in flat], np.uint64),
                dict_start=np.array([s for s, _ in live], np.uint64), dict_end=np.array([e for _, e in live], np.uint64))


def assert_table(got, want, msg):
    for f in TABLE_FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{msg}: table {f}")


def run_fold(ctx, ids, pool, ops, flags, n_stored, want, msg, ei=1):
    """Command c receives pool.lists[ops[k][c]] (flag flags[k][c]) for k = 0, 1, ..: the first n_stored operands in
    an update call each, the rest in one batch laid out operand by operand (all of operand k, then all of k + 1), so
    a command's updates lie n rows apart. The final table must equal `want`."""
    n = len(ops[0])
    cmd = np.arange(n)
    s = RangeCmdStore(ctx, ei)
    try:
        for k in range(n_stored):
            s.update(update_rows(ids, cmd, pool, ops[k], flags[k]))
        rest = range(n_stored, len(ops))
        s.update(update_rows(ids, np.tile(cmd, len(rest)), pool, np.concatenate([ops[k] for k in rest]),
                             np.concatenate([flags[k] for k in rest])))
        st = ctx.stats()
        assert (st["rcmd.inserted"], st["rcmd.updated"]) == ((0, n) if n_stored else (n, 0))
        assert_table(s.table(), want, msg)
    finally:
        s.close()


# ---------------------------------------------------------------- 1, 2. every ordered pair

N_UNI = 233


@pytest.fixture(scope="module")
def uni():
    u = M.universe(7)
    assert len(u) == N_UNI
    return u


@pytest.fixture(scope="module")
def pairs(uni):
    """the model over every ordered pair (a_i, b_j) on point indices, command (i, j) = row i * 233 + j; the point maps
    are monotone, so a mapped pair's result is the mapped result (checked exhaustively in test_ranges_with_model.py)"""
    res = [M.with_kind(a, b) for a in uni for b in uni]
    kinds = [k for _, k in res]
    assert (kinds.count(M.LEFT), kinds.count(M.RIGHT), kinds.count(M.SINK)) == (14875, 9376, 30038)
    return dict(ids=txn_ids(N_UNI * N_UNI), I=np.repeat(np.arange(N_UNI), N_UNI), J=np.tile(np.arange(N_UNI), N_UNI),
                res=[r for r, _ in res], tables={})


def pair_tables(uni, pairs, points):
    """(table after the a's alone, table after a.with(b)) on a point map, built once"""
    if points not in pairs["tables"]:
        pts = POINT_MAPS[points]
        first = [(False, M.mapped(uni[i], pts)) for i in pairs["I"]]
        both = [(False, M.mapped(r, pts)) for r in pairs["res"]]
        pairs["tables"][points] = (expected_table(pairs["ids"], first), expected_table(pairs["ids"], both))
    return pairs["tables"][points]


@pytest.mark.parametrize("points", POINT_MAPS)
def test_stored_then_update_exhaustive(ctx, uni, pairs, points):
    pool = Pool([M.mapped(u, POINT_MAPS[points]) for u in uni])
    first, both = pair_tables(uni, pairs, points)
    n = N_UNI * N_UNI
    s = RangeCmdStore(ctx, 1)
    try:
        s.update(update_rows(pairs["ids"], np.arange(n), pool, pairs["I"]))
        assert ctx.stats()["rcmd.inserted"] == n
        assert_table(s.table(), first, "after the a's")
        s.update(update_rows(pairs["ids"], np.arange(n), pool, pairs["J"]))
        assert ctx.stats()["rcmd.updated"] == n
        assert_table(s.table(), both, "stored a, update b")
    finally:
        s.close()


@pytest.mark.parametrize("points", POINT_MAPS)
def test_in_batch_exhaustive(ctx, uni, pairs, points):
    pool = Pool([M.mapped(u, POINT_MAPS[points]) for u in uni])
    _, both = pair_tables(uni, pairs, points)
    zeros = np.zeros(N_UNI * N_UNI, np.uint8)
    run_fold(ctx, pairs["ids"], pool, [pairs["I"], pairs["J"]], [zeros, zeros], 0, both, "a and b in one batch", ei=0)


# ---------------------------------------------------------------- 3. folds of three and four operands

N_FOLD = 20000


def fold_case(uni, n_ops):
    """N_FOLD seeded tuples of n_ops Ranges of the universe; the second operand is an ERASED update for 4 % of the
    commands, the third for 2 %. -> ops, flags, model results [(erased, ranges)], model paths"""
    rng = np.random.default_rng(0xF01D + n_ops)
    ops = [rng.integers(0, N_UNI, size=N_FOLD) for _ in range(n_ops)]
    flags = [np.zeros(N_FOLD, np.uint8) for _ in range(n_ops)]
    flags[1][rng.random(N_FOLD) < 0.04] = ERASED
    flags[2][rng.random(N_FOLD) < 0.02] = ERASED
    res, paths = [], []
    for c in range(N_FOLD):
        er, cur, path = M.fold(None, [(bool(flags[k][c]), uni[ops[k][c]]) for k in range(n_ops)])
        res.append((er, cur))
        paths.append(tuple(path))
    return ops, flags, res, paths


def assert_fold_paths(paths, n_ops):
    """What the run must contain, from the model (path[0] is FIRST: the command's ranges were null)."""
    S, Lf, R = M.SINK, M.LEFT, M.RIGHT
    seen = set(paths)
    tails = {p[1:] for p in seen}
    assert any(t[:2] == (S, S) for t in tails), "two sink results in a row: both scratch buffers written"
    assert any(t[:2] == (S, Lf) for t in tails), "LEFT while the current Ranges lie in scratch"
    assert any(t[:2] == (S, R) for t in tails), "RIGHT after a sink result: the current Ranges move to the delta's columns"
    assert any(t[0] == "ERASE" and set(t[1:]) == {"IGNORED"} for t in tails), "an ERASED update in the middle, the rest ignored"
    if n_ops == 4:
        assert (S, S, S) in tails, "three sink results: the first buffer written again while the second is read"
        assert (S, R, S) in tails, "a sink result after RIGHT after a sink result"
        assert (S, Lf, S) in tails
        assert any(t[1] == "ERASE" and t[2] == "IGNORED" for t in tails)


@pytest.fixture(scope="module")
def fold_cases(uni):
    return {}


FOLD_SHAPES = [(3, 0), (3, 1), (4, 0), (4, 1), (4, 2)]     # (operands, of which stored before the batch)


@pytest.mark.parametrize("points", POINT_MAPS)
@pytest.mark.parametrize("n_ops,n_stored", FOLD_SHAPES)
def test_multi_step_folds(ctx, uni, fold_cases, n_ops, n_stored, points):
    if n_ops not in fold_cases:
        fold_cases[n_ops] = fold_case(uni, n_ops) + (txn_ids(N_FOLD),)
    ops, flags, res, paths, ids = fold_cases[n_ops]
    assert_fold_paths(paths, n_ops)
    pts = POINT_MAPS[points]
    want = expected_table(ids, [(er, None if r is None else M.mapped(r, pts)) for er, r in res])
    pool = Pool([M.mapped(u, pts) for u in uni])
    run_fold(ctx, ids, pool, ops, flags, n_stored, want, f"{n_ops} operands, {n_stored} stored")


# ---------------------------------------------------------------- 4. long lists

SIZES = (1, 63, 64, 65, 300)


def rand_ranges(rng, k, space):
    """k sorted ranges on about `space` points; consecutive ranges touch where two neighbouring draws are equal"""
    x = np.sort(rng.integers(0, max(space - k, 2), size=2 * k)).tolist()
    return [(x[2 * i] + i, x[2 * i + 1] + i + 1) for i in range(k)]


def long_case():
    """-> lists (the pool), rows [per command the pool indices of its operands in order: the stored Ranges, then one
    update or five]
    For every (L, M): three commands stored L (+) update M on about 3 (L + M) points, two commands taking five updates
    of M ranges after their L, and three neighbouring commands of fully interleaved lists (result: exactly L + M
    ranges, the scratch of the group filled to its last slot; each row shifted, so a write past one group's scratch
    would change its neighbour's result)."""
    rng = np.random.default_rng(0x10C6)
    lists, rows = [], []

    def add(r):
        lists.append(r)
        return len(lists) - 1

    for Ln, Mn in itertools.product(SIZES, SIZES):
        space = 3 * (Ln + Mn)
        for _ in range(3):
            rows.append([add(rand_ranges(rng, Ln, space)), add(rand_ranges(rng, Mn, space))])
        for _ in range(2):
            rows.append([add(rand_ranges(rng, Ln, space))] + [add(rand_ranges(rng, Mn, space)) for _ in range(5)])
        for k in range(3):
            sh = 5 * k
            rows.append([add([(4 * t + sh, 4 * t + 1 + sh) for t in range(Ln)]), add([(4 * t + 2 + sh, 4 * t + 3 + sh) for t in range(Mn)])])
    return lists, rows


@pytest.fixture(scope="module")
def long_lists():
    lists, rows = long_case()
    res, kinds = [], []
    for r in rows:
        er, cur, path = M.fold(None, [(False, lists[i]) for i in r])
        res.append((er, cur))
        kinds.append(path)
    # what the case must contain, from the model
    for base in range(0, len(rows), 8):             # rows 5, 6, 7 of every (L, M): neighbours, each filling its scratch
        for i in (base + 5, base + 6, base + 7):
            assert kinds[i] == ["FIRST", M.SINK] and len(res[i][1]) == len(lists[rows[i][0]]) + len(lists[rows[i][1]])
    assert sum(1 for i, r in enumerate(rows) if len(r) == 2 and kinds[i][1] == M.SINK
               and len(res[i][1]) < len(lists[r[0]]) + len(lists[r[1]])) >= 25, "overlap and touching are common"
    assert any(p.count(M.SINK) >= 4 for p in kinds), "five-update groups going through the sink again and again"
    top = max(e for r in lists for _, e in r)
    return dict(lists=lists, rows=rows, res=res, top=top, ids=txn_ids(len(rows)))


@pytest.mark.parametrize("points", ["small", "wide"])
@pytest.mark.parametrize("n_stored", [1, 0])
def test_long_lists(ctx, long_lists, n_stored, points):
    d = long_lists
    step = 1 if points == "small" else (2**64 - 1) // d["top"]          # monotone: x -> x * step, the top at 2^64 - 1 or just below
    up = lambda r: [(s * step, e * step) for s, e in r]  # noqa: E731
    pool = Pool([up(r) for r in d["lists"]])
    want = expected_table(d["ids"], [(er, up(r)) for er, r in d["res"]])
    rows, n = d["rows"], len(d["rows"])
    s = RangeCmdStore(ctx, 1)
    try:
        if n_stored:
            s.update(update_rows(d["ids"], np.arange(n), pool, [r[0] for r in rows]))
        # the remaining operands round by round: every command's k-th update, then every command's (k + 1)-th
        cmd, sel = [], []
        for k in range(n_stored, 6):
            for c, r in enumerate(rows):
                if k < len(r):
                    cmd.append(c); sel.append(r[k])
        s.update(update_rows(d["ids"], cmd, pool, sel))
        assert_table(s.table(), want, f"long lists, {n_stored} stored, {points}")
    finally:
        s.close()


# ---------------------------------------------------------------- 5. device inputs

@pytest.mark.parametrize("points", POINT_MAPS)
def test_device_inputs(ctx, uni, points):
    """Store A from several batches (an erased command, commands without ranges, commands inserted between and beyond
    the stored ones); its device view handed to an empty store B on the same context as an acc_rcmd_updates with
    mem = ACC_MEM_DEVICE. B equals A on every field, and A is unchanged."""
    pts = POINT_MAPS[points]
    rng = np.random.default_rng(0xDE71CE)
    n = 601                                         # the last command appears in the last batch only, without ranges
    ids = txn_ids(n)
    pool = Pool([M.mapped(u, pts) for u in uni])
    hist = [[] for _ in range(n)]                   # per command: its updates in order
    a = RangeCmdStore(ctx, 1)
    b = RangeCmdStore(ctx, 1)
    try:
        for batch in range(3):
            cmd = rng.choice(np.arange(batch % 2, n - 1, 2 if batch < 2 else 1), size=350)  # even rows, odd rows, then any
            sel = rng.integers(0, N_UNI, size=len(cmd))
            fl = np.where(rng.random(len(cmd)) < 0.03, ERASED, 0).astype(np.uint8)
            if batch == 2:
                cmd = np.concatenate([cmd, [n - 1, 0]]); sel = np.concatenate([sel, [0, 0]]); fl = np.concatenate([fl, [0, ERASED]]).astype(np.uint8)
            a.update(update_rows(ids, cmd, pool, sel, fl))
            for c, i, f in zip(cmd.tolist(), sel.tolist(), fl.tolist()):
                hist[c].append((bool(f), uni[i]))
        present = [c for c in range(n) if hist[c]]
        res = [M.fold(None, hist[c])[:2] for c in present]
        assert any(er for er, _ in res) and any(not er and not r for er, r in res) and res[0][0]
        want = expected_table(tuple(x[present] for x in ids), [(er, None if r is None else M.mapped(r, pts)) for er, r in res])
        tab_a = a.table()
        assert_table(tab_a, want, "store A")
        v = a.view()
        ui = L.RcmdUpdates(v.n_cmd, L.ACC_MEM_DEVICE, v.n_ranges, v.txn_id, v.flags, v.rng_off, v.rng_start, v.rng_end)
        ctx.check(ctx._lib.acc_rcmd_update(ctx.handle, b._h, C.byref(ui)))
        st = ctx.stats()
        assert (st["rcmd.inserted"], st["rcmd.updated"], st["rcmd.erased_ignored"]) == (len(present), 0, 0)
        tab_b = b.table()
        assert_table(tab_b, tab_a, "store B from A's device view")
        assert tab_b["end_inclusive"] == tab_a["end_inclusive"]
        assert_table(a.table(), tab_a, "store A after B read it")
    finally:
        a.close()
        b.close()
