"""The model of acc_rcmd_partial_rangedeps (partial_rangedeps_model.py) pinned by literals worked by hand from
PreAccept.calculatePartialDeps (messages/PreAccept.java:245-265), RedundantBefore.collectDeps
(local/RedundantBefore.java:181-190, 418-421), ReducingRangeMap.foldl (utils/ReducingRangeMap.java:120-196) and
RangeDeps.with (primitives/RangeDeps.java:567-581), under both bound types. No GPU.

The store of every case (key codes; K(lo, hi) is the Range holding exactly the codes lo..hi: (lo - 1, hi] EndInclusive,
[lo, hi + 1) StartInclusive):
  commands   S = hlc 200, a SyncPoint, ranges {K(30, 39)}      D = hlc 300, a Write, ranges {K(12, 33)}
  the map    I1 = K(10, 19) -> X = hlc 100        N  = K(20, 24) -> TxnId.NONE      (25..29: no entry)
             I2 = K(30, 39) -> Y = hlc 200, given with a flag bit outside Timestamp.equals set (S's own TxnId)
             I3 = K(40, 49) -> X with another such flag bit set       I4 = K(60, 69) -> X
  S and D stay (S is not below Y, D is above every bound). Every query lies far above all of them; all are Writes,
  which witness D and not S, but for one ExclusiveSyncPoint, which witnesses both.
"""
import numpy as np
import pytest

from accord_amd import workload as W
from cfk_redundant_model import NONE, order
from partial_rangedeps_model import NO_ROW, describe, model_intervals, partial_rangedeps
from rcmd_redundant_model import RedundantModel
from test_rcmd_gpu import expect_rangedeps, queries, ts, updates

X, Y, S, D = ts(100), ts(200, W.SYNC_POINT, extra=0x20), ts(200, W.SYNC_POINT), ts(300)
X2 = ts(100, extra=0x8000)


def K(lo, hi, ei):
    return (lo - 1, hi) if ei else (lo, hi + 1)


def store(ei):
    m = RedundantModel(ei)
    m.apply(updates([(S, 0, [K(30, 39, ei)]), (D, 0, [K(12, 33, ei)])]))
    m.mark([K(10, 19, ei), K(20, 24, ei), K(30, 39, ei), K(40, 49, ei), K(60, 69, ei)], [X, NONE, Y, X2, X])
    return m


def run(m, items):
    q = queries(items)
    tab = m.table()
    res = partial_rangedeps(tab, expect_rangedeps(tab, q, m.ei), model_intervals(m), q, m.ei)
    return res, [describe(res, t) for t in range(len(items))]


def test_bound_types_are_what_the_literals_say():
    assert K(10, 19, 1) == (9, 19) and K(10, 19, 0) == (10, 20)
    assert order(X) == order(X2) and X != X2 and order(Y) == order(S) and Y != S


@pytest.mark.parametrize("ei", [0, 1])
def test_hand_worked_literals(ei):
    m = store(ei)
    tab = m.table()
    assert [order(t) for t in zip(tab["msb"], tab["lsb"], tab["node"])] == [order(S), order(D)], "the prune dropped nothing"
    assert [v for _, _, v in m.map.intervals()] == [order(X), order(NONE), order(Y), order(X), order(X)]
    k = lambda lo, hi: K(lo, hi, ei)  # noqa: E731
    I1, I2, I3, I4, Dr = k(10, 19), k(30, 39), k(40, 49), k(60, 69), k(12, 33)
    x, y, d = order(X), order(Y), order(D)
    T = lambda i: ts(1000 + i, W.WRITE, rng=0)  # noqa: E731
    Tr = lambda i: ts(1000 + i, W.WRITE)  # noqa: E731
    res, got = run(m, [
        (T(0), None, [10], []),             # a key on I1's first code: foldl finds the entry holding 10
        (T(1), None, [19], []),             # on its last code (D's range holds 19 too: the stab half)
        (T(2), None, [9], []),              # one step below: no entry
        (T(3), None, [20], []),             # one step above: the entry there holds NONE, which collectDeps skips
        (Tr(4), None, [], [k(20, 25)]),     # a range that starts where I1 ends: touching, no intersection
        (Tr(5), None, [], [k(5, 9)]),       # a range that ends where I1 starts
        (Tr(6), None, [], [k(19, 25)]),     # the same range one code longer: it intersects I1 by that code
        (ts(1007, W.EXCLUSIVE_SYNC_POINT), None, [], [k(15, 45)]),   # over I1, the NONE entry, the gap, I2 and I3: three
                                            # pairs, none for the gap (an ExclusiveSyncPoint: it witnesses S)
        (T(8), None, [12, 65], []),         # I1 and I4: two ranges, one TxnId
        (T(9), None, [], []),               # no participants
        (T(10), None, [41], []),            # I3 alone: its bound is X by Timestamp.equals
    ])
    assert got[0] == {I1: [x]}
    assert got[1] == {I1: [x], Dr: [d]}
    assert got[2] == {}
    assert got[3] == {Dr: [d]}
    assert got[4] == {Dr: [d]}
    assert got[5] == {}
    assert got[6] == {I1: [x], Dr: [d]}
    assert got[7] == {I1: [x], Dr: [d], I2: [y], I3: [x]}, "(I2, Y) is on both sides: S is stored with that range; once"
    assert got[8] == {I1: [x], I4: [x], Dr: [d]}
    assert got[9] == {}
    assert got[10] == {I3: [x]}
    # the union tables: every interval above NONE is in the dictionary, touched or not; X once, with the bits of the lowest
    # interval holding it; Y with the stored row's bits (linearUnion keeps the left instance)
    assert list(zip(res["rng_start"].tolist(), res["rng_end"].tolist())) == sorted([I1, Dr, I2, I3, I4])
    assert list(zip(res["msb"].tolist(), res["lsb"].tolist(), res["node"].tolist())) == [X, S, D]
    assert res["id_row"].tolist() == [NO_ROW, 0, 1]
    assert res["intervals"] == 1 + 1 + 0 + 0 + 0 + 0 + 1 + 3 + 2 + 0 + 1 and res["shared"] == 1
    # the CSR of query 7 in the Java layout: ranges by Range::compare, TxnIds by compareTo, rangesToTxnIds = the ends of
    # the four lists, then the lists as positions in the query's own TxnIds [X, Y, D]
    a0, a1 = int(res["arena_off"][7]), int(res["arena_off"][8])
    order_of = sorted([I1, Dr, I2, I3])
    lists = {I1: [0], Dr: [2], I2: [1], I3: [0]}
    flat = [p for r in order_of for p in lists[r]]
    assert res["arena"][a0:a1].tolist() == [5, 6, 7, 8] + flat
    assert res["range_id"][int(res["rd_off"][7]):int(res["rd_off"][8])].tolist() == [sorted([I1, Dr, I2, I3, I4]).index(r) for r in order_of]
    assert res["dep_txn"][int(res["u_off"][7]):int(res["u_off"][8])].tolist() == [0, 1, 2]


@pytest.mark.parametrize("ei", [0, 1])
def test_no_other_filter(ei):
    """No STARTED_BEFORE test (a query below its bound, and one equal to it), no witnesses() test (a Read does not witness
    a SyncPoint: the pair is still there), no look at the bound's own domain; the stab half keeps all three filters."""
    m = store(ei)
    k = lambda lo, hi: K(lo, hi, ei)  # noqa: E731
    y = order(Y)
    res, got = run(m, [
        (ts(150, W.WRITE, rng=0), None, [35], []),           # below Y: S (hlc 200) is no stab dep, the bound is a dep
        ((S[0], S[1] & ~1, S[2]), None, [35], []),           # Timestamp.equals to Y, key domain: S is never its own stab dep
        (ts(1000, W.READ, rng=0), None, [35], []),           # a Read witnesses no SyncPoint: no stab dep on S
    ])
    assert got == [{k(30, 39): [y]}] * 3
    assert res["shared"] == 0


def test_empty_store_and_none_only_map():
    m = RedundantModel(1)
    m.mark([(0, 10)], [NONE])
    res, got = run(m, [(ts(5, rng=0), None, [3], [])])
    assert got == [{}] and len(res["msb"]) == 0 and len(res["rng_start"]) == 0 and res["intervals"] == 0
    m.mark([(4, 6)], [X])
    res, got = run(m, [(ts(5, rng=0), None, [3], []), (ts(6, rng=0), None, [5], [])])
    assert got == [{}, {(4, 6): [order(X)]}] and res["id_row"].tolist() == [NO_ROW]
    assert np.array_equal(res["u_off"], [0, 0, 1])
