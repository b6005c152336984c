"""The model of acc_rcmd_redundant_before (rcmd_redundant_model.py) against the host restatement of the reference's
AbstractRanges.subtract (accord_amd.ranges.Ranges.subtract, itself pinned by the reference's literals in
test_ranges_literals.py), and hand-worked literals. No GPU."""
import itertools

import numpy as np
import pytest

import ranges_model
from accord_amd import workload as W
from accord_amd.ranges import Ranges
from rcmd_redundant_model import RedundantModel, TAGS, cut, cut_range, pairs
from test_rcmd_gpu import ts, updates


def R(prs, ei):
    return Ranges(np.array([a for a, _ in prs], np.uint64), np.array([b for _, b in prs], np.uint64), ei)


@pytest.mark.parametrize("ei", [0, 1])
def test_cut_equals_subtract_exhaustively(ei):
    """every ordered pair of Ranges over six points (touching ranges on both sides included)"""
    uni = ranges_model.universe(6)
    assert len(uni) > 80
    for left, right in itertools.product(uni, uni):
        assert cut(left, right) == list(R(left, ei).subtract(R(right, ei))), (left, right)


def test_cut_at_wide_bounds():
    uni = ranges_model.universe(5)
    pts = (0, 1, 2**32, 2**63, 2**64 - 1)
    for left, right in itertools.product(uni, uni):
        l, r = ranges_model.mapped(left, pts), ranges_model.mapped(right, pts)
        assert cut(l, r) == list(R(l, 0).subtract(R(r, 0))), (l, r)


def test_one_at_a_time_in_both_orders_equals_at_once():
    """one call with several bounds is the reference's calls one per bound, in any order"""
    uni = ranges_model.universe(6)
    for left in uni[::3]:
        for right in uni:
            if len(right) < 2:
                continue
            want = cut(left, right)
            for seq in (right, right[::-1]):
                cur = left
                for r in seq:
                    cur = cut(cur, [r])
                assert cur == want, (left, right)
            cur = R(left, 0)
            for r in right[::-1]:
                cur = cur.subtract(R([r], 0))
            assert list(cur) == want


def test_reference_literal():
    assert cut_range(100, 200, [(0, 125), (135, 140), (160, 170), (170, 175)]) == [(125, 135), (140, 160), (175, 200)]
    assert cut([(100, 200)], [(0, 125), (135, 140), (160, 170), (170, 175)]) == [(125, 135), (140, 160), (175, 200)]
    # nothing is merged across two ranges of the left side, no zero-width piece is made
    assert cut([(0, 10), (10, 20)], [(5, 15)]) == [(0, 5), (15, 20)]
    assert cut([(0, 10), (10, 20)], [(30, 40)]) == [(0, 10), (10, 20)]
    assert cut([(0, 10)], [(0, 10)]) == [] and cut([(0, 10)], [(0, 5), (5, 10)]) == []


@pytest.mark.parametrize("ei", [0, 1])
def test_mark_shard_durable_walk_through(ei):
    """InMemoryCommandStore.markShardDurable(syncId = hlc 50, ranges = {(10, 30)}) over three range commands:
         A hlc 20  {(5, 15), (40, 50)}   below syncId: ranges.subtract -> {(5, 10), (40, 50)}, not empty, stays
         B hlc 30  {(12, 28)}            below syncId: nothing is left, removeIf removes it
         C hlc 50  {(0, 100)}            compareTo(syncId) == 0, not < 0: untouched
         D hlc 60  {(20, 25)}            above syncId: untouched"""
    A, B, Cc, D = ts(20), ts(30), ts(50), ts(60)
    m = RedundantModel(ei)
    m.apply(updates([(A, 0, [(5, 15), (40, 50)]), (B, 0, [(12, 28)]), (Cc, 0, [(0, 100)]), (D, 0, [(20, 25)])]))
    m.mark([(10, 30)], [ts(50, W.WRITE, rng=0, extra=0x20)])   # bits outside compareTo (the domain bit too) do not matter
    t = m.table()
    assert t["lsb"].tolist() == [A[1], Cc[1], D[1]]
    assert t["rng_off"].tolist() == [0, 2, 3, 4]
    assert list(zip(t["rng_start"].tolist(), t["rng_end"].tolist())) == [(5, 10), (40, 50), (0, 100), (20, 25)]
    assert m.rstats == dict(cmds_cut=1, cmds_dropped=1, ranges_before=5, ranges_after=4)
    assert {"cut_tail", "covered_whole_range", "equal_bound_stays"} <= m.seen
    # registration from now on: an update of a TxnId below the bound keeps only what lies outside (10, 30)
    m.apply(updates([(ts(40), 0, [(0, 20), (25, 60)]), (ts(41), 0, [(11, 29)]), (ts(70), 0, [(11, 29)])]))
    t = m.table()
    off = t["rng_off"].tolist()
    row = lambda i: list(zip(t["rng_start"][off[i]:off[i + 1]].tolist(), t["rng_end"][off[i]:off[i + 1]].tolist()))  # noqa: E731
    assert t["lsb"].tolist() == [A[1], ts(40)[1], ts(41)[1], Cc[1], D[1], ts(70)[1]]
    assert row(1) == [(0, 10), (30, 60)] and row(2) == [] and row(5) == [(11, 29)]
    assert m.trimmed == 3 and {"trim_partial", "trim_to_nothing_inserted_empty"} <= m.seen
    # a second sync point above everything over everything: the store empties, the tombstone-free table is gone
    m.mark([(0, 1000)], [ts(1000)])
    assert len(m.table()["msb"]) == 0 and "store_emptied" in m.seen and "dropped_already_empty" in m.seen
    assert m.seen - {"shortcut_unchanged", "appended_disjoint", "merged", "in_batch_repeat", "insert_below_lowest",
                     "insert_above_highest"} <= TAGS
    assert pairs(None) == []
