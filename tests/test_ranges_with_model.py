"""The host Ranges.with and containsAll (acc_ranges_with, acc_ranges_contains_all: csrc/ranges_with.hpp, the code the
device fold of the range-command store runs as well) against the independent model of tests/ranges_model.py.

Exhaustive: every ordered pair of the 233 Ranges over seven points, on the points 0..6 and on the same points mapped to
{0, 1, 2^32 - 1, 2^32, 2^63 - 1, 2^63, 2^64 - 1}; the result is compared range by range (how it is cut, not only which
points it covers). The census of result kinds is asserted so the universe cannot shrink unnoticed.
The branch catalogue pins one hand-worked pair per branch of AbstractRanges.union / supersetLinearMerge
(primitives/AbstractRanges.java:439-585): the expected values were worked from the Java by hand, and both the model and
the library must give them."""
import ctypes as C

import numpy as np
import pytest

import ranges_model as M

POINT_MAPS = {"small": tuple(range(7)), "wide": M.WIDE_POINTS}


@pytest.fixture(scope="module")
def uni():
    return M.universe(7)


@pytest.fixture(scope="module")
def model_pairs(uni):
    """[(i, j, result, kind)] of the model over every ordered pair, on point indices (the maps are monotone, and the
    model only compares bounds, so the mapped result is the mapped ranges; test_model_commutes_with_the_point_map
    checks that on the wide map)."""
    return [(i, j) + M.with_kind(a, b) for i, a in enumerate(uni) for j, b in enumerate(uni)]


def test_universe(uni):
    assert len(uni) == 233 and max(len(r) for r in uni) == 6 and uni[0] == []
    assert len({tuple(r) for r in uni}) == 233
    for r in uni:
        assert all(s < e for s, e in r) and all(r[k - 1][1] <= r[k][0] for k in range(1, len(r)))


def test_census(model_pairs):
    """Measured through ranges_with.hpp on this universe: LEFT 14,875, RIGHT 9,376, SINK 30,038."""
    kinds = [k for _, _, _, k in model_pairs]
    assert len(kinds) == 54289
    assert (kinds.count(M.LEFT), kinds.count(M.RIGHT), kinds.count(M.SINK)) == (14875, 9376, 30038)


def test_model_commutes_with_the_point_map(uni, model_pairs):
    pts = M.WIDE_POINTS
    for i, j, res, kind in model_pairs:
        assert M.with_kind(M.mapped(uni[i], pts), M.mapped(uni[j], pts)) == (M.mapped(res, pts), kind)


class HostLib:
    """acc_ranges_with / acc_ranges_contains_all on prebuilt argument lists (one pair per call, no per-call arrays)."""

    def __init__(self, uni, points):
        from accord_amd import _lib as L
        from accord_amd.ranges import RList, _lib
        self.lib, self.ok = _lib(), L.ACC_OK
        self.keep, self.rl = [], []
        for r in uni:
            s = np.array([points[a] for a, _ in r], np.uint64)
            e = np.array([points[b] for _, b in r], np.uint64)
            self.keep.append((s, e))
            self.rl.append(RList(s.ctypes.data if len(r) else None, e.ctypes.data if len(r) else None, len(r), 0))
        self.os, self.oe = np.zeros(16, np.uint64), np.zeros(16, np.uint64)
        self.n, self.flag = C.c_uint32(0), C.c_int32(0)

    def with_(self, i, j):
        assert self.lib.acc_ranges_with(C.byref(self.rl[i]), C.byref(self.rl[j]), self.os.ctypes.data, self.oe.ctypes.data,
                                        16, C.byref(self.n)) == self.ok
        n = self.n.value
        return list(zip(self.os[:n].tolist(), self.oe[:n].tolist()))

    def contains_all(self, i, j):
        assert self.lib.acc_ranges_contains_all(C.byref(self.rl[i]), C.byref(self.rl[j]), C.byref(self.flag)) == self.ok
        return bool(self.flag.value)


@pytest.mark.parametrize("points", POINT_MAPS)
def test_with_exhaustive(uni, model_pairs, points):
    pts = POINT_MAPS[points]
    h = HostLib(uni, pts)
    bad = [(uni[i], uni[j], got, M.mapped(res, pts)) for i, j, res, _ in model_pairs
           if (got := h.with_(i, j)) != M.mapped(res, pts)]
    assert not bad, f"{len(bad)} of {len(model_pairs)} pairs differ; first (left, right, library, model): {bad[0]}"


@pytest.mark.parametrize("points", POINT_MAPS)
def test_contains_all_exhaustive(uni, points):
    pts = POINT_MAPS[points]
    h = HostLib(uni, pts)
    bad, yes = [], 0
    for i, a in enumerate(uni):
        ma = M.mapped(a, pts)
        for j, b in enumerate(uni):
            want = M.contains_all(ma, M.mapped(b, pts))
            yes += want
            if h.contains_all(i, j) != want:
                bad.append((a, b, want))
    assert not bad, f"{len(bad)} pairs differ; first (a, b, model): {bad[0]}"
    assert 233 < yes < 54289 // 2


# ---------------------------------------------------------------- literals

def lib_with(a, b):
    from accord_amd.ranges import Ranges
    r = lambda x: Ranges([s for s, _ in x], [e for _, e in x])  # noqa: E731
    return list(r(a).with_(r(b)))


NOT_COMMUTATIVE_A = [(0, 1), (2, 3), (4, 5)]
NOT_COMMUTATIVE_B = [(0, 2), (3, 5)]


def test_with_is_not_commutative():
    """Ranges.with depends on the argument order. a.with(b): equal first starts and equal last ends, so a leads
    (:504-508); (0,2) is not covered by a's first range and the run breaks on the gap at 1 (:473); the group opened by
    (0,1) x (0,2) then absorbs every later range, each starting at or below the running end (:557-569).
    b.with(a): b leads; (0,1) lies inside (0,2) (:460-463), (2,3) starts at b[0]'s end (:448-451) and ends where (3,5)
    starts (:452-455), so it is written between them as it is (:545-549); (4,5) x (3,5) opens a group of its own."""
    a, b = NOT_COMMUTATIVE_A, NOT_COMMUTATIVE_B
    for f in (M.with_, lib_with):
        assert f(a, b) == [(0, 5)]
        assert f(b, a) == [(0, 2), (2, 3), (3, 5)]
    assert M.with_kind(a, b)[1] == M.with_kind(b, a)[1] == M.SINK


# (name, left, right, expected, kind): AbstractRanges.java lines in the name's comment
CATALOGUE = [
    # :498 right.isEmpty() -> left; :499 left.isEmpty() -> right
    ("right_empty", [(1, 2), (2, 3)], [], [(1, 2), (2, 3)], M.LEFT),
    ("left_empty", [], [(1, 2), (2, 3)], [(1, 2), (2, 3)], M.RIGHT),
    # :504-508 equal first starts, left's last end below right's: right leads, and its touching run (0,1)(1,3) covers
    # (0,2) (:470-479) -> right itself (:517-518). Were left to lead, (0,2) x (1,3) would merge to {(0,3)}.
    ("tie_on_start_decided_by_last_end", [(0, 2)], [(0, 1), (1, 3)], [(0, 1), (1, 3)], M.RIGHT),
    # :505 a full tie: left leads; the run (0,1)(1,2) reaches (0,2)'s end -> left itself
    ("full_tie_left_leads", [(0, 1), (1, 2)], [(0, 2)], [(0, 1), (1, 2)], M.LEFT),
    ("full_tie_left_leads_reversed", [(0, 2)], [(0, 1), (1, 2)], [(0, 2)], M.LEFT),
    # :504 left starts above right: swapped, right covers left -> right itself
    ("swapped_superset", [(2, 3)], [(0, 5)], [(0, 5)], M.RIGHT),
    # :470-479 (1,5) covered by the touching run (0,2)(2,4)(4,6): ai moves to the run's last range, which then lies
    # before (8,9) (:448-451); (8,9) equals a's last range (:460-463, both advance)
    ("superset_through_touching_run", [(0, 2), (2, 4), (4, 6), (8, 9)], [(1, 5), (8, 9)], [(0, 2), (2, 4), (4, 6), (8, 9)], M.LEFT),
    # :473 ++tmpai == as.length: the run (0,2)(2,4) ends before reaching 5; nothing copied, one group absorbs all
    ("run_falls_short", [(0, 2), (2, 4)], [(1, 5)], [(0, 5)], M.SINK),
    # :473 second clause: the run breaks on the gap between 2 and 3; (3,6) starts below the running end 5
    ("run_breaks_on_gap", [(0, 2), (3, 6)], [(1, 5)], [(0, 6)], M.SINK),
    # :456-459 b starts below the a it intersects: (0,1) was passed (:448-451) and is copied (:530), then one group
    ("b_starts_below_a", [(0, 1), (3, 5)], [(2, 4)], [(0, 1), (2, 5)], M.SINK),
    # :452-455 a lies wholly after b: break; (0,1) copied, b written between (:545-549), a's tail copied (:574-575)
    ("a_after_b", [(0, 1), (5, 6)], [(2, 3)], [(0, 1), (2, 3), (5, 6)], M.SINK),
    # :460-463 b ends with a: both advance; the next b lies in the next a
    ("equal_ends_advance_both", [(0, 2), (2, 4)], [(1, 2), (2, 3)], [(0, 2), (2, 4)], M.LEFT),
    # a covered prefix (2,3); (1,5)(5,10) passed and copied as they are, still touching (:530); (20,30) x (25,40)
    ("covered_prefix_verbatim_pair_then_merge", [(1, 5), (5, 10), (20, 30)], [(2, 3), (25, 40)], [(1, 5), (5, 10), (20, 40)], M.SINK),
    # :563 a next range joins a group unless it starts above the running end: (4,6) touches the end 4 and joins, then
    # (6,8) touches 6 and joins
    ("touching_absorbed_inside_group", [(0, 2), (4, 6)], [(1, 4), (6, 8)], [(0, 8)], M.SINK),
    # touching before any group stays apart: (0,2) | (2,4) (:540-549 write them one by one); the group (5,7) x (6,9)
    # then absorbs (9,10), which touches its end
    ("touching_kept_before_group", [(0, 2), (5, 7), (9, 10)], [(2, 4), (6, 9)], [(0, 2), (2, 4), (5, 10)], M.SINK),
    # :557-569 one group fed from both sides in turn: a, b, a, b, a, b
    ("group_alternates_sides", [(0, 3), (4, 7), (8, 11)], [(2, 5), (6, 9), (10, 13)], [(0, 13)], M.SINK),
    # :557-564 a exhausted inside the group, b's next range starts above the end: break; b's tail copied (:577-578)
    ("b_tail_copied", [(0, 2)], [(1, 3), (5, 6), (6, 7)], [(0, 3), (5, 6), (6, 7)], M.SINK),
    # :540-544 after a group, an a before the next b is written as it is; then a second group
    ("a_between_two_groups", [(0, 2), (4, 5), (8, 10)], [(1, 3), (9, 11)], [(0, 3), (4, 5), (8, 11)], M.SINK),
    # RangesTest.addTest (RangesTest.java:78-83): touching ranges of different inputs, no overlap anywhere
    ("interleaved_touching", [(0, 50), (100, 150)], [(50, 100), (150, 200)], [(0, 50), (50, 100), (100, 150), (150, 200)], M.SINK),
]


@pytest.mark.parametrize("name,left,right,want,kind", CATALOGUE, ids=[c[0] for c in CATALOGUE])
def test_branch_catalogue(name, left, right, want, kind):
    assert M.with_kind(left, right) == (want, kind)
    assert lib_with(left, right) == want
    top = 2**64 - 1 - 200                       # the same case against the top of the u64 space
    up = lambda rs: [(s + top, e + top) for s, e in rs]  # noqa: E731
    assert M.with_(up(left), up(right)) == up(want)
    assert lib_with(up(left), up(right)) == up(want)


def test_contains_all_literals():
    """supersetLinearMerge as containsAll uses it (:96-101): the cases of test_ranges_literals, on the model."""
    cov = [(0, 100), (100, 200), (300, 400)]
    assert M.contains_all(cov, [(10, 20), (150, 200)]) and M.contains_all(cov, [(50, 150)])
    assert not M.contains_all(cov, [(150, 250)]) and not M.contains_all(cov, [(250, 260)])
    assert M.contains_all([], []) and not M.contains_all([], [(1, 2)]) and M.contains_all(cov, [])
