"""An independent model of Ranges.with and AbstractRanges.containsAll(Ranges), for the tests.

What it specifies: AbstractRanges.union(MERGE_OVERLAPPING, left, right) (primitives/AbstractRanges.java:496-585), which
Ranges.with calls (primitives/Ranges.java:119-127), with its helper supersetLinearMerge (AbstractRanges.java:439-484) and
the other user of that helper, containsAll(AbstractRanges) (AbstractRanges.java:96-101).

How it was obtained: by reading those loops and stating what they compute as properties of the two inputs (which operand
leads, which prefix of the other is already covered, what is copied as it is, how a sweep in start order groups the
rest), not by restating the two-pointer loops; no text of the reference is copied. It shares no code with the library:
plain Python over lists of (start, end) int tuples with arbitrary-precision ints, so bounds at 2^63 and 2^64 - 1 need no
care. tests/test_ranges_with_model.py compares it with the library on every ordered pair of Ranges over seven points
and pins hand-worked cases per branch of the Java.

A Ranges is a list of (start, end) with start < end, sorted, each start >= the previous end (touching allowed).
"""
from bisect import bisect_right

LEFT, RIGHT, SINK = "LEFT", "RIGHT", "SINK"


def components(rs):
    """The ranges with every run of touching ranges (end == next start) merged into one."""
    out = []
    for s, e in rs:
        if out and out[-1][1] == s:
            out[-1] = (out[-1][0], e)
        else:
            out.append((s, e))
    return out


def _covered_prefix(a, b):
    """Length of the longest prefix of b whose ranges each lie inside one component of a."""
    comps = components(a)
    starts = [c[0] for c in comps]
    n = 0
    for s, e in b:
        i = bisect_right(starts, s) - 1          # the last component starting at or below s
        if i < 0 or e > comps[i][1]:
            break
        n += 1
    return n


def contains_all(a, b):
    """a.containsAll(b): every range of b lies inside one touching-merged component of a."""
    return _covered_prefix(a, b) == len(b)


def with_kind(left, right):
    """left.with(right) -> (result, kind). kind says where the result is: LEFT or RIGHT when the method returns the
    operand it was given (result is that list, unchanged), SINK when it builds a new list."""
    left, right = list(left), list(right)
    if not right:
        return left, LEFT
    if not left:
        return right, RIGHT
    # the leading operand: the smaller first start; on a tie the larger last end; on a full tie left
    lead_right = (right[0][0], -right[-1][1]) < (left[0][0], -left[-1][1])
    a, b = (right, left) if lead_right else (left, right)
    bi = _covered_prefix(a, b)
    if bi == len(b):
        return a, (RIGHT if lead_right else LEFT)
    # everything of a that ends at or before the first uncovered range of b starts is copied as it is
    ai = sum(1 for _, e in a if e <= b[bi][0])
    out = a[:ai]
    cur, merged = None, False
    for s, e in sorted(a[ai:] + b[bi:], key=lambda r: r[0]):
        if cur is not None and (s < cur[1] or (merged and s == cur[1])):
            cur = (cur[0], max(cur[1], e))
            merged = True
            continue
        if cur is not None:
            out.append(cur)
        cur, merged = (s, e), False
    out.append(cur)
    return out, SINK


def with_(left, right):
    return with_kind(left, right)[0]


def fold(stored, updates):
    """A range command under InMemorySafeStore.update per update in order (impl/InMemoryCommandStore.java:739-762,
    RangeCommand.update: ranges = ranges == null ? add : ranges.with(add)).
    stored: None (no such command), or (erased, ranges or None); updates: [(erased, ranges)].
    -> (erased, ranges or None, path): path lists per update "ERASE", "IGNORED" (the command was erased already),
    "FIRST" (ranges == null) or the kind of the with()."""
    erased, cur = (False, None) if stored is None else stored
    path = []
    for er, add in updates:
        if erased:
            path.append("IGNORED")
        elif er:
            erased, cur = True, None
            path.append("ERASE")
        elif cur is None:
            cur = list(add)
            path.append("FIRST")
        else:
            cur, k = with_kind(cur, add)
            path.append(k)
    return erased, cur, path


# ---------------------------------------------------------------- the exhaustive universe

def universe(n_points=7):
    """Every Ranges whose bounds are among the points 0 .. n_points - 1, touching allowed, the empty one first:
    233 for seven points, the longest of 6 ranges."""
    out = []

    def grow(prefix, lo):
        out.append(list(prefix))
        for s in range(lo, n_points):
            for e in range(s + 1, n_points):
                grow(prefix + [(s, e)], e)

    grow([], 0)
    return out


WIDE_POINTS = (0, 1, 2**32 - 1, 2**32, 2**63 - 1, 2**63, 2**64 - 1)


def mapped(rs, points):
    return [(points[s], points[e]) for s, e in rs]
