"""The searches of csrc/search.hpp on their own, through the test shim (csrc/prims_test.hip, prims_shim.py): lower_bound /
upper_bound for u32 and u64 elements under a u32 and a u64 index type, seg_of, find_sorted, the Timestamp bounds over a
column triple, and wave_search. References: numpy.searchsorted (left / right), and for Timestamps Python's bisect over
the key (msb, lsb & IDENTITY_LSB, signed node). Every comparison is exact equality, and every output carries a guard
element that must keep the shim's fill.

Array lengths sit on both sides of a wave and a block (0 .. 3, 255 .. 257); wave_search adds the lengths at which it takes
one, two and three probe rounds (64 / 65, 4096 / 4097 = 64 * 64 + 1, 262145 = 64^3 + 1). Arrays hold runs of equal values
at the start, in the middle and at the end; queries lie below all, above all, on the first and last element, on every
element and between neighbours; windows start above 0 and end below the array's end.
"""
import bisect

import numpy as np
import pytest

from prims_shim import FILL32, FILL64, Shim

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 255, 256, 257]
IDENTITY_LSB = 0xFFFFFFFFFFFF001E
NOT_FOUND = 0xFFFFFFFF


@pytest.fixture(scope="module")
def shim():
    from accord_amd.deps import Context
    c = Context(0)
    s = Shim(c)
    yield s
    s.close()
    c.close()


def eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    if not np.array_equal(got.astype(np.uint64), want.astype(np.uint64)):
        i = int(np.flatnonzero(got.astype(np.uint64) != want.astype(np.uint64))[0])
        raise AssertionError(f"{what}: first difference at query {i} of {len(want)}: got {got[i]}, want {want[i]}")


def sorted_with_runs(rng, n, dtype):
    """n sorted values over the whole range of dtype (u64: half of them >= 2^63), runs of equal values at the start, the
    middle and the end; from 3 elements on the first run is 0 and the last one the type's largest value"""
    a = rng.randint(0, 1 << 32, size=n, dtype=np.uint64)
    if dtype == np.uint64:
        a = (a << np.uint64(32)) | rng.randint(0, 1 << 32, size=n, dtype=np.uint64)
    a = np.sort(a.astype(dtype))
    if n:
        r = max(1, min(5, n // 3))
        a[:r] = 0 if n >= 3 else a[0]
        a[n // 2:n // 2 + r] = a[n // 2]
        a[n - r:] = np.iinfo(dtype).max if n >= 3 else a[n - 1]
    assert (a[:-1] <= a[1:]).all()
    return a


def queries_for(a, dtype):
    """below all, above all, the type's ends, every element, and the values next to and between the elements"""
    top = np.iinfo(dtype).max
    q = [0, 1, top, top - 1]
    if dtype == np.uint64:
        q += [1 << 63, (1 << 63) - 1, (1 << 63) + 1]
    for x in a.tolist():
        q += [x, max(x - 1, 0), min(x + 1, top)]
    for x, y in zip(a[:-1].tolist(), a[1:].tolist()):
        q.append(x + (y - x) // 2)
    return np.array(q, dtype=dtype)


def windows(n):
    """(lo, hi): the whole array, a non-zero lo, an hi below the end, both, and an empty window inside"""
    w = [(0, n)]
    if n >= 2:
        w += [(1, n), (0, n - 1), (n // 3, n - n // 4), (n // 2, n // 2)]
    if n >= 3:
        w.append((1, n - 1))
    return w


def ref_bound(a, lo, hi, v, upper):
    return lo + np.searchsorted(a[lo:hi], v, side="right" if upper else "left")


@pytest.mark.parametrize("idx64", [False, True])
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("upper", [False, True])
def test_lower_upper_bound(shim, upper, dtype, idx64):
    rng = np.random.RandomState(7 + 2 * int(upper) + int(dtype == np.uint64))
    for n in LENGTHS:
        a = sorted_with_runs(rng, n, dtype)
        q = queries_for(a, dtype)
        for lo, hi in windows(n):
            got, guard = shim.search_bound(a, np.full(len(q), lo), np.full(len(q), hi), q, upper, idx64)
            what = f"{'upper' if upper else 'lower'}_bound {np.dtype(dtype).name} idx64={idx64} n={n} window [{lo}, {hi})"
            eq(got, ref_bound(a, lo, hi, q, upper), what)
            assert lo <= got.min() and got.max() <= hi, f"{what}: a result outside the window"
            assert guard == FILL64, f"{what}: guard element overwritten"


def test_seg_of(shim):
    rng = np.random.RandomState(11)
    for n in [1, 2, 3, 255, 256, 257]:
        # offsets from 0 with repeated values: empty segments at the start, the middle and the end
        cnt = rng.randint(0, 4, size=n).astype(np.uint32)
        cnt[rng.randint(0, n, size=max(1, n // 3))] = 0
        if n >= 3:
            cnt[0] = 0
            cnt[n // 2] = 0
        off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint32)   # off[i] = start of segment i
        last = int(off[-1])
        v = np.unique(np.array([0, last, last + 1, last + 1000] + off.tolist() + (off + 1).tolist(), dtype=np.uint32))
        got, guard = shim.seg_of(off, v)
        # the last i with off[i] <= v: among equal offsets the last one, so empty segments are skipped
        eq(got, np.searchsorted(off, v, side="right") - 1, f"seg_of n={n}")
        assert guard == FILL32
    got, guard = shim.seg_of(np.zeros(0, np.uint32), [0, 5])   # n == 0: 0 by definition, nothing is read
    eq(got, [0, 0], "seg_of n=0")
    assert guard == FILL32


def test_find_sorted(shim):
    rng = np.random.RandomState(13)
    for n in LENGTHS:
        a = np.unique(sorted_with_runs(rng, n + 16, np.uint64))   # a store's keys: strictly ascending, 0 and 2^64 - 1 among them
        a = np.concatenate([a[:n // 2], a[len(a) - (n - n // 2):]])
        assert len(a) == n and (a[:-1] < a[1:]).all()
        q = queries_for(a, np.uint64)
        got, guard = shim.find_sorted(a, q)
        index = {int(x): i for i, x in enumerate(a)}
        eq(got, np.array([index.get(int(x), NOT_FOUND) for x in q], dtype=np.uint32), f"find_sorted n={n}")
        assert guard == FILL32


def ts_key(m, l, n):
    return (int(m), int(l) & IDENTITY_LSB, int(n))


def ts_columns(rng, n):
    """n Timestamps sorted by Timestamp order: msb on both sides of 2^63, nodes of both signs, neighbours that differ only
    in lsb bits outside IDENTITY_LSB (equal Timestamps), runs of equal ones at the start, the middle and the end"""
    msbs, idents, nodes = [5, (1 << 63) - 1, 1 << 63, (1 << 64) - 1], [0, 2, 0x1E], [-(1 << 31), -7, -1, 0, 1, 9, (1 << 31) - 1]
    ts = []
    for i in range(n):
        l = (int(rng.randint(0, 4)) << 16) | idents[rng.randint(0, len(idents))]
        ts.append((msbs[rng.randint(0, len(msbs))], l, nodes[rng.randint(0, len(nodes))]))
    r = max(1, min(4, n // 3)) if n else 0
    for s in ([0, n // 2, n - r] if n else []):
        for i in range(s, min(s + r, n)):
            ts[i] = ts[s]
    ts.sort(key=lambda t: ts_key(*t))
    # the same Timestamp with other non-identity lsb bits (the flag bits 0x0001 and 0xFFE0) on every other element
    ts = [(m, l | (0x0001 | 0x0FE0 if i % 2 else 0), nd) for i, (m, l, nd) in enumerate(ts)]
    return ts


@pytest.mark.parametrize("upper", [False, True])
def test_ts_bounds(shim, upper):
    rng = np.random.RandomState(17 + int(upper))
    for n in LENGTHS:
        ts = ts_columns(rng, n)
        keys = [ts_key(*t) for t in ts]
        assert keys == sorted(keys)
        cols = ([t[0] for t in ts], [t[1] for t in ts], [t[2] for t in ts])
        qs = list(ts) + [(m, l ^ 0x0021, nd) for m, l, nd in ts]                  # equal under IDENTITY_LSB
        qs += [(m, l, nd + 1) for m, l, nd in ts if nd < (1 << 31) - 1] + [(m, l + (1 << 16), nd) for m, l, nd in ts]
        qs += [(0, 0, 0), (0, 0, -(1 << 31)), ((1 << 64) - 1, (1 << 64) - 1, (1 << 31) - 1), (1 << 63, 0, -1), ((1 << 63) - 1, 0x1E, 1)]
        qcols = ([t[0] for t in qs], [t[1] for t in qs], [t[2] for t in qs])
        for lo, hi in windows(n):
            got, guard = shim.ts_bound(cols, np.full(len(qs), lo), np.full(len(qs), hi), qcols, upper)
            bis = bisect.bisect_right if upper else bisect.bisect_left
            want = [bis(keys, ts_key(*t), lo, hi) for t in qs]
            eq(got, np.array(want, dtype=np.uint32), f"{'upper' if upper else 'lower'}_bound_ts n={n} window [{lo}, {hi})")
            assert guard == FILL32
    # two elements that differ only outside IDENTITY_LSB are one Timestamp: the bounds span both
    cols = ([9, 9], [0x30000, 0x30000 | 0x0FE1], [-3, -3])
    lo_, _ = shim.ts_bound(cols, [0], [2], ([9], [0x30001], [-3]), False)
    up_, _ = shim.ts_bound(cols, [0], [2], ([9], [0x30001], [-3]), True)
    assert (int(lo_[0]), int(up_[0])) == (0, 2)


@pytest.mark.parametrize("upper", [False, True])
def test_wave_search(shim, upper):
    rng = np.random.RandomState(19 + int(upper))
    for n in LENGTHS + [63, 64, 65, 4096, 4097, 262145]:
        a = sorted_with_runs(rng, n, np.uint64)
        if n <= 257:
            q = queries_for(a, np.uint64)
        else:   # the ends, the runs, and a sample of elements with their neighbours: every probe position class
            pick = np.unique(np.concatenate([np.arange(0, 70), np.arange(n - 70, n), np.arange(n // 2 - 3, n // 2 + 8),
                                             rng.randint(0, n, size=300), np.arange(0, n, max(1, (n + 63) // 64))[:64]]))
            q = queries_for(a[pick], np.uint64)
        for lo, hi in windows(n):
            got, guard = shim.wave_search(a, np.full(len(q), lo), np.full(len(q), hi), q, upper)
            what = f"wave_search upper={upper} n={n} window [{lo}, {hi})"
            eq(got[:, 0], ref_bound(a, lo, hi, q, upper), what)
            assert (got == got[:, :1]).all(), f"{what}: the lanes of a wave disagree"
            assert guard == FILL32, f"{what}: guard element overwritten"
