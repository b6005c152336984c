"""The primitives of csrc/prims.hpp on their own, at their own edges, against the numpy references of prims_model.py:
the look-back scan, the radix sorts (one-sweep and three-launch) and the block / wave helpers, through the test shim
libaccord_prims_test.so (csrc/prims_test.hip, bound by prims_shim.py). Every comparison is exact equality.

Sizes sit on the kernels' own tiles: scan_multi's 8192 (u32) / 4096 (u64) elements, the sort's 1024 elements below
rs_small_n() = 262,144 and 4096 from there up. Sequences on one context exercise the double-buffered status words (a scan
zeroes the other buffer of its lane, a sort's histogram kernel the words its tag's previous sort dirtied).

No caller scans in place (no scan / scan_multi call in csrc/ passes the same array as in and out), so in-place scans are
not a case here. u64 scan values stay below 2^62, the documented precondition: larger ones would corrupt the status flags.
"""
import numpy as np
import pytest

import prims_model as M
from prims_shim import (FILL64, SCAN_TYPES, TOT_CSR, TOT_NONE, TOT_WORD, U32ADD, U32MAX, U64ADD, U64MAX, Shim,
                        fill_of, scan_tile)

pytestmark = pytest.mark.gpu

ACC_E_STATE = -2
RS_SMALL_N = 262144


def _open():
    from accord_amd.deps import Context
    c = Context(0)
    return c, Shim(c)


@pytest.fixture(scope="module")
def shim():
    c, s = _open()
    yield s
    s.close()
    c.close()


@pytest.fixture()
def fresh():
    """a context of its own: the status buffers start unallocated, so a sequence's sizes alone decide their history"""
    c, s = _open()
    yield s
    s.close()
    c.close()


def eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: first difference at {i} of {len(want)}: got {got[i]}, want {want[i]}")


# ---------------------------------------------------------------- scan

def scan_sizes(t):
    T = scan_tile(t)
    return [1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T, 64 * T, 64 * T + 1, 65 * T + 3, 1100 * T + 5]


def scan_values(rng, t, n):
    """random values whose running total stays below 2^62 (u64) or wraps (u32 add: that is its contract)"""
    dt, op = SCAN_TYPES[t]
    if dt == np.uint32:
        return rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if op == "max":
        return rng.randint(0, 1 << 62, size=n, dtype=np.uint64)
    return rng.randint(0, (1 << 62) // n, size=n, dtype=np.uint64)


def check_scan(shim, t, x, exclusive, tot_mode, side_lane=False, what=""):
    dt, op = SCAN_TYPES[t]
    x = np.asarray(x, dtype=dt)
    n = len(x)
    want, total = M.scan(x, op, exclusive)
    out, word = shim.scan(t, x, exclusive, tot_mode, side_lane)
    what = f"scan type {t} n={n} exclusive={exclusive} total mode {tot_mode} lane={int(side_lane)} {what}"
    eq(out[:n], want, what)
    assert out[n] == (total if tot_mode == TOT_CSR else fill_of(dt)), f"{what}: out[n] = {out[n]}, total {total}"
    assert word == (total if tot_mode == TOT_WORD else fill_of(dt)), f"{what}: total word = {word}, total {total}"


@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("t", [U32ADD, U32MAX, U64ADD, U64MAX])
def test_scan_random_at_tile_edges(shim, t, exclusive):
    rng = np.random.RandomState(100 + t)
    for i, n in enumerate(scan_sizes(t)):
        x = scan_values(rng, t, n)
        # every total mode at every size but the largest, which takes one (a different one per instantiation)
        for mode in ([TOT_NONE, TOT_WORD, TOT_CSR] if i + 1 < len(scan_sizes(t)) else [(t + exclusive) % 3]):
            check_scan(shim, t, x, exclusive, mode)


@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("t", [U32ADD, U32MAX, U64ADD, U64MAX])
def test_scan_sparse_data(shim, t, exclusive):
    """all identity; one non-identity value at element 0 (its prefix travels through every tile), at a tile's last
    element and at n - 1; for max, a maximum at element 0 over smaller random values"""
    dt, op = SCAN_TYPES[t]
    T = scan_tile(t)
    rng = np.random.RandomState(200 + t)
    big = (1 << 32) - 1 if dt == np.uint32 else (1 << 62) - 1
    for n in [1, 257, T, T + 1, 2 * T, 64 * T + 1, 65 * T + 3, 130 * T + 1]:
        check_scan(shim, t, np.zeros(n, dt), exclusive, TOT_WORD, what="all identity")
        for at in sorted(a for a in {0, T - 1, n - 1, (n - 1) // T * T - 1} if 0 <= a < n):
            for v in (1, big):
                x = np.zeros(n, dt)
                x[at] = v
                check_scan(shim, t, x, exclusive, TOT_CSR, what=f"single {v} at {at}")
        if op == "max":
            x = scan_values(rng, t, n) >> dt(1)
            x[0] = big
            check_scan(shim, t, x, exclusive, TOT_WORD, what="maximum first")


def test_scan_value_limits(shim):
    rng = np.random.RandomState(7)
    for T, t in ((4096, U64MAX), (4096, U64ADD), (8192, U32MAX), (8192, U32ADD)):
        n = 65 * T + 3
        for exclusive in (False, True):
            if t == U64MAX:      # values up to exactly 2^62 - 1, the largest a status word holds
                x = rng.randint(0, 1 << 62, size=n, dtype=np.uint64)
                x[n // 2] = (1 << 62) - 1
            elif t == U64ADD:    # a total of exactly 2^62 - 1
                x = np.full(n, ((1 << 62) - 1) // n, np.uint64)
                x[-1] += np.uint64(((1 << 62) - 1) % n)
                assert int(x.sum(dtype=np.uint64)) == (1 << 62) - 1
            elif t == U32MAX:
                x = rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
                x[T + 1] = 0xFFFFFFFF
            else:                # a u32 add-scan wraps (many times here), as numpy's cumsum in uint32 does
                x = rng.randint(1 << 31, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
            for mode in (TOT_WORD, TOT_CSR):
                check_scan(shim, t, x, exclusive, mode, what="value limits")
            if t == U32ADD:      # ... and sum_u32 beside it gives the true total
                true = int(x.sum(dtype=np.uint64))
                assert true > 1 << 32
                assert shim.sum_u32(x) == (true, FILL64)


def test_sum_u32(shim):
    rng = np.random.RandomState(8)
    assert shim.sum_u32(np.zeros(0, np.uint32)) == (0, FILL64)
    # one block, a partial block, exactly the 1024-block grid, past it (blocks stride), all zero (no atomic at all)
    for n in [1, 255, 256, 257, 1024 * 256 - 1, 1024 * 256, 1024 * 256 + 1, 3 * 1024 * 256 + 77]:
        for x in (rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32), np.full(n, 0xFFFFFFFF, np.uint32),
                  np.zeros(n, np.uint32)):
            assert shim.sum_u32(x) == (int(x.sum(dtype=np.uint64)), FILL64), f"sum_u32 n={n}"


def seq_sizes(t):
    T = scan_tile(t)
    return [65 * T + 3, 1, T + 1, 1100 * T + 5, 2, 64 * T]


def run_scan_sequence(s, types, lanes, rng):
    """scans of shrinking and growing sizes, forwards and backwards: call i is of type types[i % ..] on lane lanes[i % ..]"""
    i = 0
    for sizes in (lambda t: seq_sizes(t), lambda t: seq_sizes(t)[::-1]):
        for j in range(6):
            t = types[i % len(types)]
            n = sizes(t)[j]
            check_scan(s, t, scan_values(rng, t, n), bool(i & 1) ^ bool(i & 4), (TOT_WORD, TOT_CSR, TOT_NONE)[i % 3],
                       side_lane=bool(lanes[i % len(lanes)]), what=f"sequence step {i}")
            i += 1


@pytest.mark.parametrize("types", [[U32ADD], [U32MAX], [U64ADD], [U64MAX], [U64ADD, U32ADD, U64MAX]],
                         ids=["u32add", "u32max", "u64add", "u64max", "mixed"])
def test_scan_sequence_on_one_context(fresh, types):
    """the status buffers are per lane, shared by every instantiation: sizes (and with them the ticket word at
    status + nb) shrink and grow from call to call"""
    run_scan_sequence(fresh, types, [0], np.random.RandomState(31))


@pytest.mark.parametrize("lanes", [[0, 1], [1, 0], [1], [0, 0, 1]], ids=["main-side", "side-main", "side", "two-one"])
def test_scan_sequence_across_lanes(fresh, lanes):
    """the side lane (aux[0] between lane_fork and lane_join) has status buffers and a parity of its own"""
    run_scan_sequence(fresh, [U64ADD, U32ADD], lanes, np.random.RandomState(32))


def test_scan_sequence_after_a_refused_call(fresh):
    rng = np.random.RandomState(33)
    T = scan_tile(U64ADD)
    check_scan(fresh, U64ADD, scan_values(rng, U64ADD, 3 * T + 1), True, TOT_WORD)   # leaves one buffer dirty
    for lane in (0, 1):
        xs = [np.ones(5, np.uint64)] * 6
        rc, _, _ = fresh.scan_multi_rc(U64ADD, xs, True, [TOT_NONE] * 6, side_lane=bool(lane))
        assert rc == ACC_E_STATE
        rc, _, _ = fresh.scan_multi_rc(U64ADD, [], True, [], side_lane=bool(lane))
        assert rc == ACC_E_STATE
    run_scan_sequence(fresh, [U64ADD, U32MAX], [0, 1], rng)


def multi_tuples(T):
    big = 70 * T + 9
    return [(T + 1,), (0,), (big,),
            (0, T), (T, 0), (big, 1),
            (1, 0, T + 1), (0, 0, 0), (T, T + 1, big),
            (0, T + 1, 0, 1), (big, 0, T, T), (1, 1, 0, 0),
            (0, 1, T, T + 1, big), (big, T + 1, 0, 0, 1), (T, 0, T + 1, 0, 0), (0, 0, 0, 0, 0), (1, 1, 1, 1, 1),
            (0, 0, 0, 0, T - 1)]


@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("t", [U32ADD, U64ADD, U64MAX])
def test_scan_multi(shim, t, exclusive):
    """k = 1 .. 5 arrays in one launch, zero-length ones first, in the middle and last; totals as a separate word, at
    out + n (the callers' CSR idiom) or not at all, per array; consecutive launches with different tuples"""
    dt, op = SCAN_TYPES[t]
    rng = np.random.RandomState(300 + t)
    modes = [TOT_WORD, TOT_NONE, TOT_CSR, TOT_WORD, TOT_CSR, TOT_NONE, TOT_NONE]
    for q, ns in enumerate(multi_tuples(scan_tile(t))):
        for tm in ([modes[(q + i) % len(modes)] for i in range(len(ns))], [TOT_NONE] * len(ns)):
            xs = [scan_values(rng, t, n) if n else np.zeros(0, dt) for n in ns]
            outs, tots = shim.scan_multi(t, xs, exclusive, tm, side_lane=(q % 5 == 4))
            for i, (x, out, n) in enumerate(zip(xs, outs, ns)):
                want, total = M.scan(x, op, exclusive)     # a zero-length array's total is 0
                what = f"scan_multi type {t} exclusive={exclusive} lengths {ns} modes {tm} array {i}"
                eq(out[:n], want, what)
                assert out[n] == (total if tm[i] == TOT_CSR else fill_of(dt)), f"{what}: out[n] = {out[n]}"
                assert tots[i] == (total if tm[i] == TOT_WORD else fill_of(dt)), f"{what}: total word = {tots[i]}"


# ---------------------------------------------------------------- radix sort

SORT_BITS = [0, 1, 7, 8, 9, 16, 33, 64]
SORT_SMALL = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5 * 1024 + 7]
SORT_LARGE = [RS_SMALL_N - 1, RS_SMALL_N, RS_SMALL_N + 1, 800 * 4096 + 11]
# past the BLOCK * 8 = 2048 tiles one trip of the three-launch sort's column scan covers (the numpy reference sorts
# these 8.4M keys in about 1.2 s)
SORT_3L_LARGE = 2049 * 4096 + 5
DISTS = ["uniform", "three", "equal", "sorted", "reverse", "digit", "tied"]


def sort_keys_for(rng, dist, n, bits):
    """keys with every bit above `bits` zero"""
    mask = np.uint64((1 << bits) - 1)
    r = rng.randint(0, 1 << 63, size=n, dtype=np.uint64) << np.uint64(1) | rng.randint(0, 2, size=n, dtype=np.uint64)
    if dist == "uniform":
        k = r
    elif dist == "three":
        k = np.array([0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x0123456789ABCDEE], np.uint64)[rng.randint(0, 3, size=n)]
    elif dist in ("equal", "tied"):      # (all sorted bits equal = all equal here: no key bit lies outside them)
        k = np.full(n, 0xA5A5A5A5A5A5A5A5 if dist == "equal" else 0, np.uint64)
    elif dist == "sorted":
        k = np.sort(r & mask)
    elif dist == "reverse":
        k = np.sort(r & mask)[::-1].copy()
    else:                                # "digit": the second digit constant, the others random
        k = (r & ~np.uint64(0xFF00)) | np.uint64(0x5A00)
    return k & mask


def check_sort(shim, tag, keys, vals, bits, three, what):
    wk, wv = M.sort_pairs(keys, vals, bits)
    gk, gv = shim.radix_sort(tag, keys, vals, bits, three_launch=three)
    what = f"radix_sort{'_3launch' if three else ''} n={len(keys)} bits={bits} vals={'given' if vals is not None else 'iota'} {what}"
    eq(gk, wk, what + " keys")
    eq(gv, wv, what + " vals")     # the stable order: a correct but unstable sort fails here
    return wk, wv


@pytest.mark.parametrize("n", SORT_SMALL)
@pytest.mark.parametrize("three", [False, True], ids=["onesweep", "3launch"])
def test_radix_sort_small(shim, three, n):
    rng = np.random.RandomState(400 + n)
    for bits in SORT_BITS:
        for dist in DISTS:
            keys = sort_keys_for(rng, dist, n, bits)
            check_sort(shim, "pt_s", keys, rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32), bits, three, dist)
            check_sort(shim, "pt_s", keys, None, bits, three, dist)


@pytest.mark.parametrize("bits", SORT_BITS)
@pytest.mark.parametrize("n", SORT_LARGE)
def test_radix_sort_large_bits(shim, n, bits):
    """around rs_small_n() the tile changes from 1024 to 4096 elements; 800 tiles of 4096 are more than are resident"""
    rng = np.random.RandomState(500 + bits)
    keys = sort_keys_for(rng, "uniform", n, bits)
    check_sort(shim, "pt_l", keys, rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32), bits, False, "uniform")
    check_sort(shim, "pt_l", keys, None, bits, False, "uniform")


@pytest.mark.parametrize("dist", DISTS[1:])
@pytest.mark.parametrize("n", SORT_LARGE)
def test_radix_sort_large_distributions(shim, n, dist):
    rng = np.random.RandomState(600)
    keys = sort_keys_for(rng, dist, n, 24)
    check_sort(shim, "pt_l", keys, rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32), 24, False, dist)
    check_sort(shim, "pt_l", keys, None, 24, False, dist)


@pytest.mark.parametrize("dist,bits,iota", [("uniform", 33, False), ("three", 16, True), ("digit", 24, True)])
def test_radix_sort_3launch_past_one_column_trip(shim, dist, bits, iota):
    rng = np.random.RandomState(700)
    n = SORT_3L_LARGE
    keys = sort_keys_for(rng, dist, n, bits)
    vals = None if iota else rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    check_sort(shim, "pt_3", keys, vals, bits, True, dist)


@pytest.mark.parametrize("three", [False, True], ids=["onesweep", "3launch"])
def test_radix_sort_3launch_multi_tile(shim, three):
    """a few hundred 4096-element tiles through both routes: the same input, the same answer"""
    rng = np.random.RandomState(701)
    for n in (300 * 4096 + 1, 301 * 4096 - 1):
        for bits in (9, 40):
            keys = sort_keys_for(rng, "uniform", n, bits)
            check_sort(shim, "pt_3", keys, None, bits, three, "uniform")


TAG_SIZES = [800 * 4096 + 11, 5, RS_SMALL_N, 1025, 300000, 1]


def test_radix_sort_tag_sequences(fresh):
    """sorts of shrinking and growing sizes on one tag (each zeroes the status words the one before dirtied), then on two
    tags in turn: each tag's last result stays readable while the other tag sorts"""
    rng = np.random.RandomState(800)
    for i, n in enumerate(TAG_SIZES + TAG_SIZES[::-1]):
        bits = (24, 9, 33)[i % 3]
        vals = None if i & 1 else rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        check_sort(fresh, "pt_a", sort_keys_for(rng, "uniform", n, bits), vals, bits, False, f"one tag, step {i}")
    for i, (na, nb) in enumerate(zip(TAG_SIZES, TAG_SIZES[::-1])):
        wa = check_sort(fresh, "pt_a", sort_keys_for(rng, "uniform", na, 24), None, 24, False, f"tag a, step {i}")
        wb = check_sort(fresh, "pt_b", sort_keys_for(rng, "digit", nb, 17), None, 17, False, f"tag b, step {i}")
        kc = field_keys(rng, "uniform", nb, 8, 32)       # a keys-only sort on a third tag between
        eq(fresh.radix_sort_keys("pt_c", kc, 8, 32), M.sort_keys(kc, 8, 32), f"tag c, step {i}")
        for tag, (wk, wv) in (("pt_a", wa), ("pt_b", wb)):
            gk, gv = fresh.sort_result(tag, len(wk))
            eq(gk, wk, f"tag {tag} read again, step {i}, keys")
            eq(gv, wv, f"tag {tag} read again, step {i}, vals")


KEY_FIELDS = [(0, 8), (20, 12), (32, 32), (13, 9), (40, 24), (0, 64)]


def field_keys(rng, dist, n, lo, bits):
    """random bits below lo (they ride along), the field in [lo, lo + bits), zero above"""
    f = sort_keys_for(rng, dist, n, bits)
    low = rng.randint(0, 1 << 62, size=n, dtype=np.uint64) & np.uint64((1 << lo) - 1)
    return (f << np.uint64(lo)) | low if lo else f


@pytest.mark.parametrize("n", SORT_SMALL)
def test_radix_sort_keys_small(shim, n):
    rng = np.random.RandomState(900 + n)
    for lo, bits in KEY_FIELDS + [(0, 0), (17, 0)]:      # bits = 0: the copy path
        for dist in DISTS:
            keys = field_keys(rng, dist, n, lo, bits)
            eq(shim.radix_sort_keys("pt_k", keys, lo, bits), M.sort_keys(keys, lo, bits),
               f"radix_sort_keys n={n} lo={lo} bits={bits} {dist}")


@pytest.mark.parametrize("lo,bits", KEY_FIELDS)
@pytest.mark.parametrize("n", SORT_LARGE)
def test_radix_sort_keys_large(shim, n, lo, bits):
    rng = np.random.RandomState(1000 + lo)
    for dist in ("uniform", "tied"):      # tied: the field equal in every key, so the low bits keep their input order
        keys = field_keys(rng, dist, n, lo, bits)
        eq(shim.radix_sort_keys("pt_kl", keys, lo, bits), M.sort_keys(keys, lo, bits),
           f"radix_sort_keys n={n} lo={lo} bits={bits} {dist}")


# ---------------------------------------------------------------- block and wave primitives

@pytest.mark.parametrize("t", [U32ADD, U32MAX, U64ADD, U64MAX])
def test_block_exclusive(shim, t):
    dt, op = SCAN_TYPES[t]
    rng = np.random.RandomState(1100 + t)
    top = int(np.iinfo(dt).max)
    cases = [rng.randint(0, 1 << 62, size=768, dtype=np.uint64).astype(dt), np.zeros(768, dt), np.full(768, top, dt),
             (rng.randint(0, 1 << 62, size=768, dtype=np.uint64) >> np.uint64(40)).astype(dt)]
    for at in (0, 63, 64, 255, 256 + 127, 512 + 192):      # one value: first / last lane of a wave, of the block
        x = np.zeros(768, dt)
        x[at] = top
        cases.append(x)
    for q, x in enumerate(cases):
        out, tot = shim.block_exclusive(t, x)
        for b in range(3):
            want, total = M.scan(x[256 * b:256 * b + 256], op, True)      # (wraps in the element type, as the kernel does)
            eq(out[256 * b:256 * b + 256], want, f"block_exclusive type {t} case {q} block {b}")
            assert tot[b] == total, f"block_exclusive type {t} case {q} block {b}: total {tot[b]} vs {total}"


@pytest.mark.parametrize("dt", [np.uint32, np.uint64])
def test_bitonic_reg(shim, dt):
    rng = np.random.RandomState(1200)
    hi = dt(1) << dt(np.dtype(dt).itemsize * 8 - 1)
    rnd = rng.randint(0, 1 << 63, size=512, dtype=np.uint64).astype(dt) | (rng.randint(0, 2, size=512).astype(dt) * hi)
    dup = rng.randint(0, 4, size=512).astype(dt) | (rng.randint(0, 2, size=512).astype(dt) * hi)
    srt = np.sort(rnd.reshape(8, 64), axis=1).reshape(-1)
    rev = srt.reshape(8, 64)[:, ::-1].reshape(-1).copy()
    for name, x in (("random", rnd), ("duplicates", dup), ("sorted", srt), ("reversed", rev), ("equal", np.full(512, hi | dt(7)))):
        eq(shim.bitonic_reg(x), np.sort(x.reshape(8, 64), axis=1).reshape(-1), f"bitonic_reg {np.dtype(dt).name} {name}")


@pytest.mark.parametrize("n2", [1 << s for s in range(1, 14)])
@pytest.mark.parametrize("where", ["lds-u32", "global-u32", "global-u64"])
def test_block_bitonic(shim, where, n2):
    dt = np.uint64 if where.endswith("u64") else np.uint32
    rng = np.random.RandomState(1300 + n2)
    top = np.dtype(dt).itemsize * 8
    for name, x in (("random", rng.randint(0, 1 << 63, size=3 * n2, dtype=np.uint64).astype(dt) | dt(1 << (top - 1))),
                    ("duplicates", rng.randint(0, 5, size=3 * n2).astype(dt) << dt(top - 3)),
                    ("reversed", np.arange(3 * n2, 0, -1).astype(dt))):
        out, guard = shim.block_bitonic(x, n2, where.startswith("lds"))
        eq(out, np.sort(x.reshape(3, n2), axis=1).reshape(-1), f"block_bitonic {where} n2={n2} {name}")
        assert guard == fill_of(dt)


CH = 8 * 256      # chunk_owners<8>: the positions of one chunk


def owner_cases():
    rng = np.random.RandomState(1400)
    yield "one run over four chunks", [5, 5 + 3 * CH + 17]
    yield "one run of one element", [9, 10]
    yield "empty runs between", [10, 13, 13, 15, 15, 15, 18]
    yield "several runs start at one position", [100, 100, 100, 100, 130, 130, 130, 5000, 5000]
    yield "a run starts at a chunk boundary", [0, CH, CH, 2 * CH + 5, 2 * CH + 5, 3 * CH, 3 * CH + 1]
    yield "runs start at boundaries of a shifted range", [1 << 40, (1 << 40) + CH, (1 << 40) + 2 * CH, (1 << 40) + 2 * CH + 1]
    yield "a run spans three chunks", [0, 10, 10 + 2 * CH + 100, 10 + 2 * CH + 101, 3 * CH + 7]
    yield "leading and trailing empty runs", [7, 7, 7, 9, 9, 9]
    yield "all runs empty", [4, 4, 4]
    yield "BLOCK runs of one element", list(range(33, 33 + 257))
    yield "BLOCK runs of 8: exactly one chunk", list(range(0, 8 * 256 + 1, 8))
    yield "BLOCK runs of 9: one element past a chunk", list(range(0, 9 * 256 + 1, 9))
    for q in range(4):      # BLOCK runs, many of them empty, from a large base offset
        lens = rng.choice([0, 0, 0, 1, 7, 100, 2048, 2049][:5 + q], size=256)
        yield f"random {q}", (np.concatenate([[0], np.cumsum(lens)]) + (q << 33) + q).tolist()
    lens = np.zeros(256, np.int64)
    lens[[0, 255]] = [1, 3 * CH]
    yield "first and last of BLOCK runs", np.concatenate([[0], np.cumsum(lens)]).tolist()


@pytest.mark.parametrize("name,off", list(owner_cases()), ids=[n for n, _ in owner_cases()])
def test_chunk_owners(shim, name, off):
    """position by position over consecutive chunks, the carry from chunk to chunk included"""
    off = np.asarray(off, dtype=np.uint64)
    own, carry = shim.chunk_owners(off)
    nch = len(carry)
    assert nch == -(-(int(off[-1]) - int(off[0])) // CH)
    pos = int(off[0]) + np.arange(nch * CH, dtype=np.uint64)
    want = M.owners(off, pos)      # (past off[nt], in the last chunk: the last non-empty run, what a max-scan leaves)
    eq(own, want, f"chunk_owners {name}")
    eq(carry, want[CH - 1::CH], f"chunk_owners {name} carries")


def pext_masks():
    rng = np.random.RandomState(1500)
    m12 = sum(1 << (3 + 4 * i) for i in range(12))
    masks = [0, M.M64, 1, 1 << 63, m12, m12 | 1 << 51, m12 | 1 << 63, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA,
             0x00FF00FF00FF00FF, 0x8000000000000001, 0xFFFFFFFF00000000, 0x7FFFFFFFFFFFFFFE]
    for _ in range(24):
        a, b, c = (int(x) for x in rng.randint(0, 1 << 63, size=3, dtype=np.uint64) * 2 + rng.randint(0, 2, size=3).astype(np.uint64))
        masks += [a, a & b, a | b | c]
    return masks


def test_pext_runs(shim):
    rng = np.random.RandomState(1501)
    w = np.concatenate([rng.randint(0, 1 << 63, size=500, dtype=np.uint64) * np.uint64(2) + rng.randint(0, 2, size=500).astype(np.uint64),
                        np.array([0, M.M64, 1, 1 << 63], np.uint64)])
    counts = set()
    for mask in pext_masks():
        nruns = len(M.runs_of(mask))
        counts.add(min(nruns, 13))
        out, bits, n = shim.pext_runs(mask, w)
        want = np.array([M.pext_runs(int(x), mask)[0] for x in w], np.uint64)
        what = f"pext_runs mask {mask:#018x} ({nruns} runs)"
        assert bits == M.pext_runs(0, mask)[1] and n == (nruns if nruns <= 12 else 1), f"{what}: bits {bits}, runs {n}"
        eq(out, want, what)
        if nruns <= 12:      # the true pext
            assert bits == bin(mask).count("1")
            eq(out, np.array([M.pext(int(x), mask) for x in w], np.uint64), what + " against pext")
        # order preserving on the masked words, in every case (past 12 runs the hull's extra bits are zero in them):
        # equal where they are equal, less where they are less
        mw = np.sort(w & np.uint64(mask))
        po, _, _ = shim.pext_runs(mask, mw)
        eq(po, np.array([M.pext_runs(int(x), mask)[0] for x in mw], np.uint64), what + " masked words")
        assert np.array_equal(mw[1:] == mw[:-1], po[1:] == po[:-1]) and np.all(po[1:] >= po[:-1]), what + " order"
    assert {0, 1, 12, 13} <= counts
