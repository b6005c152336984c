"""Pins tests/prims_model.py (the numpy references of csrc/prims.hpp's primitives) with hand-written literals."""
import numpy as np

import prims_model as M


def test_scan_add_wraps_in_the_element_type():
    x = np.array([0xFFFFFFF0, 0x20, 5], dtype=np.uint32)
    incl, total = M.scan(x, "add", False)
    assert incl.tolist() == [0xFFFFFFF0, 0x10, 0x15] and int(total) == 0x15 and incl.dtype == np.uint32
    excl, total = M.scan(x, "add", True)
    assert excl.tolist() == [0, 0xFFFFFFF0, 0x10] and int(total) == 0x15
    y = np.array([1 << 61, 1 << 61, 7], dtype=np.uint64)   # no wrap in u64 below 2^62
    assert M.scan(y, "add", False)[0].tolist() == [1 << 61, 1 << 62, (1 << 62) + 7]


def test_scan_max_and_empty():
    x = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint64)
    incl, total = M.scan(x, "max", False)
    assert incl.tolist() == [3, 3, 4, 4, 5, 9, 9, 9] and int(total) == 9
    excl, total = M.scan(x, "max", True)
    assert excl.tolist() == [0, 3, 3, 4, 4, 5, 9, 9] and int(total) == 9
    for op in ("add", "max"):
        out, total = M.scan(np.zeros(0, np.uint32), op, True)
        assert len(out) == 0 and int(total) == 0


def test_stable_sort_keeps_ties_in_input_order():
    keys = np.array([2, 1, 2, 0, 1, 2], dtype=np.uint64)
    vals = np.array([10, 11, 12, 13, 14, 15], dtype=np.uint32)
    k, v = M.sort_pairs(keys, vals, 2)
    assert k.tolist() == [0, 1, 1, 2, 2, 2] and v.tolist() == [13, 11, 14, 10, 12, 15]
    k, v = M.sort_pairs(keys, None, 2)
    assert v.tolist() == [3, 1, 4, 0, 2, 5]
    k, v = M.sort_pairs(keys, vals, 0)   # no sorted bit: the input order
    assert k.tolist() == keys.tolist() and v.tolist() == vals.tolist()


def test_sort_keys_on_a_field_carries_the_low_bits():
    # field = bits [4, 8): 0xA, 0x3, 0xA, 0x3; the low nibble rides along, bit 8 and up are outside (lo + bits = 8)
    keys = np.array([0xA7, 0x39, 0xA1, 0x30], dtype=np.uint64)
    assert M.sort_keys(keys, 4, 4).tolist() == [0x39, 0x30, 0xA7, 0xA1]
    assert M.field(keys, 4, 4).tolist() == [0xA, 0x3, 0xA, 0x3]
    assert M.field(np.array([M.M64], dtype=np.uint64), 0, 64).tolist() == [M.M64]
    assert M.field(np.array([M.M64], dtype=np.uint64), 13, 9).tolist() == [0x1FF]


def test_pext_literals():
    assert M.pext(0b1011_0110, 0b1100_1010) == 0b1001          # bits 1, 3, 6, 7 of w: 1, 0, 0, 1
    assert M.pext(0xDEADBEEFCAFEF00D, M.M64) == 0xDEADBEEFCAFEF00D
    assert M.pext(0xDEADBEEFCAFEF00D, 0) == 0
    assert M.pext(1 << 63, 1 << 63) == 1
    assert M.pext_runs(0x1234_5678_9ABC_DEF0, M.M64) == (0x1234_5678_9ABC_DEF0, 64)
    assert M.pext_runs(0xFF00, 0x0F00) == (0xF, 4)


def test_pext_runs_past_twelve_runs_is_pext_over_the_hull():
    m12 = sum(1 << (3 + 4 * i) for i in range(12))     # 12 single-bit runs: bits 3, 7, ..., 47
    m13 = m12 | 1 << 51                                # 13 runs: hull = bits [3, 51]
    assert len(M.runs_of(m12)) == 12 and len(M.runs_of(m13)) == 13
    assert M.plan_mask(m12) == m12
    hull = ((1 << 52) - 1) & ~0b111
    assert M.plan_mask(m13) == hull
    w = 0x0123_4567_89AB_CDEF
    assert M.pext_runs(w, m12) == (M.pext(w, m12), 12)
    assert M.pext_runs(w, m13) == ((w >> 3) & ((1 << 49) - 1), 49)
    assert M.pext(w, m13) != M.pext_runs(w, m13)[0]
    assert M.runs_of(0b0110_0001) == [(0, 1), (5, 2)] and M.runs_of(M.M64) == [(0, 64)] and M.runs_of(0) == []


def test_owner_map_skips_empty_runs():
    #        run: 0      1 (empty)  2       3 (empty) 4 (empty) 5
    off = [10, 13, 13, 15, 15, 15, 18]
    pos = np.arange(10, 18)
    assert M.owners(off, pos).tolist() == [0, 0, 0, 2, 2, 5, 5, 5]
    assert M.owners(off, [18, 40]).tolist() == [5, 5]             # past the end: the last non-empty run
    assert M.owners([7, 7, 7, 9], [7, 8]).tolist() == [2, 2]      # leading empty runs
    assert M.owners([4, 4, 4], [4]).tolist() == [0]               # all empty
