"""Plain numpy references of the primitives in csrc/prims.hpp, a few lines each; pinned by tests/test_prims_model.py
with hand-written literals and compared with the HIP primitives by tests/test_prims_gpu.py."""
import numpy as np

M64 = (1 << 64) - 1


def scan(x, op, exclusive):
    """(prefixes, total) of x under op ("add" wraps in x's dtype, "max" over unsigned values); identity 0."""
    x = np.asarray(x)
    incl = np.cumsum(x, dtype=x.dtype) if op == "add" else np.maximum.accumulate(x) if len(x) else x.copy()
    total = incl[-1] if len(x) else x.dtype.type(0)
    if not exclusive:
        return incl, total
    excl = np.zeros_like(x)
    excl[1:] = incl[:-1]
    return excl, total


def field(keys, lo, bits):
    """(key >> lo) & (2^bits - 1)"""
    keys = np.asarray(keys, dtype=np.uint64)
    if bits <= 0:
        return np.zeros_like(keys)
    f = keys >> np.uint64(lo) if lo else keys
    return f & np.uint64((1 << bits) - 1) if bits < 64 else f


def stable_order(keys, lo, bits):
    """the permutation of a stable sort on bits [lo, lo + bits)"""
    return np.argsort(field(keys, lo, bits), kind="stable")


def sort_pairs(keys, vals, bits):
    """radix_sort: (keys, vals) in the stable order of the low `bits` bits; vals None = the index"""
    keys = np.asarray(keys, dtype=np.uint64)
    vals = np.arange(len(keys), dtype=np.uint32) if vals is None else np.asarray(vals, dtype=np.uint32)
    o = stable_order(keys, 0, bits)
    return keys[o], vals[o]


def sort_keys(keys, lo, bits):
    """radix_sort_keys: whole keys in the stable order of bits [lo, lo + bits)"""
    keys = np.asarray(keys, dtype=np.uint64)
    return keys[stable_order(keys, lo, bits)]


def pext(w, mask):
    """the bits of w under mask, packed to the low end, bit by bit"""
    o = b = 0
    for i in range(64):
        if (mask >> i) & 1:
            o |= ((int(w) >> i) & 1) << b
            b += 1
    return o


def runs_of(mask):
    """the maximal runs of ones of mask as (lo, length), ascending"""
    r, i = [], 0
    while i < 64:
        if not (mask >> i) & 1:
            i += 1
            continue
        j = i
        while j < 64 and (mask >> j) & 1:
            j += 1
        r.append((i, j - i))
        i = j
    return r


MAX_RUNS = 12


def plan_mask(mask):
    """the mask make_runs really extracts: mask itself up to MAX_RUNS runs, its hull [lowest, highest set bit] past that"""
    r = runs_of(mask)
    if len(r) <= MAX_RUNS:
        return mask
    lo, hi = r[0][0], r[-1][0] + r[-1][1]
    return ((1 << hi) - 1) & ~((1 << lo) - 1) & M64


def pext_runs(w, mask):
    """(pext over the planned mask, Runs.bits)"""
    m = plan_mask(mask)
    return pext(w, m), bin(m).count("1")


def owners(off, pos):
    """own[p] = the run k with off[k] <= pos[p] < off[k + 1] among the NON-EMPTY runs of the ascending offsets off
    (a position past the last run belongs to the last non-empty one, one before the first to run 0)"""
    off = np.asarray(off, dtype=np.uint64)
    ne = np.flatnonzero(off[1:] > off[:-1])
    if len(ne) == 0:
        return np.zeros(len(pos), dtype=np.uint32)
    k = np.searchsorted(off[ne], np.asarray(pos, dtype=np.uint64), "right") - 1
    return np.where(k >= 0, ne[np.maximum(k, 0)], 0).astype(np.uint32)
