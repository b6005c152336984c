"""ctypes binding of the test shim over csrc/prims.hpp and csrc/search.hpp (accord_amd/libaccord_prims_test.so, csrc/prims_test.hip): numpy
arrays in, numpy arrays out, on a context of the main library. A missing library or symbol raises: nothing here skips.

ACC_PRIMS_TEST_LIB names another build of the shim (a deliberately mutated prims.hpp, to see which test notices)."""
import ctypes as C
import os

import numpy as np

from accord_amd import _lib

LIB_PATH = os.environ.get("ACC_PRIMS_TEST_LIB") or os.path.join(_lib.HERE, "libaccord_prims_test.so")

U32ADD, U32MAX, U64ADD, U64MAX = 0, 1, 2, 3
SCAN_TYPES = {U32ADD: (np.uint32, "add"), U32MAX: (np.uint32, "max"), U64ADD: (np.uint64, "add"), U64MAX: (np.uint64, "max")}
TOT_NONE, TOT_WORD, TOT_CSR = 0, 1, 2
FILL32, FILL64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
BLOCK = 256


def scan_tile(scan_type):
    """elements per tile of scan_multi's kernel for that element type"""
    return 8192 if SCAN_TYPES[scan_type][0] == np.uint32 else 4096


def fill_of(dtype):
    return np.dtype(dtype).type(FILL32 if np.dtype(dtype).itemsize == 4 else FILL64)


_SIGS = {
    "acct_scan": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_int],
    "acct_scan_multi": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                        C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_int],
    "acct_sum_u32": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p],
    "acct_radix_sort": [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "acct_radix_sort_keys": [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p],
    "acct_sort_result": [C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)],
    "acct_block_exclusive": [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "acct_bitonic_reg": [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p],
    "acct_block_bitonic": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "acct_chunk_owners": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p],
    "acct_pext_runs": [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "acct_search_bound": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_uint32, C.c_void_p],
    "acct_seg_of": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p],
    "acct_find_sorted": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p],
    "acct_ts_bound": [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p],
    "acct_wave_search": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p],
}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Shim:
    """The shim's entry points on one context (accord_amd.deps.Context). rc != ACC_OK raises through ctx.check, except
    where a method says it returns the code."""

    def __init__(self, ctx):
        _lib.load()                       # the main library (and the HIP runtime it shares with torch) first
        self.ctx = ctx
        self.h = ctx._h
        self.lib = C.CDLL(LIB_PATH)       # OSError if it was not built
        for name, argtypes in _SIGS.items():
            f = getattr(self.lib, name)   # AttributeError if the shim lacks the symbol
            f.argtypes, f.restype = argtypes, C.c_int
        self.lib.acct_forget.argtypes, self.lib.acct_forget.restype = [C.c_void_p], None

    def close(self):
        self.lib.acct_forget(self.h)

    def scan(self, scan_type, x, exclusive, tot_mode=TOT_NONE, side_lane=False):
        """-> (out[n + 1], total word): out[n] is the total in TOT_CSR mode, the fill otherwise"""
        dt = SCAN_TYPES[scan_type][0]
        x = np.ascontiguousarray(x, dtype=dt)
        out, tot = np.zeros(len(x) + 1, dt), np.zeros(1, dt)
        self.ctx.check(self.lib.acct_scan(self.h, scan_type, _p(x), _p(out), len(x), int(exclusive), tot_mode, _p(tot),
                                          int(side_lane)))
        return out, tot[0]

    def scan_multi_rc(self, scan_type, xs, exclusive, tot_modes, side_lane=False):
        """-> (rc, [out_i[n_i + 1]], totals[k])"""
        dt = SCAN_TYPES[scan_type][0]
        k = len(xs)
        xs = [np.ascontiguousarray(x, dtype=dt) for x in xs]
        outs = [np.zeros(len(x) + 1, dt) for x in xs]
        tots = np.zeros(max(k, 1), dt)
        ins = (C.c_void_p * max(k, 1))(*[x.ctypes.data for x in xs])
        ous = (C.c_void_p * max(k, 1))(*[o.ctypes.data for o in outs])
        ns = (C.c_uint64 * max(k, 1))(*[len(x) for x in xs])
        tm = (C.c_int * max(k, 1))(*tot_modes)
        rc = self.lib.acct_scan_multi(self.h, scan_type, k, ins, ous, ns, int(exclusive), tm, _p(tots), int(side_lane))
        return rc, outs, tots[:k]

    def scan_multi(self, scan_type, xs, exclusive, tot_modes, side_lane=False):
        rc, outs, tots = self.scan_multi_rc(scan_type, xs, exclusive, tot_modes, side_lane)
        self.ctx.check(rc)
        return outs, tots

    def sum_u32(self, x):
        """-> (total, guard word)"""
        x = np.ascontiguousarray(x, dtype=np.uint32)
        out = np.zeros(2, np.uint64)
        self.ctx.check(self.lib.acct_sum_u32(self.h, _p(x), len(x), _p(out)))
        return int(out[0]), int(out[1])

    def radix_sort(self, tag, keys, vals, bits, three_launch=False):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        if vals is not None:
            vals = np.ascontiguousarray(vals, dtype=np.uint32)
        ko, vo = np.zeros(len(keys), np.uint64), np.zeros(len(keys), np.uint32)
        self.ctx.check(self.lib.acct_radix_sort(self.h, tag.encode(), _p(keys), None if vals is None else _p(vals), len(keys),
                                                bits, int(three_launch), _p(ko), _p(vo)))
        return ko, vo

    def radix_sort_keys(self, tag, keys, lo, bits):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        ko = np.zeros(len(keys), np.uint64)
        self.ctx.check(self.lib.acct_radix_sort_keys(self.h, tag.encode(), _p(keys), len(keys), lo, bits, _p(ko)))
        return ko

    def sort_result(self, tag, cap):
        """the tag's last result again -> (keys, vals)"""
        ko, vo, n = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), C.c_uint64(0)
        self.ctx.check(self.lib.acct_sort_result(self.h, tag.encode(), cap, _p(ko), _p(vo), C.byref(n)))
        return ko[:n.value], vo[:n.value]

    def block_exclusive(self, scan_type, x):
        """x: nblocks * 256 values -> (exclusive prefixes, per-block totals)"""
        dt = SCAN_TYPES[scan_type][0]
        x = np.ascontiguousarray(x, dtype=dt)
        assert len(x) % BLOCK == 0
        out, tot = np.zeros(len(x), dt), np.zeros(len(x) // BLOCK, dt)
        self.ctx.check(self.lib.acct_block_exclusive(self.h, scan_type, _p(x), len(x) // BLOCK, _p(out), _p(tot)))
        return out, tot

    def bitonic_reg(self, x):
        """x: nwaves * 64 u32 or u64 values -> each wave's 64 sorted"""
        x = np.ascontiguousarray(x)
        assert x.dtype in (np.uint32, np.uint64) and len(x) % 64 == 0
        out = np.zeros_like(x)
        self.ctx.check(self.lib.acct_bitonic_reg(self.h, int(x.dtype == np.uint64), _p(x), len(x) // 64, _p(out)))
        return out

    def block_bitonic(self, x, n2, in_lds):
        """x: nblocks * n2 values -> (each block's n2 sorted, the guard element)"""
        x = np.ascontiguousarray(x)
        assert x.dtype in (np.uint32, np.uint64) and len(x) % n2 == 0
        out = np.zeros(len(x) + 1, x.dtype)
        self.ctx.check(self.lib.acct_block_bitonic(self.h, int(x.dtype == np.uint64), int(in_lds), _p(x), n2, len(x) // n2,
                                                   _p(out)))
        return out[:-1], out[-1]

    def chunk_owners(self, off, pt=8):
        """-> (own[nchunks * pt * 256], carry[nchunks]) over the runs off[0 .. nt]"""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        ch = pt * BLOCK
        nch = (int(off[-1]) - int(off[0]) + ch - 1) // ch
        own, carry = np.zeros(nch * ch, np.uint32), np.zeros(nch, np.uint32)
        self.ctx.check(self.lib.acct_chunk_owners(self.h, len(off) - 1, _p(off), _p(own), _p(carry)))
        return own, carry

    def pext_runs(self, mask, w):
        """-> (out, Runs.bits, Runs.n)"""
        w = np.ascontiguousarray(w, dtype=np.uint64)
        out, bits, nruns = np.zeros(len(w), np.uint64), C.c_int(-1), C.c_int(-1)
        self.ctx.check(self.lib.acct_pext_runs(self.h, mask, _p(w), len(w), _p(out), C.byref(bits), C.byref(nruns)))
        return out, bits.value, nruns.value

    # ---- csrc/search.hpp: every method returns (results, the guard element behind them)

    def search_bound(self, a, lo, hi, v, upper, idx64):
        """lower_bound / upper_bound over a (u32 or u64), query q over the window [lo[q], hi[q]) for v[q]"""
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.uint32, np.uint64)
        lo, hi, v = (np.ascontiguousarray(x, dtype=np.uint64) for x in (lo, hi, v))
        out = np.zeros(len(v) + 1, np.uint64)
        self.ctx.check(self.lib.acct_search_bound(self.h, int(a.dtype == np.uint64), int(idx64), int(upper), _p(a), len(a),
                                                  _p(lo), _p(hi), _p(v), len(v), _p(out)))
        return out[:-1], out[-1]

    def seg_of(self, off, v):
        off, v = np.ascontiguousarray(off, dtype=np.uint32), np.ascontiguousarray(v, dtype=np.uint32)
        out = np.zeros(len(v) + 1, np.uint32)
        self.ctx.check(self.lib.acct_seg_of(self.h, _p(off), len(off), _p(v), len(v), _p(out)))
        return out[:-1], out[-1]

    def find_sorted(self, a, v):
        a, v = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(v, dtype=np.uint64)
        out = np.zeros(len(v) + 1, np.uint32)
        self.ctx.check(self.lib.acct_find_sorted(self.h, _p(a), len(a), _p(v), len(v), _p(out)))
        return out[:-1], out[-1]

    def ts_bound(self, cols, lo, hi, qcols, upper):
        """cols / qcols: (msb u64, lsb u64, node i32) column triples"""
        m, l, n = (np.ascontiguousarray(x, dtype=t) for x, t in zip(cols, (np.uint64, np.uint64, np.int32)))
        qm, ql, qn = (np.ascontiguousarray(x, dtype=t) for x, t in zip(qcols, (np.uint64, np.uint64, np.int32)))
        lo, hi = np.ascontiguousarray(lo, dtype=np.uint32), np.ascontiguousarray(hi, dtype=np.uint32)
        out = np.zeros(len(qm) + 1, np.uint32)
        self.ctx.check(self.lib.acct_ts_bound(self.h, int(upper), _p(m), _p(l), _p(n), len(m), _p(lo), _p(hi), _p(qm), _p(ql),
                                              _p(qn), len(qm), _p(out)))
        return out[:-1], out[-1]

    def wave_search(self, a, lo, hi, v, upper):
        """-> (results[nq, 64]: every lane's, the guard element)"""
        a, v = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(v, dtype=np.uint64)
        lo, hi = np.ascontiguousarray(lo, dtype=np.uint32), np.ascontiguousarray(hi, dtype=np.uint32)
        out = np.zeros(len(v) * 64 + 1, np.uint32)
        self.ctx.check(self.lib.acct_wave_search(self.h, _p(a), len(a), _p(lo), _p(hi), _p(v), int(upper), len(v), _p(out)))
        return out[:-1].reshape(len(v), 64), out[-1]
