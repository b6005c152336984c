// recovery_pred.hpp — the per-command tests of InMemorySafeStore.mapReduceRangesInternal
// (impl/InMemoryCommandStore.java:889-933), stated once for the two routes that evaluate them: recovery.hip over a table
// the caller passes (RrCmds) and rcmd.hip over the resident range-command store's columns. Both are templated over the
// column record C, which names
//   tm, tl, tn, em, el, en   TxnId and executeAt columns          status, flags   Status ordinal, ACC_RCMD_* bits
//   roff, rs, re             each command's Ranges                 doff, dm, dl, dn, ds, de, dk   its flattened PartialDeps
//   end_incl                 the Range bound type
#pragma once

#include "../../include/accord_amd.h"
#include "ts.hpp"

namespace acc {

struct RcParams {
    uint32_t started_at, test_dep, test_status, exec_after;
};

__device__ __forceinline__ bool rr_contains(uint64_t s, uint64_t e, uint64_t k, bool ei)
{
    return ei ? (s < k && k <= e) : (s <= k && k < e);   // Range.contains (Range.java:40-138)
}

// Deps.intersects(X, ranges of entry i): a KeyDeps entry of X whose key one of the ranges contains, or a RangeDeps entry
// of X whose range intersects one of them
template <class C>
__device__ bool rr_deps_intersect(const C &c, uint32_t i, uint64_t xm, uint64_t xl, int32_t xn)
{
    uint32_t lo = c.doff[i], hi = c.doff[i + 1];
    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (ts_cmp(c.dm[m], c.dl[m], c.dn[m], xm, xl, xn) < 0) lo = m + 1; else hi = m; }
    const uint32_t r0 = c.roff[i], r1 = c.roff[i + 1];
    const bool ei = c.end_incl != 0;
    for (uint32_t j = lo; j < c.doff[i + 1] && ts_cmp(c.dm[j], c.dl[j], c.dn[j], xm, xl, xn) == 0; ++j) {
        const uint64_t s = c.ds[j];
        if (c.dk[j]) {
            uint32_t a = r0, b = r1;   // first range whose end reaches the key
            while (a < b) { const uint32_t m = (a + b) >> 1; if (ei ? c.re[m] < s : c.re[m] <= s) a = m + 1; else b = m; }
            if (a < r1 && rr_contains(c.rs[a], c.re[a], s, ei)) return true;
        } else {
            const uint64_t t = c.de[j];
            uint32_t a = r0, b = r1;   // first range ending after s
            while (a < b) { const uint32_t m = (a + b) >> 1; if (c.re[m] <= s) a = m + 1; else b = m; }
            if (a < r1 && c.rs[a] < t) return true;
        }
    }
    return false;
}

// the per-command tests of mapReduceRangesInternal (:889-933) plus the optional executeAt > testTxnId map filter, the
// cheap ones first: kind, flags and status byte, executeAt against X, and only for what is left under WITH / WITHOUT
// the search of X in the command's deps (*probed tells that it ran)
template <class C>
__device__ bool rr_command_passes(const C &c, const RcParams &p, uint32_t i, uint32_t mask, uint64_t xm, uint64_t xl, int32_t xn,
                                  bool *probed = nullptr)
{
    const uint32_t f = c.flags[i];
    const bool hist = (f & ACC_RCMD_HISTORICAL) != 0;
    if (!(((mask >> ((c.tl[i] >> 1) & 7u)) & 1u))) return false;   // testKind.test(txnId.kind())
    if (hist) {
        if (p.test_status != 0 || p.test_dep != 2) return false;      // historical: ANY_STATUS + ANY_DEPS only
        if (p.exec_after && ts_cmp(c.tm[i], c.tl[i], c.tn[i], xm, xl, xn) <= 0) return false;   // executeAt = txnId
        return true;
    }
    if (f & ACC_RCMD_ERASED) return false;
    const uint32_t st = c.status[i];
    if (p.test_status == 1 && !(st == 3 || st == 4 || st == 5)) return false;   // IS_PROPOSED: Accepted, PreCommitted, Committed
    if (p.test_status == 2 && !(st >= 6 && st < 9)) return false;               // IS_STABLE: Stable <= s < Truncated
    if (p.test_dep != 2 && !(f & ACC_RCMD_HAS_DEPS)) return false;
    const int ex_cmp = ts_cmp(c.em[i], c.el[i], c.en[i], xm, xl, xn);
    // STARTED_BEFORE falls through into ANY's test (:897-901)
    if (p.started_at != 1 && p.test_dep != 2 && ex_cmp < 0) return false;
    if (p.exec_after && ex_cmp <= 0) return false;
    if (p.test_dep != 2) {
        if (probed) *probed = true;
        const bool has = rr_deps_intersect(c, i, xm, xl, xn);
        if ((p.test_dep == 0) == !has) return false;
    }
    return true;
}

}  // namespace acc
