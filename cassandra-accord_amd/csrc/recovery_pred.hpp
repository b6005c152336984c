// recovery_pred.hpp — what the recovery scans (SafeCommandStore.mapReduceFull) test, stated once for every route: the
// call-wide parameters (RcParams, checked and built by recovery_params) and the two per-element predicates.
// cfk_entry_passes<V>: the per-entry tests of CommandsForKey.mapReduceFull (local/CommandsForKey.java:577-607), for
// recovery.hip over the CFK snapshot (TxnId ranks, packed status | kind byte) and cfkquery.hip over the resident segments
// (raw timestamp columns). V views one query against one of the two: mask (its Kinds mask), status(e), kind(e),
// executes_after_x(e) (executeAt > X = testTxnId), x_in_missing(e). An accessor does its loads when it is called.
// rr_command_passes<C>: the per-command tests of InMemorySafeStore.mapReduceRangesInternal
// (impl/InMemoryCommandStore.java:889-933), for recovery.hip over a table the caller passes (RrCmds) and rcmd.hip over
// the resident range-command store's columns. C is the column record, which names
//   tm, tl, tn, em, el, en   TxnId and executeAt columns          status, flags   Status ordinal, ACC_RCMD_* bits
//   roff, rs, re             each command's Ranges                 doff, dm, dl, dn, ds, de, dk   its flattened PartialDeps
//   end_incl                 the Range bound type
#pragma once

#include "../../include/accord_amd.h"
#include "ctx.hpp"
#include "search.hpp"

namespace acc {

struct RcParams {
    uint32_t started_at, test_dep, test_status, exec_after;
    int32_t test_kinds;   // the Kinds mask, or -1: testTxnId.kind().witnessedBy()
};

// the call-wide tests of acc_recovery_in and its kin
inline RcParams recovery_params(uint32_t started_at, uint32_t test_dep, uint32_t test_status, uint32_t flags, int32_t test_kinds)
{
    if (started_at > ACC_STARTED_ANY || test_dep > ACC_DEP_ANY || test_status > ACC_STATUS_IS_STABLE)
        fail(ACC_E_ARG, "started_at / test_dep / test_status must be TestStartedAt / TestDep / TestStatus ordinals");
    if (flags & ~ACC_FULL_EXECUTES_AFTER) fail(ACC_E_ARG, "unknown flags");
    if (test_kinds > 0x3F) fail(ACC_E_ARG, "test_kinds must be a mask over the six Kind ordinals, or -1");
    return RcParams{ started_at, test_dep, test_status, flags & ACC_FULL_EXECUTES_AFTER, test_kinds < 0 ? -1 : test_kinds };
}

// the per-entry tests (:577-607) plus the optional executeAt > testTxnId map filter, the cheap ones first: the status
// byte alone refuses most entries of a steady-state segment; missing[] is searched only under WITH / WITHOUT
template <class V>
__device__ __forceinline__ bool cfk_entry_passes(const V &v, const RcParams &p, uint32_t e)
{
    const uint32_t st = v.status(e);
    switch (p.test_status) {
    case ACC_STATUS_IS_PROPOSED: if (st != ACC_ST_ACCEPTED && st != ACC_ST_COMMITTED) return false; break;
    case ACC_STATUS_IS_STABLE:   if (st < ACC_ST_STABLE || st >= ACC_ST_INVALID_OR_TRUNCATED) return false; break;
    default:                     if (st == ACC_ST_TRANSITIVELY_KNOWN) return false; break;
    }
    const bool dep = p.test_dep != ACC_DEP_ANY;
    if (dep && (st < ACC_ST_ACCEPTED || st > ACC_ST_APPLIED)) return false;   // !InternalStatus.hasInfo
    if (!((v.mask >> v.kind(e)) & 1u)) return false;                          // testKind.test(txnId.kind())
    if ((dep || p.exec_after) && !v.executes_after_x(e)) return false;
    if (dep && v.x_in_missing(e) == (p.test_dep == ACC_DEP_WITH)) return false;   // hasAsDep != (testDep == WITH)
    return true;
}

__device__ __forceinline__ bool rr_contains(uint64_t s, uint64_t e, uint64_t k, bool ei)
{
    return ei ? (s < k && k <= e) : (s <= k && k < e);   // Range.contains (Range.java:40-138)
}

// Deps.intersects(X, ranges of entry i): a KeyDeps entry of X whose key one of the ranges contains, or a RangeDeps entry
// of X whose range intersects one of them
template <class C>
__device__ bool rr_deps_intersect(const C &c, uint32_t i, uint64_t xm, uint64_t xl, int32_t xn)
{
    const uint32_t lo = lower_bound_ts(c.dm, c.dl, c.dn, c.doff[i], c.doff[i + 1], Ts{ xm, xl, xn });
    const uint32_t r0 = c.roff[i], r1 = c.roff[i + 1];
    const bool ei = c.end_incl != 0;
    // (the two range searches below stay hand loops: through search.hpp the scan kernels that inline this take two more
    // SGPRs, and recovery.hip's k_rr_scan loses a wave per SIMD)
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

// local/Status.java ordinals of a range command's status column (the public header lists them without names)
constexpr uint32_t RR_ST_ACCEPTED = 3, RR_ST_PRECOMMITTED = 4, RR_ST_COMMITTED = 5;   // Accepted, PreCommitted, Committed
constexpr uint32_t RR_ST_STABLE = 6, RR_ST_TRUNCATED = 9, RR_ST_INVALIDATED = 10;     // Stable, Truncated, Invalidated (the last)

// the per-command tests of mapReduceRangesInternal (:889-933) plus the optional executeAt > testTxnId map filter, the
// cheap ones first: kind, flags and status byte, executeAt against X, and only for what is left under WITH / WITHOUT
// the search of X in the command's deps (*probed tells that it ran)
template <class C>
__device__ bool rr_command_passes(const C &c, const RcParams &p, uint32_t i, uint32_t mask, uint64_t xm, uint64_t xl, int32_t xn,
                                  bool *probed = nullptr)
{
    const uint32_t f = c.flags[i];
    const bool hist = (f & ACC_RCMD_HISTORICAL) != 0;
    const bool dep = p.test_dep != ACC_DEP_ANY;
    if (!(((mask >> ((c.tl[i] >> 1) & 7u)) & 1u))) return false;   // testKind.test(txnId.kind())
    if (hist) {
        if (p.test_status != ACC_STATUS_ANY || dep) return false;     // historical: ANY_STATUS + ANY_DEPS only
        if (p.exec_after && ts_cmp(c.tm[i], c.tl[i], c.tn[i], xm, xl, xn) <= 0) return false;   // executeAt = txnId
        return true;
    }
    if (f & ACC_RCMD_ERASED) return false;
    const uint32_t st = c.status[i];
    if (p.test_status == ACC_STATUS_IS_PROPOSED && !(st == RR_ST_ACCEPTED || st == RR_ST_PRECOMMITTED || st == RR_ST_COMMITTED))
        return false;
    if (p.test_status == ACC_STATUS_IS_STABLE && !(st >= RR_ST_STABLE && st < RR_ST_TRUNCATED)) return false;
    if (dep && !(f & ACC_RCMD_HAS_DEPS)) return false;
    const int ex_cmp = ts_cmp(c.em[i], c.el[i], c.en[i], xm, xl, xn);
    // STARTED_BEFORE falls through into ANY's test (:897-901)
    if (p.started_at != ACC_STARTED_AFTER && dep && ex_cmp < 0) return false;
    if (p.exec_after && ex_cmp <= 0) return false;
    if (dep) {
        if (probed) *probed = true;
        const bool has = rr_deps_intersect(c, i, xm, xl, xn);
        if ((p.test_dep == ACC_DEP_WITH) == !has) return false;
    }
    return true;
}

}  // namespace acc
