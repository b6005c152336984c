// waiting.hip — the resident WaitingOn store (acc_waiting_*): Command.WaitingOn (local/Command.java:1294-1610) of every
// registered Stable command, advanced as local/Commands.java advances it (initialiseWaitingOn :735-753, updateWaitingOn
// :755-830, updateDependencyAndMaybeExecute :832-857, removeWaitingOnKeyAndMaybeExecute :859-876) against the per-command
// state of an acc_rcmd store. include/accord_amd.h states the semantics (evaluate(W, i), steps 0-5); DESIGN.md
// "acc_waiting" the layout.
//
// The table: records in TxnId order; keys and deps as two CSRs; the mutable columns (dep_state, key_wait,
// execute_at_least, the two waiting counts) twice, so that a call works on the spare set and commits by exchanging the
// two; idx = the dep slots in dep TxnId order (the index from a changed dep to the slots that hold it).
// Evaluation is two passes over a worklist of dep slots in ascending slot order (so grouped by record):
//   k_wt_own    a thread per slot: everything evaluate() reads outside its record (D's row in the acc_rcmd table, D's own
//               record R), folded into the slot's own branch: REMOVE (step 3), SET (step 2), APPLIED (step 4), and
//               whether step 1 raises execute_at_least;
//   k_wt_walk_* a record's worklist slots in descending order, a slot the walk cleared earlier skipped; by one of two
//               tiers chosen by the record's dep count:
//        LANE  n_dep <= WT_LANE_MAX: one lane walks the slots and merges R.dep into W.dep with two cursors;
//        WAVE  the rest: one wave; 64 worklist slots at a time, the still-waiting ones taken highest first from a
//              ballot; a propagation is a lane per W slot searching R.dep, after which the chunk's states are re-read.
// R is read from the table as it stood when the call began (the live columns; the walk writes the spare ones), so no
// walk reads what another writes.
// register: waiters validated and ranked (dense_rank), the merged record order placed by rank, both CSRs gathered into
// a new table, the index sorted (three stable radix passes), the new records evaluated, then the table exchanged.
// notify: the index ranges of the changed deps expanded into the worklist and sorted by slot; the release pairs sorted
// by record and applied by one lane per record; the ready list from the counts before and after.
// erase: a stable compaction through the same gather.
#include "dict.hpp"
#include "prims.hpp"
#include "rcmd_partial.hpp"
#include "search.hpp"

#include <chrono>

namespace acc {
namespace wt {

constexpr uint32_t WT_LANE_MAX = 16;   // dep slots of a record the lane tier walks by default
constexpr uint32_t NONE = 0xFFFFFFFFu;

enum : uint64_t {
    E_OFF = 1, E_KEYS = 2, E_DEPS = 4, E_DOMAIN = 8, E_KIND = 16, E_WAIT = 32, E_DUP = 64, E_APPLIED = 128, E_INVARIANT = 256,
    E_CHANGED = 512, E_RELFLAGS = 1024, E_IDS = 2048
};
enum : uint32_t { T_LANE = ACC_WT_TIER_LANE, T_WAVE = ACC_WT_TIER_WAVE };
// a worklist slot's own branch (k_wt_own): the action, and whether step 1 raises execute_at_least
enum : uint32_t { A_NONE = 0, A_REMOVE = 1, A_SET = 2, A_APPLIED = 3, A_MASK = 3, A_EAL = 4 };
// counters of a call
enum : int { C_EVAL = 0, C_PROP = 1, C_KREL = 2, C_KIGN = 3, C_CHANGED = 4, C_N = 5 };

__host__ __device__ __forceinline__ uint32_t tier_of(uint32_t n_dep, uint32_t forced)
{
    return forced ? forced : n_dep <= WT_LANE_MAX ? T_LANE : T_WAVE;
}


// the table as the kernels see it
struct Tab {
    uint32_t nr, nk, nd;
    uint64_t *tm, *tl, *xm, *xl;
    int32_t *tn, *xn;
    uint8_t *flags;
    uint32_t *key_off, *dep_off;
    uint64_t *key, *dm, *dl;
    int32_t *dn;
    uint32_t *idx;          // [nd] dep slots in dep TxnId order, ties in slot order
    // mutable
    uint8_t *kw, *ds;
    uint64_t *am, *al;
    int32_t *an;
    uint32_t *nwd, *nwk;    // [nr] WAITING dep slots, set key bits
};

// the acc_rcmd columns evaluate() reads
struct Rc {
    uint32_t n;
    const uint64_t *tm, *tl, *xm, *xl;
    const int32_t *tn, *xn;
    const uint8_t *status;
};

__device__ __forceinline__ Ts txn_of(const Tab &t, uint32_t r) { return Ts{ t.tm[r], t.tl[r], t.tn[r] }; }
__device__ __forceinline__ Ts x_of(const Tab &t, uint32_t r) { return Ts{ t.xm[r], t.xl[r], t.xn[r] }; }
__device__ __forceinline__ Ts dep_of(const Tab &t, uint32_t s) { return Ts{ t.dm[s], t.dl[s], t.dn[s] }; }
__device__ __forceinline__ uint32_t clr_of(uint32_t flags) { return flags & ACC_WT_RANGE_DOMAIN ? ACC_WT_APPLIED_OR_INVALIDATED : ACC_WT_NOT_WAITING; }

// the element of [lo, hi) that equals t, or NONE
__device__ __forceinline__ uint32_t find_ts(const uint64_t *m, const uint64_t *l, const int32_t *n, uint32_t lo, uint32_t hi, const Ts &t)
{
    const uint32_t p = lower_bound_ts(m, l, n, lo, hi, t);
    return p < hi && cmp(ts_at(m, l, n, p), t) == 0 ? p : NONE;
}

__device__ __forceinline__ void err(uint64_t *errs, uint64_t e) { atomicOr((unsigned long long *)errs, (unsigned long long)e); }

// updateExecuteAtLeast: nonNullOrMax(x, executeAtLeast), the new value on a tie (Timestamp.max, primitives/Timestamp.java:265-268)
__device__ __forceinline__ bool raise(Ts &eal, const Ts &x)
{
    if (!is_null(eal) && cmp(x, eal) < 0) return false;
    eal = x;
    return true;
}

// ---------------------------------------------------------------- evaluation

struct Work {
    uint32_t n;
    const uint32_t *wl;     // [n] dep slots, ascending
    uint8_t *own;           // [n] A_*
    uint32_t *drow, *ridx;  // [n] D's row in the acc_rcmd table; D's record in the table as the call found it (A_APPLIED)
};

__global__ __launch_bounds__(BLOCK) void k_wt_own(Work w, Tab W, Tab S, Rc rc, unsigned long long *__restrict__ cnt)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    bool vis = false;
    if (p < w.n) {
        const uint32_t s = w.wl[p];
        uint32_t o = A_NONE, row = NONE, R = NONE;
        if (W.ds[s] == ACC_WT_WAITING) {
            vis = true;
            const uint32_t r = seg_of(W.dep_off, W.nr, s);
            const Ts d = dep_of(W, s);
            row = find_ts(rc.tm, rc.tl, rc.tn, 0, rc.n, d);
            const uint32_t st = row == NONE ? 0u : rc.status[row];
            if (st >= 4) {
                const Ts dx = ts_at(rc.xm, rc.xl, rc.xn, row);
                const bool aod = W.flags[r] & ACC_WT_AWAITS_ONLY_DEPS;
                if (aod && st <= 9 && !is_null(dx) && cmp(dx, txn_of(W, r)) > 0) o |= A_EAL;
                if (st >= 9) o |= A_SET;
                else if (!aod && cmp(dx, x_of(W, r)) > 0) o |= A_REMOVE;
                else if (st == 8) { o |= A_APPLIED; R = find_ts(S.tm, S.tl, S.tn, 0, S.nr, d); }
            }
        }
        w.own[p] = (uint8_t)o;
        w.drow[p] = row;
        w.ridx[p] = R;
    }
    const unsigned long long b = __ballot(vis);
    if (b && lane_id() == 0) atomicAdd(cnt + C_EVAL, (unsigned long long)__popcll(b));
}

struct Walk {
    uint32_t nt;
    const uint32_t *trec, *woff;   // [nt] the touched records, [nt + 1] their worklist ranges
    Work w;
    uint32_t forced;
    unsigned long long *cnt;
    uint64_t *errs;
};

__global__ __launch_bounds__(BLOCK) void k_wt_walk_lane(Walk k, Tab W, Tab S, Rc rc)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= k.nt) return;
    const uint32_t r = k.trec[t], d0 = W.dep_off[r], d1 = W.dep_off[r + 1];
    if (tier_of(d1 - d0, k.forced) != T_LANE) return;
    const uint32_t p0 = k.woff[t], p1 = k.woff[t + 1], clr = clr_of(W.flags[r]);
    Ts eal{ W.am[r], W.al[r], W.an[r] };
    bool dirty = false;
    uint32_t cleared = 0, prop = 0;
    for (uint32_t p = p1; p-- > p0;) {
        const uint32_t o = k.w.own[p];
        if (!o) continue;
        const uint32_t s = k.w.wl[p];
        if (W.ds[s] != ACC_WT_WAITING) continue;   // cleared earlier in the walk
        if (o & A_EAL) dirty |= raise(eal, ts_at(rc.xm, rc.xl, rc.xn, k.w.drow[p]));
        const uint32_t a = o & A_MASK;
        if (a == A_NONE) continue;
        W.ds[s] = (uint8_t)(a == A_REMOVE ? ACC_WT_NOT_WAITING : clr);
        ++cleared;
        const uint32_t R = a == A_APPLIED ? k.w.ridx[p] : NONE;
        if (R == NONE) continue;
        if (S.nwd[R] + S.nwk[R]) { err(k.errs, E_INVARIANT); continue; }
        if (!(S.flags[R] & ACC_WT_RANGE_DOMAIN)) continue;
        uint32_t i = S.dep_off[R], j = d0;
        const uint32_t i1 = S.dep_off[R + 1];
        while (i < i1 && j < d1) {   // forEachIntersection(propagate.txnIds, txnIds)
            const int c = cmp(dep_of(S, i), dep_of(W, j));
            if (c < 0) ++i;
            else if (c > 0) ++j;
            else {
                if (S.ds[i] == ACC_WT_APPLIED_OR_INVALIDATED && W.ds[j] == ACC_WT_WAITING) { W.ds[j] = (uint8_t)clr; ++cleared; ++prop; }
                ++i; ++j;
            }
        }
    }
    if (cleared) W.nwd[r] -= cleared;
    if (dirty) { W.am[r] = eal.m; W.al[r] = eal.l; W.an[r] = eal.n; }
    if (prop) atomicAdd(k.cnt + C_PROP, (unsigned long long)prop);
}

__global__ __launch_bounds__(BLOCK) void k_wt_walk_wave(uint64_t first, Walk k, Tab W, Tab S, Rc rc)
{
    const uint64_t t64 = first + (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (t64 >= k.nt) return;   // (the whole wave)
    const uint32_t t = (uint32_t)t64, r = k.trec[t], d0 = W.dep_off[r], d1 = W.dep_off[r + 1];
    if (tier_of(d1 - d0, k.forced) != T_WAVE) return;
    const uint32_t lane = lane_id(), p0 = k.woff[t], p1 = k.woff[t + 1], clr = clr_of(W.flags[r]);
    Ts eal{ W.am[r], W.al[r], W.an[r] };   // wave-uniform from here on
    bool dirty = false;
    uint32_t cleared = 0, prop = 0;
    const uint32_t nchunk = (p1 - p0 + 63u) >> 6;
    for (uint32_t c = nchunk; c-- > 0;) {
        const uint32_t pb = p0 + (c << 6), p = pb + lane;
        const bool valid = p < p1;
        const uint32_t o = valid ? k.w.own[p] : 0u, s = valid ? k.w.wl[p] : 0u;
        bool wait = valid && o && W.ds[s] == ACC_WT_WAITING;
        uint64_t below = ~0ull;
        for (uint32_t it = 0; it < 64; ++it) {   // each turn takes the highest waiting slot below the last one taken
            const uint64_t act = __ballot(wait) & below;
            if (!act) break;
            const int j = 63 - __builtin_clzll(act);
            below = ((uint64_t)1 << j) - 1;
            const uint32_t oj = shfl_idx(o, j), sj = shfl_idx(s, j), pj = pb + (uint32_t)j;
            if (oj & A_EAL) dirty |= raise(eal, ts_at(rc.xm, rc.xl, rc.xn, k.w.drow[pj]));
            const uint32_t a = oj & A_MASK;
            if (a == A_NONE) continue;
            if (lane == 0) W.ds[sj] = (uint8_t)(a == A_REMOVE ? ACC_WT_NOT_WAITING : clr);
            ++cleared;
            const uint32_t R = a == A_APPLIED ? k.w.ridx[pj] : NONE;
            if (R == NONE) continue;
            if (S.nwd[R] + S.nwk[R]) { if (lane == 0) err(k.errs, E_INVARIANT); continue; }
            if (!(S.flags[R] & ACC_WT_RANGE_DOMAIN)) continue;
            const uint32_t i0 = S.dep_off[R], i1 = S.dep_off[R + 1];
            if (i1 == i0) continue;
            for (uint32_t b = d0; b < d1; b += 64) {   // a lane per W slot, searching R.dep
                const uint32_t jj = b + lane;
                bool hit = false;
                if (jj < d1 && jj != sj && W.ds[jj] == ACC_WT_WAITING) {
                    const uint32_t e = find_ts(S.dm, S.dl, S.dn, i0, i1, dep_of(W, jj));
                    hit = e != NONE && S.ds[e] == ACC_WT_APPLIED_OR_INVALIDATED;
                    if (hit) W.ds[jj] = (uint8_t)clr;
                }
                const uint32_t h = (uint32_t)__popcll(__ballot(hit));
                cleared += h;
                prop += h;
            }
            __threadfence_block();   // the lanes' stores before the chunk's states are read again
            wait = valid && o && W.ds[s] == ACC_WT_WAITING;
        }
    }
    if (lane == 0) {
        if (cleared) W.nwd[r] -= cleared;
        if (dirty) { W.am[r] = eal.m; W.al[r] = eal.l; W.an[r] = eal.n; }
        if (prop) atomicAdd(k.cnt + C_PROP, (unsigned long long)prop);
    }
}

// ---------------------------------------------------------------- register: validation and placement

struct In {
    uint32_t nw, NK, ND;
    const uint64_t *tm, *tl, *xm, *xl;
    const int32_t *tn, *xn;
    const uint32_t *key_off, *dep_off;
    const uint64_t *key, *dm, *dl;
    const int32_t *dn;
    const uint8_t *key_wait, *dep_wait;   // null: all ones
};

// per waiter: kind, offsets, the compare words for the ranking, its place in the table, its row in the acc_rcmd table
__global__ __launch_bounds__(BLOCK) void k_wt_reg_waiters(In d, Tab S, Rc rc, uint64_t *__restrict__ w0, uint64_t *__restrict__ w1,
                                                          uint64_t *__restrict__ w2, uint32_t *__restrict__ lb, uint64_t *__restrict__ errs)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= d.nw) return;
    uint64_t e = 0;
    const Ts id{ d.tm[i], d.tl[i], d.tn[i] };
    if (((uint32_t)(id.l >> 1) & 7u) > ACC_KIND_LOCAL_ONLY) e |= E_KIND;
    const uint32_t k0 = d.key_off[i], k1 = d.key_off[i + 1], a0 = d.dep_off[i], a1 = d.dep_off[i + 1];
    if (k1 < k0 || k1 > d.NK || (i == 0 && k0 != 0) || (i + 1 == d.nw && k1 != d.NK)) e |= E_OFF;
    if (a1 < a0 || a1 > d.ND || (i == 0 && a0 != 0) || (i + 1 == d.nw && a1 != d.ND)) e |= E_OFF;
    w0[i] = id.m;
    w1[i] = ts_w1(id.l);
    w2[i] = ts_w2(id.n);
    const uint32_t p = lower_bound_ts(S.tm, S.tl, S.tn, 0, S.nr, id);
    if (p < S.nr && cmp(txn_of(S, p), id) == 0) e |= E_DUP;
    lb[i] = p;
    const uint32_t row = find_ts(rc.tm, rc.tl, rc.tn, 0, rc.n, id);
    if (row != NONE && rc.status[row] >= 8) e |= E_APPLIED;
    if (e) err(errs, e);
}

// keys of a waiter sorted unique, wait bytes 0 / 1: checked slot by slot (offsets are valid by now)
__global__ __launch_bounds__(BLOCK) void k_wt_reg_keys(In d, uint64_t *__restrict__ errs)
{
    const uint32_t u = blockIdx.x * BLOCK + threadIdx.x;
    if (u >= d.NK) return;
    uint64_t e = 0;
    if (d.key_wait && d.key_wait[u] > 1) e |= E_WAIT;
    if (u > 0 && d.key[u - 1] >= d.key[u] && d.key_off[seg_of(d.key_off, d.nw, u)] != u) e |= E_KEYS;
    if (e) err(errs, e);
}

__global__ __launch_bounds__(BLOCK) void k_wt_reg_deps(In d, uint64_t *__restrict__ errs)
{
    const uint32_t u = blockIdx.x * BLOCK + threadIdx.x;
    if (u >= d.ND) return;
    uint64_t e = 0;
    if (d.dep_wait && d.dep_wait[u] > 1) e |= E_WAIT;
    if (!(d.dl[u] & 1u)) e |= E_DOMAIN;   // rangeDeps hold range-domain TxnIds
    if (u > 0 && cmp(ts_at(d.dm, d.dl, d.dn, u - 1), ts_at(d.dm, d.dl, d.dn, u)) >= 0 && d.dep_off[seg_of(d.dep_off, d.nw, u)] != u)
        e |= E_DEPS;
    if (e) err(errs, e);
}

// where every record of the next table comes from: an old record (srco) or a waiter (srcw), and its slot counts
struct Src {
    uint32_t *srco, *srcw, *kc, *dc;
};

// the stable merge: an old record moves up by the waiters below it, a waiter sits at its rank plus the old records below
// it. perm: the waiters in TxnId order (null: as given)
__global__ __launch_bounds__(BLOCK) void k_wt_place(In d, Tab S, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ perm,
                                                    const uint32_t *__restrict__ lb, Src o, uint32_t *__restrict__ npos)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= S.nr + d.nw) return;
    if (i < S.nr) {
        const Ts id = txn_of(S, i);
        const uint32_t lo = partition_point(0u, d.nw, [&](uint32_t m) { return cmp(ts_at(d.tm, d.tl, d.tn, perm ? perm[m] : m), id) < 0; });
        const uint32_t q = i + lo;
        o.srco[q] = i; o.srcw[q] = NONE;
        o.kc[q] = S.key_off[i + 1] - S.key_off[i];
        o.dc[q] = S.dep_off[i + 1] - S.dep_off[i];
    } else {
        const uint32_t w = i - S.nr, q = rank[w] + lb[w];
        o.srco[q] = NONE; o.srcw[q] = w;
        o.kc[q] = d.key_off[w + 1] - d.key_off[w];
        o.dc[q] = d.dep_off[w + 1] - d.dep_off[w];
        npos[w] = q;
    }
}

// ---------------------------------------------------------------- the gather into a new table (register, erase)

__global__ __launch_bounds__(BLOCK) void k_wt_fill_rec(Tab N, Tab S, In d, Src o)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= N.nr) return;
    const uint32_t r = o.srco[q];
    if (r != NONE) {
        N.tm[q] = S.tm[r]; N.tl[q] = S.tl[r]; N.tn[q] = S.tn[r];
        N.xm[q] = S.xm[r]; N.xl[q] = S.xl[r]; N.xn[q] = S.xn[r];
        N.flags[q] = S.flags[r];
        N.am[q] = S.am[r]; N.al[q] = S.al[r]; N.an[q] = S.an[r];
        N.nwd[q] = S.nwd[r]; N.nwk[q] = S.nwk[r];
    } else {
        const uint32_t w = o.srcw[q];
        const uint64_t l = d.tl[w];
        const uint32_t kind = (uint32_t)(l >> 1) & 7u;
        N.tm[q] = d.tm[w]; N.tl[q] = l; N.tn[q] = d.tn[w];
        N.xm[q] = d.xm[w]; N.xl[q] = d.xl[w]; N.xn[q] = d.xn[w];
        N.flags[q] = (uint8_t)((kind == ACC_KIND_EXCLUSIVE_SYNC_POINT || kind == ACC_KIND_EPHEMERAL_READ ? ACC_WT_AWAITS_ONLY_DEPS : 0u) |
                               (l & 1u ? ACC_WT_RANGE_DOMAIN : 0u));
        N.am[q] = 0; N.al[q] = 0; N.an[q] = 0;
        N.nwd[q] = 0; N.nwk[q] = 0;   // counted by the slot passes
    }
}

__global__ __launch_bounds__(BLOCK) void k_wt_fill_keys(Tab N, Tab S, In d, Src o)
{
    const uint32_t u = blockIdx.x * BLOCK + threadIdx.x;
    if (u >= N.nk) return;
    const uint32_t q = seg_of(N.key_off, N.nr, u), j = u - N.key_off[q], r = o.srco[q];
    if (r != NONE) {
        const uint32_t s = S.key_off[r] + j;
        N.key[u] = S.key[s];
        N.kw[u] = S.kw[s];
    } else {
        const uint32_t s = d.key_off[o.srcw[q]] + j;
        const uint8_t w = d.key_wait ? d.key_wait[s] : (uint8_t)1;
        N.key[u] = d.key[s];
        N.kw[u] = w;
        if (w) atomicAdd(&N.nwk[q], 1u);
    }
}

__global__ __launch_bounds__(BLOCK) void k_wt_fill_deps(Tab N, Tab S, In d, Src o)
{
    const uint32_t u = blockIdx.x * BLOCK + threadIdx.x;
    if (u >= N.nd) return;
    const uint32_t q = seg_of(N.dep_off, N.nr, u), j = u - N.dep_off[q], r = o.srco[q];
    if (r != NONE) {
        const uint32_t s = S.dep_off[r] + j;
        N.dm[u] = S.dm[s]; N.dl[u] = S.dl[s]; N.dn[u] = S.dn[s];
        N.ds[u] = S.ds[s];
    } else {
        const uint32_t s = d.dep_off[o.srcw[q]] + j;
        const uint8_t w = d.dep_wait ? d.dep_wait[s] : (uint8_t)1;
        N.dm[u] = d.dm[s]; N.dl[u] = d.dl[s]; N.dn[u] = d.dn[s];
        N.ds[u] = w;
        if (w) atomicAdd(&N.nwd[q], 1u);
    }
}

// sort word `word` of the dep slot at sorted position r: 0 node, 1 lsb, 2 msb (ts.hpp's word order)
__global__ __launch_bounds__(BLOCK) void k_wt_sortkey(Tab N, int word, const uint32_t *__restrict__ perm, uint64_t *__restrict__ key)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= N.nd) return;
    const uint32_t s = perm ? perm[r] : r;
    key[r] = word == 0 ? ts_w2(N.dn[s]) : word == 1 ? ts_w1(N.dl[s]) : N.dm[s];
}

// the new records' worklist: every dep slot of waiter perm[t] at its place in the new table, t ascending
__global__ __launch_bounds__(BLOCK) void k_wt_reg_trec(In d, Tab N, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ npos,
                                                       uint32_t *__restrict__ trec, uint32_t *__restrict__ wcnt)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= d.nw) return;
    const uint32_t w = perm ? perm[t] : t;
    trec[t] = npos[w];
    wcnt[t] = d.dep_off[w + 1] - d.dep_off[w];
}

__global__ __launch_bounds__(BLOCK) void k_wt_reg_wl(uint32_t n, uint32_t nt, Tab N, const uint32_t *__restrict__ trec,
                                                     const uint32_t *__restrict__ woff, uint32_t *__restrict__ wl)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t t = seg_of(woff, nt, p);
    wl[p] = N.dep_off[trec[t]] + (p - woff[t]);
}

__global__ __launch_bounds__(BLOCK) void k_wt_reg_out(uint32_t nw, Tab N, const uint32_t *__restrict__ npos, uint32_t *__restrict__ waiting,
                                                      uint64_t *__restrict__ om, uint64_t *__restrict__ ol, int32_t *__restrict__ on)
{
    const uint32_t w = blockIdx.x * BLOCK + threadIdx.x;
    if (w >= nw) return;
    const uint32_t q = npos[w];
    waiting[w] = N.nwd[q] + N.nwk[q];
    om[w] = N.am[q]; ol[w] = N.al[q]; on[w] = N.an[q];
}

// ---------------------------------------------------------------- notify: the worklist from the index

struct Ids {
    uint32_t n;
    const uint64_t *m, *l;
    const int32_t *nn;
};

// per changed dep: sorted unique; its range of the index
__global__ __launch_bounds__(BLOCK) void k_wt_ranges(Ids c, Tab S, uint32_t *__restrict__ clo, uint32_t *__restrict__ ccnt,
                                                     uint64_t *__restrict__ errs)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= c.n) return;
    const Ts id = ts_at(c.m, c.l, c.nn, i);
    if (i > 0 && cmp(ts_at(c.m, c.l, c.nn, i - 1), id) >= 0) err(errs, E_CHANGED);
    const uint32_t first = partition_point(0u, S.nd, [&](uint32_t m) { return cmp(dep_of(S, S.idx[m]), id) < 0; });
    clo[i] = first;
    ccnt[i] = partition_point(first, S.nd, [&](uint32_t m) { return cmp(dep_of(S, S.idx[m]), id) <= 0; }) - first;
}

__global__ __launch_bounds__(BLOCK) void k_wt_expand(uint32_t n, uint32_t nc, const uint32_t *__restrict__ coff, const uint32_t *__restrict__ clo,
                                                     Tab S, uint64_t *__restrict__ key)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t c = seg_of(coff, nc, p);
    key[p] = S.idx[clo[c] + (p - coff[c])];
}

// the sorted worklist: each slot, and whether it is the first of its record
__global__ __launch_bounds__(BLOCK) void k_wt_heads(uint32_t n, const uint64_t *__restrict__ key, Tab S, uint32_t *__restrict__ wl,
                                                    uint32_t *__restrict__ rec, uint32_t *__restrict__ head)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t s = key ? (uint32_t)key[p] : p, r = seg_of(S.dep_off, S.nr, s);
    wl[p] = s;
    rec[p] = r;
    const uint32_t s0 = p == 0 ? 0u : key ? (uint32_t)key[p - 1] : p - 1;
    head[p] = p == 0 || seg_of(S.dep_off, S.nr, s0) != r;
}

__global__ __launch_bounds__(BLOCK) void k_wt_trec(uint32_t n, const uint32_t *__restrict__ rec, const uint32_t *__restrict__ head,
                                                   const uint32_t *__restrict__ hpos, uint32_t *__restrict__ trec, uint32_t *__restrict__ woff)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    if (p == 0) woff[hpos[n]] = n;
    if (!head[p]) return;
    trec[hpos[p]] = rec[p];
    woff[hpos[p]] = p;
}

// ---------------------------------------------------------------- notify: the release pairs

struct Rel {
    uint32_t n;
    const uint64_t *tm, *tl, *key, *um, *ul;
    const int32_t *tn, *un;
    const uint8_t *flags;
};

__global__ __launch_bounds__(BLOCK) void k_wt_rel_find(Rel q, Tab S, uint64_t *__restrict__ rkey, uint64_t *__restrict__ errs)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= q.n) return;
    if (q.flags[i] > 1) err(errs, E_RELFLAGS);
    rkey[i] = find_ts(S.tm, S.tl, S.tn, 0, S.nr, ts_at(q.tm, q.tl, q.tn, i));
}

// the pairs sorted by record (stable): the first pair of a record applies all of them in input order
__global__ __launch_bounds__(BLOCK) void k_wt_rel_apply(Rel q, const uint64_t *__restrict__ rkey, const uint32_t *__restrict__ src, Tab W,
                                                        unsigned long long *__restrict__ cnt)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= q.n) return;
    const uint32_t r = (uint32_t)rkey[p];
    if (r == NONE) { atomicAdd(cnt + C_KIGN, 1ull); return; }
    if (p > 0 && (uint32_t)rkey[p - 1] == r) return;
    const uint32_t k0 = W.key_off[r], k1 = W.key_off[r + 1];
    const bool aod = W.flags[r] & ACC_WT_AWAITS_ONLY_DEPS;
    Ts eal{ W.am[r], W.al[r], W.an[r] };
    bool dirty = false;
    uint32_t released = 0, ignored = 0;
    for (uint32_t p2 = p; p2 < q.n && (uint32_t)rkey[p2] == r; ++p2) {
        const uint32_t i = src[p2];
        if (q.flags[i] & ACC_WT_REL_KEY) {
            const uint64_t c = q.key[i];
            const uint32_t lo = lower_bound(W.key, k0, k1, c);
            if (lo < k1 && W.key[lo] == c && W.kw[lo]) { W.kw[lo] = 0; ++released; }
            else ++ignored;
        }
        const Ts u = ts_at(q.um, q.ul, q.un, i);
        // executesAt.compareTo(executeAtLeast(Timestamp.NONE)) > 0 (local/CommandsForKey.java:1375, 1478): strictly above
        if (aod && !is_null(u) && (is_null(eal) || cmp(u, eal) > 0)) { eal = u; dirty = true; }
    }
    if (released) { W.nwk[r] -= released; atomicAdd(cnt + C_KREL, (unsigned long long)released); }
    if (ignored) atomicAdd(cnt + C_KIGN, (unsigned long long)ignored);
    if (dirty) { W.am[r] = eal.m; W.al[r] = eal.l; W.an[r] = eal.n; }
}

// ---------------------------------------------------------------- notify: the ready list

__global__ __launch_bounds__(BLOCK) void k_wt_ready(Tab W, Tab S, uint32_t *__restrict__ flag, unsigned long long *__restrict__ cnt)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= W.nr) return;
    const uint32_t before = S.nwd[r] + S.nwk[r], after = W.nwd[r] + W.nwk[r];
    flag[r] = before != 0 && after == 0;
    if (before != after) atomicAdd(cnt + C_CHANGED, (unsigned long long)(before - after));
}

__global__ __launch_bounds__(BLOCK) void k_wt_ready_emit(Tab W, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                         uint32_t *__restrict__ rec, uint64_t *__restrict__ tm, uint64_t *__restrict__ tl,
                                                         int32_t *__restrict__ tn, uint64_t *__restrict__ am, uint64_t *__restrict__ al,
                                                         int32_t *__restrict__ an)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= W.nr || !flag[r]) return;
    const uint32_t q = pos[r];
    rec[q] = r;
    tm[q] = W.tm[r]; tl[q] = W.tl[r]; tn[q] = W.tn[r];
    am[q] = W.am[r]; al[q] = W.al[r]; an[q] = W.an[r];
}

// ---------------------------------------------------------------- erase, view

__global__ __launch_bounds__(BLOCK) void k_wt_erase_keep(Ids c, Tab S, uint32_t *__restrict__ keep, uint64_t *__restrict__ errs)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < c.n && i > 0 && cmp(ts_at(c.m, c.l, c.nn, i - 1), ts_at(c.m, c.l, c.nn, i)) >= 0) err(errs, E_IDS);
    if (i < S.nr) keep[i] = find_ts(c.m, c.l, c.nn, 0, c.n, txn_of(S, i)) == NONE;
}

__global__ __launch_bounds__(BLOCK) void k_wt_erase_src(Tab S, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ kpos, Src o)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= S.nr || !keep[i]) return;
    const uint32_t q = kpos[i];
    o.srco[q] = i; o.srcw[q] = NONE;
    o.kc[q] = S.key_off[i + 1] - S.key_off[i];
    o.dc[q] = S.dep_off[i + 1] - S.dep_off[i];
}

// WaitingOn.nextWaitingOn: the highest WAITING dep slot
__global__ __launch_bounds__(BLOCK) void k_wt_next(Tab S, uint32_t *__restrict__ next)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= S.nr) return;
    const uint32_t d0 = S.dep_off[r], d1 = S.dep_off[r + 1];
    uint32_t v = NONE;
    if (S.nwd[r])
        for (uint32_t i = d1; i-- > d0;)
            if (S.ds[i] == ACC_WT_WAITING) { v = i - d0; break; }
    next[r] = v;
}

}  // namespace wt
}  // namespace acc

// The store: the live table and the spare set of its mutable columns (same capacities).
struct acc_waiting {
    int device = 0;
    acc::wt::Tab t{};
    uint8_t *kw2 = nullptr, *ds2 = nullptr;
    uint64_t *am2 = nullptr, *al2 = nullptr;
    int32_t *an2 = nullptr;
    uint32_t *nwd2 = nullptr, *nwk2 = nullptr;
};

namespace acc {

using namespace wt;

namespace {

template <class T>
T *dalloc(size_t n)
{
    T *p = nullptr;
    ACC_HIP(hipMalloc(&p, ((n ? n : 1) * sizeof(T) + 15) & ~(size_t)15));
    return p;
}

void free_cols(acc_waiting &w)
{
    Tab &t = w.t;
    for (void *p : { (void *)t.tm, (void *)t.tl, (void *)t.xm, (void *)t.xl, (void *)t.tn, (void *)t.xn, (void *)t.flags,
                     (void *)t.key_off, (void *)t.dep_off, (void *)t.key, (void *)t.dm, (void *)t.dl, (void *)t.dn, (void *)t.idx,
                     (void *)t.kw, (void *)t.ds, (void *)t.am, (void *)t.al, (void *)t.an, (void *)t.nwd, (void *)t.nwk,
                     (void *)w.kw2, (void *)w.ds2, (void *)w.am2, (void *)w.al2, (void *)w.an2, (void *)w.nwd2, (void *)w.nwk2 })
        (void)hipFree(p);
    const int dev = w.device;
    w = acc_waiting{};
    w.device = dev;
}

// a table under construction: freed unless it is committed into the store
struct Next {
    acc_waiting w;
    ~Next() { free_cols(w); }
    void records(uint32_t nr)
    {
        Tab &t = w.t;
        t.nr = nr;
        t.tm = dalloc<uint64_t>(nr); t.tl = dalloc<uint64_t>(nr); t.xm = dalloc<uint64_t>(nr); t.xl = dalloc<uint64_t>(nr);
        t.tn = dalloc<int32_t>(nr); t.xn = dalloc<int32_t>(nr);
        t.flags = dalloc<uint8_t>(nr);
        t.key_off = dalloc<uint32_t>((size_t)nr + 1); t.dep_off = dalloc<uint32_t>((size_t)nr + 1);
        t.am = dalloc<uint64_t>(nr); t.al = dalloc<uint64_t>(nr); t.an = dalloc<int32_t>(nr);
        t.nwd = dalloc<uint32_t>(nr); t.nwk = dalloc<uint32_t>(nr);
        w.am2 = dalloc<uint64_t>(nr); w.al2 = dalloc<uint64_t>(nr); w.an2 = dalloc<int32_t>(nr);
        w.nwd2 = dalloc<uint32_t>(nr); w.nwk2 = dalloc<uint32_t>(nr);
    }
    void slots(uint32_t nk, uint32_t nd)
    {
        Tab &t = w.t;
        t.nk = nk; t.nd = nd;
        t.key = dalloc<uint64_t>(nk); t.kw = dalloc<uint8_t>(nk); w.kw2 = dalloc<uint8_t>(nk);
        t.dm = dalloc<uint64_t>(nd); t.dl = dalloc<uint64_t>(nd); t.dn = dalloc<int32_t>(nd);
        t.ds = dalloc<uint8_t>(nd); w.ds2 = dalloc<uint8_t>(nd);
        t.idx = dalloc<uint32_t>(nd);
    }
};

Rc rc_of(const acc_rcmd *s) { return Rc{ s->n, s->tm, s->tl, s->em, s->el, s->tn, s->en, s->status }; }

// the live table with the spare mutable columns in place of its own
Tab spare_of(const acc_waiting &w)
{
    Tab t = w.t;
    t.kw = w.kw2; t.ds = w.ds2; t.am = w.am2; t.al = w.al2; t.an = w.an2; t.nwd = w.nwd2; t.nwk = w.nwk2;
    return t;
}

void swap_spare(acc_waiting &w)
{
    std::swap(w.t.kw, w.kw2); std::swap(w.t.ds, w.ds2); std::swap(w.t.am, w.am2); std::swap(w.t.al, w.al2);
    std::swap(w.t.an, w.an2); std::swap(w.t.nwd, w.nwd2); std::swap(w.t.nwk, w.nwk2);
}

uint64_t us_since(std::chrono::steady_clock::time_point t0)
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

// scans of the slot counts into the new table's offsets, the slot columns gathered, the index sorted
void gather(acc_ctx *ctx, Next &nx, const Tab &S, const In &d, const Src &o, uint32_t NR)
{
    nx.records(NR);
    Tab &N = nx.w.t;
    uint64_t *tot = ctx->get<uint64_t>("wt_tot", 2);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, o.kc, N.key_off, NR, true, N.key_off + NR);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, o.dc, N.dep_off, NR, true, N.dep_off + NR);
    sum_u32(ctx, o.kc, NR, tot);
    sum_u32(ctx, o.dc, NR, tot + 1);
    uint64_t nk = 0, nd = 0;
    {
        ReadBack rb(ctx);
        const auto h = rb.words((const uint64_t *)tot, 2);
        rb.wait();
        nk = h[0]; nd = h[1];
    }
    if (NR >= 0xFFFFFFFFull || nk >= 0xFFFFFFFFull || nd >= 0xFFFFFFFFull) fail(ACC_E_CAP, "the store would hold 2^32-1 records or slots");
    nx.slots((uint32_t)nk, (uint32_t)nd);
    if (NR == 0) {
        ACC_HIP(hipMemsetAsync(N.key_off, 0, 4, ctx->stream));
        ACC_HIP(hipMemsetAsync(N.dep_off, 0, 4, ctx->stream));
    }
    launch(ctx, "wt_fill_rec", k_wt_fill_rec, dim3(grid_for(NR, BLOCK)), dim3(BLOCK), 0, N, S, d, o);
    if (nk) launch(ctx, "wt_fill_keys", k_wt_fill_keys, dim3(grid_for(nk, BLOCK)), dim3(BLOCK), 0, N, S, d, o);
    if (nd) launch(ctx, "wt_fill_deps", k_wt_fill_deps, dim3(grid_for(nd, BLOCK)), dim3(BLOCK), 0, N, S, d, o);
    if (nd) {
        uint64_t *skey = ctx->get<uint64_t>("wt_skey", nd);
        static const char *const tag[3] = { "wt_s0", "wt_s1", "wt_s2" };
        const int bits[3] = { 32, 64, 64 };
        const uint32_t *perm = nullptr;
        for (int wd = 0; wd < 3; ++wd) {
            launch(ctx, "wt_sortkey", k_wt_sortkey, dim3(grid_for(nd, BLOCK)), dim3(BLOCK), 0, N, wd, perm, skey);
            perm = radix_sort(ctx, tag[wd], skey, perm, nd, bits[wd]).vals;
        }
        ACC_HIP(hipMemcpyAsync(N.idx, perm, (size_t)nd * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
}

void commit(acc_ctx *ctx, acc_waiting *w, Next &nx)
{
    ctx->sync();
    std::swap(*w, nx.w);   // the previous table is freed with nx
    w->device = nx.w.device;
}

Src src_bufs(acc_ctx *ctx, size_t n)
{
    return Src{ ctx->get<uint32_t>("wt_srco", n), ctx->get<uint32_t>("wt_srcw", n), ctx->get<uint32_t>("wt_kc", n),
                ctx->get<uint32_t>("wt_dc", n) };
}

struct Counts { uint64_t v[C_N]; };

// the two evaluation passes over a worklist (W: the columns written; S: the table as the call found it)
void evaluate(acc_ctx *ctx, const Work &wk, uint32_t nt, const uint32_t *trec, const uint32_t *woff, uint32_t forced, const Tab &W,
              const Tab &S, const Rc &rc, unsigned long long *cnt, uint64_t *errs)
{
    if (wk.n == 0 || nt == 0) return;
    launch(ctx, "wt_own", k_wt_own, dim3(grid_for(wk.n, BLOCK)), dim3(BLOCK), 0, wk, W, S, rc, cnt);
    const Walk k{ nt, trec, woff, wk, forced, cnt, errs };
    if (forced != T_WAVE) launch(ctx, "wt_walk_lane", k_wt_walk_lane, dim3(grid_for(nt, BLOCK)), dim3(BLOCK), 0, k, W, S, rc);
    if (forced != T_LANE) launch_waves(ctx, "wt_walk_wave", k_wt_walk_wave, nt, k, W, S, rc);
}

Work work_bufs(acc_ctx *ctx, uint32_t n, const uint32_t *wl)
{
    return Work{ n, wl, ctx->get<uint8_t>("wt_own", n), ctx->get<uint32_t>("wt_drow", n), ctx->get<uint32_t>("wt_ridx", n) };
}

void check_mem_tier(uint32_t mem, uint32_t tier)
{
    if (mem != ACC_MEM_HOST && mem != ACC_MEM_DEVICE) fail(ACC_E_ARG, "mem must be ACC_MEM_HOST or ACC_MEM_DEVICE");
    if (tier > ACC_WT_TIER_WAVE) fail(ACC_E_ARG, "tier must be 0 (default) or ACC_WT_TIER_LANE / _WAVE");
}

void store_stats(acc_ctx *ctx, const acc_waiting *w)
{
    ctx->stat("wt.records", w->t.nr);
    ctx->stat("wt.slots", (uint64_t)w->t.nk + w->t.nd);
}

}  // namespace

acc_waiting *waiting_new(int device)
{
    acc_waiting *w = new acc_waiting();
    w->device = device;
    return w;
}

void waiting_free(acc_waiting *w)
{
    if (!w) return;
    (void)hipSetDevice(w->device);
    free_cols(*w);
    delete w;
}

void waiting_register(acc_ctx *ctx, acc_waiting *w, acc_rcmd *rcmd, const acc_waiting_register_in *in, acc_waiting_register_out *out)
{
    if (!w || !rcmd || !in || !out) fail(ACC_E_ARG, "null argument");
    check_mem_tier(in->mem, in->tier);
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = ctx->stream;
    const uint32_t nw = in->n_waiters, mem = in->mem, forced = in->tier;
    *out = acc_waiting_register_out{};
    ctx->stat("wt.register_evaluated", 0);
    ctx->stat("wt.propagated", 0);
    if (nw == 0) { store_stats(ctx, w); ctx->stat("wt.register_us", us_since(t0)); return; }
    if (in->n_keys >= 0xFFFFFFFFull || in->n_deps >= 0xFFFFFFFFull || (uint64_t)w->t.nr + nw >= 0xFFFFFFFFull)
        fail(ACC_E_CAP, "the store would hold 2^32-1 records or slots");
    const Tab S = w->t;
    const Rc rc = rc_of(rcmd);
    In d{};
    d.nw = nw; d.NK = (uint32_t)in->n_keys; d.ND = (uint32_t)in->n_deps;
    d.tm = stage_in(ctx, "wt_in_tm", in->txn_id.msb, nw, mem);
    d.tl = stage_in(ctx, "wt_in_tl", in->txn_id.lsb, nw, mem);
    d.tn = stage_in(ctx, "wt_in_tn", in->txn_id.node, nw, mem);
    d.xm = stage_in(ctx, "wt_in_xm", in->execute_at.msb, nw, mem);
    d.xl = stage_in(ctx, "wt_in_xl", in->execute_at.lsb, nw, mem);
    d.xn = stage_in(ctx, "wt_in_xn", in->execute_at.node, nw, mem);
    d.key_off = stage_in(ctx, "wt_in_koff", in->key_off, (size_t)nw + 1, mem);
    d.dep_off = stage_in(ctx, "wt_in_doff", in->dep_off, (size_t)nw + 1, mem);
    d.key = stage_in(ctx, "wt_in_key", in->key, d.NK, mem);
    d.dm = stage_in(ctx, "wt_in_dm", in->dep.msb, d.ND, mem);
    d.dl = stage_in(ctx, "wt_in_dl", in->dep.lsb, d.ND, mem);
    d.dn = stage_in(ctx, "wt_in_dn", in->dep.node, d.ND, mem);
    d.key_wait = in->key_wait ? stage_in(ctx, "wt_in_kw", in->key_wait, d.NK, mem) : nullptr;
    d.dep_wait = in->dep_wait ? stage_in(ctx, "wt_in_dw", in->dep_wait, d.ND, mem) : nullptr;

    // ---- 1. the waiters: validated, ranked, placed
    uint64_t *errs = ctx->get<uint64_t>("wt_errs", 1);
    unsigned long long *cnt = ctx->get<unsigned long long>("wt_cnt", C_N);
    ACC_HIP(hipMemsetAsync(errs, 0, 8, st));
    ACC_HIP(hipMemsetAsync(cnt, 0, C_N * 8, st));
    uint64_t *wd[3] = { ctx->get<uint64_t>("wt_w0", nw), ctx->get<uint64_t>("wt_w1", nw), ctx->get<uint64_t>("wt_w2", nw) };
    uint32_t *lb = ctx->get<uint32_t>("wt_lb", nw), *npos = ctx->get<uint32_t>("wt_npos", nw);
    launch(ctx, "wt_reg_waiters", k_wt_reg_waiters, dim3(grid_for(nw, BLOCK)), dim3(BLOCK), 0, d, S, rc, wd[0], wd[1], wd[2], lb, errs);
    const uint64_t *words[3] = { wd[0], wd[1], wd[2] };
    const DenseRank dr = dense_rank(ctx, "wt_dr", nw, 3, words, nullptr, nullptr, false);
    auto raise_errs = [](uint64_t e) {
        if (e & E_KIND) fail(ACC_E_ARG, "Kind.ofOrdinal: invalid kind ordinal in a waiter's TxnId flags");
        if (e & E_OFF) fail(ACC_E_ARG, "key_off / dep_off must start at 0, be non-decreasing and end at n_keys / n_deps");
        if (e & E_DUP) fail(ACC_E_ARG, "a waiter is already registered");
        if (e & E_KEYS) fail(ACC_E_ARG, "keys of a waiter must be sorted and unique");
        if (e & E_DEPS) fail(ACC_E_ARG, "deps of a waiter must be sorted and unique");
        if (e & E_DOMAIN) fail(ACC_E_ARG, "a dep TxnId must be range-domain (rangeDeps.txnIds)");
        if (e & E_WAIT) fail(ACC_E_ARG, "a wait byte must be 0 or 1");
        if (e & E_APPLIED) fail(ACC_E_STATE, "a waiter is held at Applied or beyond by the range-command store");
        if (e & E_INVARIANT) fail(ACC_E_STATE, "an Applied dep's own record is still waiting");
    };
    {
        ReadBack rb(ctx);
        const auto h_err = rb.u64(errs), h_cnt = rb.u64(dr.count_dev);
        rb.wait();
        const uint64_t e = h_err;
        raise_errs(e & (E_KIND | E_OFF));
        if ((uint64_t)h_cnt != nw) fail(ACC_E_ARG, "waiter TxnIds of one call must be distinct");
        raise_errs(e);
    }
    if (d.NK) launch(ctx, "wt_reg_keys", k_wt_reg_keys, dim3(grid_for(d.NK, BLOCK)), dim3(BLOCK), 0, d, errs);
    if (d.ND) launch(ctx, "wt_reg_deps", k_wt_reg_deps, dim3(grid_for(d.ND, BLOCK)), dim3(BLOCK), 0, d, errs);
    const uint32_t NR = S.nr + nw;
    const Src o = src_bufs(ctx, NR);
    launch(ctx, "wt_place", k_wt_place, dim3(grid_for(NR, BLOCK)), dim3(BLOCK), 0, d, S, (const uint32_t *)dr.rank, dr.perm,
           (const uint32_t *)lb, o, npos);
    {
        ReadBack rb(ctx);
        const auto h_err = rb.u64(errs);
        rb.wait();
        raise_errs(h_err);
    }

    // ---- 2. the next table
    Next nx;
    nx.w.device = w->device;
    gather(ctx, nx, S, d, o, NR);
    const Tab N = nx.w.t;

    // ---- 3. the new records evaluated against the table as it stood
    uint32_t *trec = ctx->get<uint32_t>("wt_trec", nw), *wcnt = ctx->get<uint32_t>("wt_wcnt", nw);
    uint32_t *woff = ctx->get<uint32_t>("wt_woff", (size_t)nw + 1), *wl = ctx->get<uint32_t>("wt_wl", d.ND);
    launch(ctx, "wt_reg_trec", k_wt_reg_trec, dim3(grid_for(nw, BLOCK)), dim3(BLOCK), 0, d, N, dr.perm, (const uint32_t *)npos, trec, wcnt);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, wcnt, woff, nw, true, woff + nw);
    if (d.ND)
        launch(ctx, "wt_reg_wl", k_wt_reg_wl, dim3(grid_for(d.ND, BLOCK)), dim3(BLOCK), 0, d.ND, nw, N, (const uint32_t *)trec,
               (const uint32_t *)woff, wl);
    evaluate(ctx, work_bufs(ctx, d.ND, wl), nw, trec, woff, forced, N, S, rc, cnt, errs);
    uint32_t *waiting = ctx->get<uint32_t>("wt_out_waiting", nw);
    uint64_t *om = ctx->get<uint64_t>("wt_out_am", nw), *ol = ctx->get<uint64_t>("wt_out_al", nw);
    int32_t *on = ctx->get<int32_t>("wt_out_an", nw);
    launch(ctx, "wt_reg_out", k_wt_reg_out, dim3(grid_for(nw, BLOCK)), dim3(BLOCK), 0, nw, N, (const uint32_t *)npos, waiting, om, ol, on);
    Counts c{};
    {
        ReadBack rb(ctx);
        const auto h_err = rb.u64(errs);
        const auto h_c = rb.words((const uint64_t *)cnt, C_N);
        rb.wait();
        raise_errs(h_err);
        for (int i = 0; i < C_N; ++i) c.v[i] = h_c[i];
    }
    commit(ctx, w, nx);
    *out = acc_waiting_register_out{ nw, 0u, waiting, acc_ts_cols{ om, ol, on } };
    store_stats(ctx, w);
    ctx->stat("wt.register_evaluated", c.v[C_EVAL]);
    ctx->stat("wt.propagated", c.v[C_PROP]);
    ctx->stat("wt.register_us", us_since(t0));
}

void waiting_notify(acc_ctx *ctx, acc_waiting *w, acc_rcmd *rcmd, const acc_waiting_notify_in *in, acc_waiting_notify_out *out)
{
    if (!w || !rcmd || !in || !out) fail(ACC_E_ARG, "null argument");
    check_mem_tier(in->mem, in->tier);
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = ctx->stream;
    const uint32_t mem = in->mem, forced = in->tier, nrel = in->n_rel;
    const bool all = in->changed.msb == nullptr;
    const uint32_t nc = all ? 0u : in->n_changed;
    const Tab S = w->t;
    const Tab W = spare_of(*w);
    const Rc rc = rc_of(rcmd);
    *out = acc_waiting_notify_out{};
    for (const char *s : { "wt.notify_slots", "wt.propagated", "wt.ready", "wt.key_released", "wt.key_ignored" }) ctx->stat(s, 0);

    uint64_t *errs = ctx->get<uint64_t>("wt_errs", 1);
    unsigned long long *cnt = ctx->get<unsigned long long>("wt_cnt", C_N);
    ACC_HIP(hipMemsetAsync(errs, 0, 8, st));
    ACC_HIP(hipMemsetAsync(cnt, 0, C_N * 8, st));
    auto raise_errs = [](uint64_t e) {
        if (e & E_CHANGED) fail(ACC_E_ARG, "changed must be sorted and unique");
        if (e & E_RELFLAGS) fail(ACC_E_ARG, "a rel_flags byte must be 0 or ACC_WT_REL_KEY");
        if (e & E_INVARIANT) fail(ACC_E_STATE, "an Applied dep's own record is still waiting");
    };

    // ---- 1. the worklist: the index ranges of the changed deps, sorted by slot
    const Ids ch{ nc, stage_in(ctx, "wt_in_cm", in->changed.msb, nc, mem), stage_in(ctx, "wt_in_cl", in->changed.lsb, nc, mem),
                  stage_in(ctx, "wt_in_cn", in->changed.node, nc, mem) };
    uint32_t NW = all ? S.nd : 0u;
    uint32_t *clo = ctx->get<uint32_t>("wt_clo", nc), *ccnt = ctx->get<uint32_t>("wt_ccnt", nc);
    uint32_t *coff = ctx->get<uint32_t>("wt_coff", (size_t)nc + 1);
    if (nc) {
        uint64_t *tot = ctx->get<uint64_t>("wt_tot", 2);
        launch(ctx, "wt_ranges", k_wt_ranges, dim3(grid_for(nc, BLOCK)), dim3(BLOCK), 0, ch, S, clo, ccnt, errs);
        scan<uint32_t, OpAdd<uint32_t>>(ctx, ccnt, coff, nc, true, coff + nc);
        sum_u32(ctx, ccnt, nc, tot);
        ReadBack rb(ctx);
        const auto h_err = rb.u64(errs), h_n = rb.u64(tot);
        rb.wait();
        raise_errs(h_err);
        if ((uint64_t)h_n > S.nd) fail(ACC_E_STATE, "internal: more index entries than slots");
        NW = (uint32_t)(uint64_t)h_n;
    }
    // the mutable columns of the spare set start as the live ones
    if (S.nd) ACC_HIP(hipMemcpyAsync(W.ds, S.ds, S.nd, hipMemcpyDeviceToDevice, st));
    if (S.nk) ACC_HIP(hipMemcpyAsync(W.kw, S.kw, S.nk, hipMemcpyDeviceToDevice, st));
    if (S.nr) {
        ACC_HIP(hipMemcpyAsync(W.am, S.am, (size_t)S.nr * 8, hipMemcpyDeviceToDevice, st));
        ACC_HIP(hipMemcpyAsync(W.al, S.al, (size_t)S.nr * 8, hipMemcpyDeviceToDevice, st));
        ACC_HIP(hipMemcpyAsync(W.an, S.an, (size_t)S.nr * 4, hipMemcpyDeviceToDevice, st));
        ACC_HIP(hipMemcpyAsync(W.nwd, S.nwd, (size_t)S.nr * 4, hipMemcpyDeviceToDevice, st));
        ACC_HIP(hipMemcpyAsync(W.nwk, S.nwk, (size_t)S.nr * 4, hipMemcpyDeviceToDevice, st));
    }
    if (NW) {
        const uint64_t *skey = nullptr;
        if (!all) {
            uint64_t *key = ctx->get<uint64_t>("wt_wkey", NW);
            launch(ctx, "wt_expand", k_wt_expand, dim3(grid_for(NW, BLOCK)), dim3(BLOCK), 0, NW, nc, (const uint32_t *)coff,
                   (const uint32_t *)clo, S, key);
            skey = radix_sort_keys(ctx, "wt_ws", key, NW, 0, bits_for(S.nd - 1));
        }
        uint32_t *wl = ctx->get<uint32_t>("wt_wl", NW), *rec = ctx->get<uint32_t>("wt_rec", NW), *head = ctx->get<uint32_t>("wt_head", NW);
        uint32_t *hpos = ctx->get<uint32_t>("wt_hpos", (size_t)NW + 1);
        launch(ctx, "wt_heads", k_wt_heads, dim3(grid_for(NW, BLOCK)), dim3(BLOCK), 0, NW, skey, S, wl, rec, head);
        scan<uint32_t, OpAdd<uint32_t>>(ctx, head, hpos, NW, true, hpos + NW);
        uint32_t NT = 0;
        {
            ReadBack rb(ctx);
            const auto h_nt = rb.u32(hpos + NW);
            rb.wait();
            NT = h_nt;
            if (NT == 0 || NT > NW || NT > S.nr) fail(ACC_E_STATE, "internal: touched records of the worklist");
        }
        uint32_t *trec = ctx->get<uint32_t>("wt_trec", NT), *woff = ctx->get<uint32_t>("wt_woff", (size_t)NT + 1);
        launch(ctx, "wt_trec", k_wt_trec, dim3(grid_for(NW, BLOCK)), dim3(BLOCK), 0, NW, (const uint32_t *)rec, (const uint32_t *)head,
               (const uint32_t *)hpos, trec, woff);
        evaluate(ctx, work_bufs(ctx, NW, wl), NT, trec, woff, forced, W, S, rc, cnt, errs);
    }

    // ---- 2. the release pairs, by record
    if (nrel) {
        const Rel q{ nrel,
                     stage_in(ctx, "wt_in_rm", in->rel_txn.msb, nrel, mem), stage_in(ctx, "wt_in_rl", in->rel_txn.lsb, nrel, mem),
                     stage_in(ctx, "wt_in_rk", in->rel_key, nrel, mem),
                     stage_in(ctx, "wt_in_um", in->rel_until.msb, nrel, mem), stage_in(ctx, "wt_in_ul", in->rel_until.lsb, nrel, mem),
                     stage_in(ctx, "wt_in_rn", in->rel_txn.node, nrel, mem), stage_in(ctx, "wt_in_un", in->rel_until.node, nrel, mem),
                     stage_in(ctx, "wt_in_rf", in->rel_flags, nrel, mem) };
        uint64_t *rkey = ctx->get<uint64_t>("wt_rkey", nrel);
        launch(ctx, "wt_rel_find", k_wt_rel_find, dim3(grid_for(nrel, BLOCK)), dim3(BLOCK), 0, q, S, rkey, errs);
        const Sorted so = radix_sort(ctx, "wt_rs", rkey, nullptr, nrel, 32);
        launch(ctx, "wt_rel_apply", k_wt_rel_apply, dim3(grid_for(nrel, BLOCK)), dim3(BLOCK), 0, q, (const uint64_t *)so.keys,
               (const uint32_t *)so.vals, W, cnt);
    }

    // ---- 3. the ready list
    uint32_t *flag = ctx->get<uint32_t>("wt_rflag", S.nr), *rpos = ctx->get<uint32_t>("wt_rpos", (size_t)S.nr + 1);
    if (S.nr) launch(ctx, "wt_ready", k_wt_ready, dim3(grid_for(S.nr, BLOCK)), dim3(BLOCK), 0, W, S, flag, cnt);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, flag, rpos, S.nr, true, rpos + S.nr);
    uint32_t NRDY = 0;
    Counts c{};
    {
        ReadBack rb(ctx);
        const auto h_err = rb.u64(errs);
        const auto h_n = rb.u32(rpos + S.nr);
        const auto h_c = rb.words((const uint64_t *)cnt, C_N);
        rb.wait();
        raise_errs(h_err);
        NRDY = S.nr ? (uint32_t)h_n : 0u;
        if (NRDY > S.nr) fail(ACC_E_STATE, "internal: more ready records than records");
        for (int i = 0; i < C_N; ++i) c.v[i] = h_c[i];
    }
    uint32_t *rrec = ctx->get<uint32_t>("wt_out_rec", NRDY);
    uint64_t *tm = ctx->get<uint64_t>("wt_out_tm", NRDY), *tl = ctx->get<uint64_t>("wt_out_tl", NRDY);
    uint64_t *am = ctx->get<uint64_t>("wt_out_am", NRDY), *al = ctx->get<uint64_t>("wt_out_al", NRDY);
    int32_t *tn = ctx->get<int32_t>("wt_out_tn", NRDY), *an = ctx->get<int32_t>("wt_out_an", NRDY);
    if (NRDY)
        launch(ctx, "wt_ready_emit", k_wt_ready_emit, dim3(grid_for(S.nr, BLOCK)), dim3(BLOCK), 0, W, (const uint32_t *)flag,
               (const uint32_t *)rpos, rrec, tm, tl, tn, am, al, an);
    ctx->sync();
    swap_spare(*w);
    *out = acc_waiting_notify_out{ NRDY, 0u, c.v[C_CHANGED], rrec, acc_ts_cols{ tm, tl, tn }, acc_ts_cols{ am, al, an } };
    store_stats(ctx, w);
    ctx->stat("wt.notify_slots", c.v[C_EVAL]);
    ctx->stat("wt.propagated", c.v[C_PROP]);
    ctx->stat("wt.ready", NRDY);
    ctx->stat("wt.key_released", c.v[C_KREL]);
    ctx->stat("wt.key_ignored", c.v[C_KIGN]);
    ctx->stat("wt.notify_us", us_since(t0));
}

void waiting_erase(acc_ctx *ctx, acc_waiting *w, const acc_waiting_erase_in *in)
{
    if (!w || !in) fail(ACC_E_ARG, "null argument");
    check_mem_tier(in->mem, 0);
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = ctx->stream;
    const uint32_t n = in->n_ids, mem = in->mem;
    const Tab S = w->t;
    ctx->stat("wt.erased", 0);
    const Ids ids{ n, stage_in(ctx, "wt_in_cm", in->txn_id.msb, n, mem), stage_in(ctx, "wt_in_cl", in->txn_id.lsb, n, mem),
                   stage_in(ctx, "wt_in_cn", in->txn_id.node, n, mem) };
    uint64_t *errs = ctx->get<uint64_t>("wt_errs", 1);
    ACC_HIP(hipMemsetAsync(errs, 0, 8, st));
    uint32_t *keep = ctx->get<uint32_t>("wt_keep", S.nr), *kpos = ctx->get<uint32_t>("wt_kpos", (size_t)S.nr + 1);
    const uint32_t span = std::max(n, S.nr);
    if (span) launch(ctx, "wt_erase_keep", k_wt_erase_keep, dim3(grid_for(span, BLOCK)), dim3(BLOCK), 0, ids, S, keep, errs);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, keep, kpos, S.nr, true, kpos + S.nr);
    uint32_t NR = 0;
    {
        ReadBack rb(ctx);
        const auto h_err = rb.u64(errs);
        const auto h_n = rb.u32(kpos + S.nr);
        rb.wait();
        if ((uint64_t)h_err & E_IDS) fail(ACC_E_ARG, "txn_id must be sorted and unique");
        NR = S.nr ? (uint32_t)h_n : 0u;
        if (NR > S.nr) fail(ACC_E_STATE, "internal: a compaction grew the table");
    }
    if (NR != S.nr) {
        const Src o = src_bufs(ctx, NR);
        launch(ctx, "wt_erase_src", k_wt_erase_src, dim3(grid_for(S.nr, BLOCK)), dim3(BLOCK), 0, S, (const uint32_t *)keep,
               (const uint32_t *)kpos, o);
        Next nx;
        nx.w.device = w->device;
        gather(ctx, nx, S, In{}, o, NR);
        commit(ctx, w, nx);
    }
    store_stats(ctx, w);
    ctx->stat("wt.erased", S.nr - NR);
    ctx->stat("wt.erase_us", us_since(t0));
}

void waiting_view(acc_ctx *ctx, acc_waiting *w, acc_waiting_table *out)
{
    if (!w || !out) fail(ACC_E_ARG, "null argument");
    const Tab &t = w->t;
    uint32_t *next = ctx->get<uint32_t>("wt_next", t.nr);
    uint32_t *z = ctx->get<uint32_t>("wt_zero", 4);   // an empty store has no arrays yet: key_off = dep_off = one zero
    ACC_HIP(hipMemsetAsync(z, 0, 16, ctx->stream));
    if (t.nr) launch(ctx, "wt_next", k_wt_next, dim3(grid_for(t.nr, BLOCK)), dim3(BLOCK), 0, t, next);
    ctx->sync();
    *out = acc_waiting_table{ t.nr, 0u, t.nk, t.nd, acc_ts_cols{ t.tm, t.tl, t.tn }, acc_ts_cols{ t.xm, t.xl, t.xn },
                              acc_ts_cols{ t.am, t.al, t.an }, t.flags, t.key_off ? t.key_off : z, t.key, t.kw,
                              t.dep_off ? t.dep_off : z, acc_ts_cols{ t.dm, t.dl, t.dn }, t.ds, t.nwd, t.nwk, next };
    store_stats(ctx, w);
}

}  // namespace acc
