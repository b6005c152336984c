// keydeps.hpp — what the KeyDeps translation units share (keydeps.hip: CFK build and the run-based path;
// keydeps_replay.hip: the exact replay path; keydeps_mixed.hip: range-domain txns; recovery.hip reads the record):
// the record of a batch's built CommandsForKey (CfkBuild), the stage entry points, and the exact-replay query
// (CfkView, make_query*, run_query), which is device code in a header because keydeps_replay.hip's and
// keydeps_mixed.hip's kernels both run it.
#pragma once

#include "dict.hpp"
#include "search.hpp"

namespace acc {

struct PairPlan {
    Runs rk;       // key code compaction
    int rbits;     // txn-rank bits in the composite (0 when the batch is already in TxnId order)
    int mode;      // 0: key only (sorted batch), 1: (key << rbits) | rank, 2: key only after a rank pre-sort,
                   // 3: (key << 32) | pair index, keys-only sort (sorted batch, key within 32 bits);
                   // 4: (key << 32) | owner << sb | slot (mode 3 with the pair's txn packed: the CFK columns gather the
                   //    16-MB txn records directly instead of a 16-B per-pair copy)
    int sb;        // mode 4: bits of the key slot within its txn
};

struct V2Cols {
    uint4 *rdir;          // [P / RD_W + 1] chunks of 16 u32, as 4 x uint4
    uint32_t *list_rank;  // class lists (TxnId ranks), list l at bases[l]
    uint32_t *bc_rank, *bc_exec;  // bumped committed, position order
    uint8_t *bc_kind;
    uint64_t *bc_pm_in;   // (seg << 32) | exec+1, for the segmented prefix max
    uint64_t *bc_key;     // (seg << rbits) | exec, for the (seg, executeAt) sort; null when the build made that order
                          // from the txn side (CfkBuild::bc_side)
};

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m)
{
    uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

// in-LDS bitonic sort of n2 (power of two, >= 128) u64 entries by one wave
__device__ __forceinline__ void wave_bitonic_lds(uint64_t *buf, uint32_t n2)
{
    const uint32_t lane = lane_id();
    for (uint32_t k = 2; k <= n2; k <<= 1) {
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            for (uint32_t i = lane; i < n2; i += 64) {
                uint32_t l = i ^ jj;
                if (l > i) {
                    uint64_t a = buf[i], b = buf[l];
                    bool up = (i & k) == 0;
                    if ((a > b) == up) { buf[i] = b; buf[l] = a; }
                }
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        }
    }
}

// ---------------------------------------------------------------- the conflict scan

struct CfkView {
    const uint32_t *seg_start, *s_rank, *s_exec, *seg_incl, *pair_pos, *owner, *rank;
    const uint8_t *s_info;
    const uint32_t *cl_start, *cl_exec, *lastw;   // lastw = inclusive max-scan of (isWrite ? c+1 : 0)
    const uint32_t *pmax;                          // low 32 bits of the segmented prefix max (exec+1)
    const uint32_t *cum_u, *u_pos;
    const uint64_t *tl;
    uint32_t n;
    const uint32_t *vseg;   // non-null: query j is (owner[j], segment vseg[j]) (range-domain txns, no CFK member)
};

struct Query {
    uint32_t s0, pos, scan_start, ub, ue, trank, wk;
    bool p1, has_m;
    uint32_t m;
};

__device__ __forceinline__ Query make_query_ts(const CfkView &v, uint32_t t, uint32_t seg);

__device__ __forceinline__ Query make_query(const CfkView &v, uint32_t j)
{
    return make_query_ts(v, v.owner[j], v.vseg ? v.vseg[j] : v.seg_incl[v.pair_pos[j]] - 1);
}

// the query of txn t against CFK segment seg
__device__ __forceinline__ Query make_query_ts(const CfkView &v, uint32_t t, uint32_t seg)
{
    Query q;
    uint32_t s0 = v.seg_start[seg], s1 = v.seg_start[seg + 1];
    uint32_t S = v.rank[v.n + t];          // startedBefore = T.executeAt
    q.trank = v.rank[t];
    q.p1 = S != q.trank;                   // p1 = executeAt.equals(txnId) ? null : txnId
    q.wk = witnesses((uint32_t)(v.tl[t] >> 1) & 7u);
    q.s0 = s0;
    // insertPos(0, startedBefore): first txn with TxnId >= S (CommandsForKey.java:1698-1703)
    q.pos = lower_bound(v.s_rank, s0, s1, S);
    // maxCommittedBefore (CommandsForKey.java:618-625): FAST bisection of S over committed[] by executeAt
    uint32_t c0 = v.cl_start[seg], c1 = v.cl_start[seg + 1];
    uint32_t from = c0, to = c1;
    long i = -1;
    bool found = false;
    while (from < to) {
        uint32_t mid = (from + to) >> 1;
        uint32_t e = v.cl_exec[mid];
        if (S < e) to = mid;
        else if (S > e) from = mid + 1;
        else { i = (long)mid - 1; found = true; break; }
    }
    if (!found) i = (long)to - 1;
    q.has_m = false;
    q.m = 0;
    if (i >= (long)c0) {
        uint32_t w = v.lastw[i];           // greatest Write index <= i, +1 (0: none anywhere before)
        if (w != 0 && w - 1 >= c0) { q.has_m = true; q.m = v.cl_exec[w - 1]; }
    }
    // Committed entries below scanStart all have executeAt < M (prefix max < M): pruned
    q.scan_start = q.has_m ? lower_bound(v.pmax, s0, q.pos, q.m + 1) : s0;
    q.ub = v.cum_u[s0];
    q.ue = v.cum_u[q.scan_start];
    return q;
}

// EMIT: every entry to out[0..c); FIRST (count pass): only the first entry, to out[0]
template <bool EMIT, bool FIRST = false>
__device__ __forceinline__ uint32_t run_query(const CfkView &v, const Query &q, uint32_t *__restrict__ out)
{
    uint32_t c = 0;
    // uncommitted (HISTORICAL / PREACCEPTED / ACCEPTED) entries below scanStart: always witnessed
    for (uint32_t u = q.ub; u < q.ue; ++u) {
        uint32_t p = v.u_pos[u];
        uint32_t kind = v.s_info[p] >> 3;
        if (!((q.wk >> kind) & 1u)) continue;
        uint32_t r = v.s_rank[p];
        if (q.p1 && r == q.trank) continue;
        if (EMIT) out[c] = r;
        else if (FIRST && c == 0) out[0] = r;
        ++c;
    }
    // [scanStart, insertPos): the reference's per-entry switch (CommandsForKey.java:628-647)
    for (uint32_t p = q.scan_start; p < q.pos; ++p) {
        uint32_t info = v.s_info[p];
        uint32_t st = info & 7u, kind = info >> 3;
        if (!((q.wk >> kind) & 1u)) continue;
        if (st == 0 || st == 7) continue;                                    // TRANSITIVELY_KNOWN, INVALID
        if (st >= 4 && st <= 6 && q.has_m && v.s_exec[p] < q.m) continue;   // pruned committed
        uint32_t r = v.s_rank[p];
        if (q.p1 && r == q.trank) continue;
        if (EMIT) out[c] = r;
        else if (FIRST && c == 0) out[0] = r;
        ++c;
    }
    return c;
}

// ---------------------------------------------------------------- the CFK of a batch

// What a caller needs of the build beyond plain KeyDeps. acc_keydeps_batch asks for neither (config 2's time depends
// on it: no seg_key is written, and pair_pos only when a later stage turns out to need it).
struct CfkOpts {
    bool seg_keys = false;   // seg_key (every segment's key code) and pair_pos, for the consumers that search the sorted
                             // keys or address pairs by index (range-domain queries, recovery)
    bool sparse = false;     // many txns list no keys (a mixed batch's range txns): the TxnId compaction walks only the
                             // txns that have entries
};

// The CommandsForKey snapshot of a key batch as build_cfk leaves it: pairs sorted by (key, TxnId rank) = one segment
// per key, entries in CommandsForKey.txns order, with the columns the later stages read. Device pointers owned by the
// context, valid until its next compute call. cfk = false: the batch has no pairs; only n, P and key_off are set and
// ctx->kd_view holds the (empty) KeyDeps.
struct CfkBuild {
    bool cfk = false;
    CfkOpts opts;
    uint32_t n = 0;
    size_t P = 0;
    // staged inputs
    const uint64_t *tm = nullptr, *tl = nullptr, *em = nullptr, *el = nullptr;
    const int32_t *tn = nullptr, *en = nullptr;
    const uint8_t *status = nullptr;
    const uint32_t *key_off = nullptr;
    const uint64_t *key_code = nullptr;
    Dictionary dict;                  // final: a deferred tie check has been resolved
    uint32_t *owner = nullptr;        // [P] txn of every pair
    uint64_t *g = nullptr;            // the prep / dictionary flag words (PREP_G_WORDS)
    bool ties = false;                // an executeAt equals another timestamp: KeyDeps by the replay path
    PairPlan pp{};
    uint32_t *perm = nullptr;         // [P] entry -> input pair index
    uint32_t *pair_pos = nullptr;     // [P] input pair index -> entry; filled only when have_pair_pos
    bool have_pair_pos = false;
    uint32_t *seg_incl = nullptr;     // [P] inclusive count of segment starts (segment of entry p = seg_incl[p] - 1)
    uint32_t *seg_start = nullptr;    // [nseg + 1] first entry of each segment
    uint64_t *seg_key = nullptr;      // [nseg] key code of each segment, ascending (opts.seg_keys, else null)
    uint32_t nseg = 0;                // set by cfk_snapshot only (one more device read)
    uint32_t *s_rank = nullptr, *s_exec = nullptr;   // [P] TxnId / executeAt rank per entry
    uint8_t *s_info = nullptr;        // [P] status | kind << 3
    uint4 *tinfo = nullptr;           // [n] the per-txn records (k_txn_info)
    uint32_t *bigflag = nullptr;      // [n] zeroed by the column kernels, set by the count pass
    uint32_t htot[16] = {};           // the tile counts' totals as read at the build's sync ([6] = bumped committed)
    // the bumped committed entries in (segment, executeAt) order, made by the build on the side lane from the txn side
    // (bc_side; else keydeps_runs sorts cols.bc_key): executeAt ranks, nearest-Write index + 1 (inclusive prefix max)
    bool bc_side = false;
    uint32_t *bcs_exec = nullptr;
    uint64_t *bcs_lastw64 = nullptr;
    V2Cols cols{};                    // the run-based scan's columns
    uint32_t *bases = nullptr;        // the class lists' bases in cols.list_rank
    uint64_t *tot = nullptr;          // count / mark accumulators, zeroed by the column kernels
    uint64_t *gstat = nullptr;        // tier statistics and batch totals, zeroed by the column kernels
    bool v1 = false;                  // the exact-replay columns are built (kept for a mixed batch's range queries)
    CfkView v1view{};
};

// keydeps.hip
CfkBuild build_cfk(acc_ctx *ctx, const acc_batch_in *in, CfkOpts opts);
void keydeps_of(acc_ctx *ctx, CfkBuild &cb, acc_keydeps_view *view);   // replay on ties, else the run-based path
uint32_t cfk_nseg(acc_ctx *ctx, const CfkBuild &cb);                    // segment count (one small copy and a host sync)
// the snapshot for the scans other than mapReduceActive (recovery.hip): the build with segment keys, and nseg
CfkBuild cfk_snapshot(acc_ctx *ctx, const acc_batch_in *in);
// keydeps_replay.hip
CfkView build_v1_cfk(acc_ctx *ctx, const CfkBuild &cb, bool multi_only = false);
void keydeps_replay(acc_ctx *ctx, CfkBuild &cb, acc_keydeps_view *view);

}  // namespace acc
