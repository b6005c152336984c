// keydeps_replay.hip — the exact replay path of KeyDeps (v1), over a built CFK (CfkBuild, keydeps.hpp).
//
// committed[] per segment sorted by (executeAt rank, txn order) (CommandsForKey ctor, local/CommandsForKey.java:459-469),
// the nearest-Write index, per-segment prefix maxima of committed executeAt and the uncommitted list; then per (T, k)
// query the reference's FAST bisection for maxCommittedBefore (SortedArrays.java:992-1027, replayed on ranks, so ties
// resolve identically) and a scan of [scanStart, insertPos) plus the uncommitted entries before scanStart (the query
// itself is in keydeps.hpp); per-(T, k) lists emitted in order, then the per-T union by binary search and the Java
// keysToTxnIds layout (utils/RelationMultiMap.java:88-260).
//
// Taken when executeAt ties exist (the run-based path of keydeps.hip assumes none) or under ACC_OPT_FORCE_REPLAY, and
// its columns (build_v1_cfk) serve the range-domain queries of keydeps_mixed.hip. It stays independent of the
// run-based path: the tests compare the two.
#include "keydeps.hpp"

namespace acc {

// v1 only: committed / uncommitted flags and the segmented prefix-max input
// multi_seg (non-null): committed[] lists only for segments of two or more entries (the mixed path answers
// single-entry segments without them, k_mx_pcount)
__global__ __launch_bounds__(BLOCK) void k_v1_flags(size_t P, const uint8_t *__restrict__ s_info, const uint32_t *__restrict__ s_exec,
                                                    const uint32_t *__restrict__ seg_incl, const uint32_t *__restrict__ multi_seg,
                                                    uint32_t *__restrict__ cflag, uint32_t *__restrict__ uflag,
                                                    uint64_t *__restrict__ pmax_in)
{
    size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    uint32_t st = s_info[p] & 7u;
    bool c = st >= 4 && st <= 6;
    if (multi_seg) {
        const uint32_t sg = seg_incl[p] - 1;
        cflag[p] = c && multi_seg[sg + 1] - multi_seg[sg] >= 2;
    } else {
        cflag[p] = c;
    }
    uflag[p] = st >= 1 && st <= 3;
    // segmented prefix-max via a segment-id prefix: max over (seg << 32 | exec+1) never crosses segments
    pmax_in[p] = ((uint64_t)(seg_incl[p] - 1) << 32) | (c ? (uint64_t)s_exec[p] + 1 : 0);
}

__global__ __launch_bounds__(BLOCK) void k_low32(size_t P, const uint64_t *__restrict__ in, uint32_t *__restrict__ out)
{
    size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p < P) out[p] = (uint32_t)in[p];
}
__global__ __launch_bounds__(BLOCK) void k_low32x2(size_t P, const uint64_t *__restrict__ a, uint32_t *__restrict__ a32,
                                                   const uint64_t *__restrict__ b, uint32_t *__restrict__ b32)
{
    size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p < P) { a32[p] = (uint32_t)a[p]; b32[p] = (uint32_t)b[p]; }
}

// Committed entries -> (seg << ebits | execRank) composite for the stable (seg, executeAt) sort; pads
// (all ones in `bits`) fill [NC, P) so the sort runs on the host-known size P.
__global__ __launch_bounds__(BLOCK) void k_committed_keys(size_t P, const uint32_t *__restrict__ cflag, const uint32_t *__restrict__ cum_c,
                                                          const uint32_t *__restrict__ seg_incl, const uint32_t *__restrict__ s_exec,
                                                          const uint32_t *__restrict__ uflag, const uint32_t *__restrict__ cum_u,
                                                          int ebits, int bits, uint64_t *__restrict__ ckey,
                                                          uint32_t *__restrict__ cpos, uint32_t *__restrict__ u_pos, int pads)
{
    size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    uint32_t nc = cum_c[P];
    if (cflag[p]) {
        uint32_t c = cum_c[p];
        ckey[c] = ((uint64_t)(seg_incl[p] - 1) << ebits) | s_exec[p];
        cpos[c] = (uint32_t)p;
    }
    if (pads && p >= nc) {
        ckey[p] = bits >= 64 ? ~0ull : ((1ull << bits) - 1);
        cpos[p] = 0xFFFFFFFFu;
    }
    if (uflag[p]) u_pos[cum_u[p]] = (uint32_t)p;
}

// cl_exec / lastWrite input / cl_start per segment.
__global__ __launch_bounds__(BLOCK) void k_committed_cols(size_t P, const uint32_t *__restrict__ cpos_sorted,
                                                          const uint32_t *__restrict__ s_exec, const uint8_t *__restrict__ s_info,
                                                          const uint32_t *__restrict__ cum_c, uint32_t *__restrict__ cl_exec,
                                                          uint32_t *__restrict__ lastw_in)
{
    size_t c = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (c >= P) return;
    uint32_t nc = cum_c[P];
    if (c >= nc) { lastw_in[c] = 0; return; }
    uint32_t p = cpos_sorted[c];
    cl_exec[c] = s_exec[p];
    // committed[i].kind().isWrite(): kind of the TxnId (CommandsForKey.java:623)
    lastw_in[c] = ((s_info[p] >> 3) == 1) ? (uint32_t)c + 1 : 0;
}

__global__ __launch_bounds__(BLOCK) void k_seg_committed_start(size_t P, const uint32_t *__restrict__ seg_incl,
                                                               const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ cum_c,
                                                               uint32_t *__restrict__ cl_start)
{
    size_t s = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t nseg = seg_incl[P - 1];
    if (s > nseg) return;
    cl_start[s] = s == nseg ? cum_c[P] : cum_c[seg_start[s]];
}

__global__ __launch_bounds__(BLOCK) void k_query_count(size_t P, CfkView v, uint64_t *__restrict__ cnt)
{
    size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= P) return;
    Query q = make_query(v, (uint32_t)j);
    cnt[j] = run_query<false>(v, q, nullptr);
}

__global__ __launch_bounds__(BLOCK) void k_query_emit(size_t P, CfkView v, const uint64_t *__restrict__ dep_off,
                                                      uint32_t *__restrict__ deps, uint32_t *__restrict__ list_of)
{
    size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= P) return;
    Query q = make_query(v, (uint32_t)j);
    uint64_t o = dep_off[j];
    uint32_t c = run_query<true>(v, q, deps + o);
    for (uint32_t k = 0; k < c; ++k) list_of[o + k] = (uint32_t)j;
}

// ---------------------------------------------------------------- KeyDeps assembly

__device__ __forceinline__ bool contains_u32(const uint32_t *a, uint64_t lo, uint64_t hi, uint32_t v)
{
    while (lo < hi) {
        uint64_t mid = (lo + hi) >> 1;
        uint32_t x = a[mid];
        if (x < v) lo = mid + 1;
        else if (x > v) hi = mid;
        else return true;
    }
    return false;
}

// first[e] = dep is not in an earlier key's list of the same txn (the union keeps one copy).
__global__ __launch_bounds__(BLOCK) void k_first(uint64_t E, const uint32_t *__restrict__ deps, const uint32_t *__restrict__ list_of,
                                                 const uint32_t *__restrict__ owner, const uint32_t *__restrict__ key_off,
                                                 const uint64_t *__restrict__ dep_off, uint32_t *__restrict__ first)
{
    uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= E) return;
    uint32_t j = list_of[e];
    uint32_t t = owner[j];
    uint32_t d = deps[e];
    uint32_t f = 1;
    for (uint32_t jj = key_off[t]; jj < j; ++jj)
        if (contains_u32(deps, dep_off[jj], dep_off[jj + 1], d)) { f = 0; break; }
    first[e] = f;
}

__global__ __launch_bounds__(BLOCK) void k_nonempty(size_t P, const uint64_t *__restrict__ cnt, uint32_t *__restrict__ nz)
{
    size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < P) nz[j] = cnt[j] != 0;
}

__global__ __launch_bounds__(BLOCK) void k_txn_sizes(uint32_t n, const uint32_t *__restrict__ key_off, const uint64_t *__restrict__ dep_off,
                                                     const uint32_t *__restrict__ cnz, const uint32_t *__restrict__ cumf,
                                                     uint64_t *__restrict__ kd_cnt, uint64_t *__restrict__ u_cnt,
                                                     uint64_t *__restrict__ a_cnt)
{
    uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n) return;
    uint32_t j0 = key_off[t], j1 = key_off[t + 1];
    uint64_t e0 = dep_off[j0], e1 = dep_off[j1];
    uint64_t kd = cnz[j1] - cnz[j0];
    kd_cnt[t] = kd;
    u_cnt[t] = cumf[e1] - cumf[e0];
    a_cnt[t] = kd + (e1 - e0);
}

// arena indices (KeyDeps.keysToTxnIds value part) and KeyDeps.txnIds (as batch indices)
__global__ __launch_bounds__(BLOCK) void k_write_entries(uint64_t E, const uint32_t *__restrict__ deps, const uint32_t *__restrict__ list_of,
                                                         const uint32_t *__restrict__ owner, const uint32_t *__restrict__ key_off,
                                                         const uint64_t *__restrict__ dep_off, const uint32_t *__restrict__ cumf,
                                                         const uint32_t *__restrict__ first, const uint32_t *__restrict__ cnz,
                                                         const uint64_t *__restrict__ arena_off, const uint64_t *__restrict__ u_off,
                                                         const uint32_t *__restrict__ txn_of_rank, int32_t *__restrict__ arena,
                                                         uint32_t *__restrict__ dep_txn)
{
    uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= E) return;
    uint32_t j = list_of[e];
    uint32_t t = owner[j];
    uint32_t d = deps[e];
    uint32_t j0 = key_off[t], j1 = key_off[t + 1];
    // index of d in the sorted union = number of distinct deps of T smaller than d
    uint32_t idx = 0;
    for (uint32_t jj = j0; jj < j1; ++jj) {
        uint64_t a = dep_off[jj], b = dep_off[jj + 1];
        if (a == b) continue;
        uint64_t lb = jj == j ? e : lower_bound(deps, a, b, d);
        idx += cumf[lb] - cumf[a];
    }
    uint32_t kd = cnz[j1] - cnz[j0];
    uint64_t base = dep_off[j0];
    arena[arena_off[t] + kd + (e - base)] = (int32_t)idx;
    if (first[e]) dep_txn[u_off[t] + idx] = txn_of_rank[d];
}

// per non-empty (T,k): KeyDeps.keys entry and the end-offset header int (KeyDeps.java:150-172)
__global__ __launch_bounds__(BLOCK) void k_write_keys(size_t P, const uint64_t *__restrict__ cnt, const uint32_t *__restrict__ owner,
                                                      const uint32_t *__restrict__ key_off, const uint64_t *__restrict__ dep_off,
                                                      const uint32_t *__restrict__ cnz, const uint64_t *__restrict__ kd_off,
                                                      const uint64_t *__restrict__ arena_off, uint32_t *__restrict__ key_idx,
                                                      int32_t *__restrict__ arena)
{
    size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= P || cnt[j] == 0) return;
    uint32_t t = owner[j];
    uint32_t j0 = key_off[t], j1 = key_off[t + 1];
    uint32_t slot = cnz[j] - cnz[j0];
    uint32_t kd = cnz[j1] - cnz[j0];
    key_idx[kd_off[t] + slot] = (uint32_t)j - j0;
    arena[arena_off[t] + slot] = (int32_t)(kd + (dep_off[j + 1] - dep_off[j0]));
}

// Exact-replay CFK columns: uncommitted/committed flags and counts, segmented executeAt prefix max, committed[] per
// segment sorted by executeAt (CommandsForKey.java:462-469) with the nearest-Write scan
// multi_only: committed[] lists of the segments with two or more entries only, sorted at their exact size (one host
// sync): the mixed path's single-entry segments never read them
CfkView build_v1_cfk(acc_ctx *ctx, const CfkBuild &cb, bool multi_only)
{
    const size_t P = cb.P;
    const int rbits = cb.dict.rbits;
    const uint32_t *seg_incl = cb.seg_incl, *seg_start = cb.seg_start, *s_exec = cb.s_exec;
    const uint8_t *s_info = cb.s_info;
    const unsigned gP = grid_for(P, BLOCK);
    uint32_t *cflag = ctx->get<uint32_t>("cflag", P);
    uint32_t *uflag = ctx->get<uint32_t>("uflag", P);
    uint64_t *pmax_in = ctx->get<uint64_t>("pmax_in", P);
    launch(ctx, "v1_flags", k_v1_flags, dim3(gP), dim3(BLOCK), 0, P, s_info, s_exec, seg_incl,
           multi_only ? seg_start : (const uint32_t *)nullptr, cflag, uflag, pmax_in);
    uint32_t *cum_c = ctx->get<uint32_t>("cum_c", P + 1);
    uint32_t *cum_u = ctx->get<uint32_t>("cum_u", P + 1);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, cflag, cum_c, P, true, cum_c + P);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, uflag, cum_u, P, true, cum_u + P);
    uint64_t *pmax64 = ctx->get<uint64_t>("pmax64", P);
    scan<uint64_t, OpMax<uint64_t>>(ctx, pmax_in, pmax64, P, false);
    uint32_t *pmax = ctx->get<uint32_t>("pmax", P);
    launch(ctx, "low32", k_low32, dim3(gP), dim3(BLOCK), 0, P, (const uint64_t *)pmax64, pmax);

    // committed[] per segment: stable sort of (segment, executeAt rank)
    const int segbits = bits_for(P);
    const int cbits = segbits + rbits;
    if (cbits > 64) fail(ACC_E_ARG, "batch too large for the committed-list composite key");
    uint64_t *ckey = ctx->get<uint64_t>("ckey", P);
    uint32_t *cpos = ctx->get<uint32_t>("cpos", P);
    uint32_t *u_pos = ctx->get<uint32_t>("u_pos", P);
    launch(ctx, "committed_keys", k_committed_keys, dim3(gP), dim3(BLOCK), 0, P, (const uint32_t *)cflag,
           (const uint32_t *)cum_c, (const uint32_t *)seg_incl, (const uint32_t *)s_exec, (const uint32_t *)uflag,
           (const uint32_t *)cum_u, rbits, cbits, ckey, cpos, u_pos, multi_only ? 0 : 1);
    size_t NC = P;
    if (multi_only) {
        ACC_HIP(hipMemcpyAsync(ctx->pinned, cum_c + P, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        NC = (size_t)(ctx->pinned[0] & 0xFFFFFFFFu);
        ctx->stat("keydeps.v1_committed_sorted", NC);
    }
    Sorted cs = radix_sort(ctx, "rs_cl", ckey, cpos, NC, cbits);
    uint32_t *cl_exec = ctx->get<uint32_t>("cl_exec", P);
    uint32_t *lastw_in = ctx->get<uint32_t>("lastw_in", P);
    uint32_t *lastw = ctx->get<uint32_t>("lastw", P);
    launch(ctx, "committed_cols", k_committed_cols, dim3(gP), dim3(BLOCK), 0, P, (const uint32_t *)cs.vals,
           (const uint32_t *)s_exec, (const uint8_t *)s_info, (const uint32_t *)cum_c, cl_exec, lastw_in);
    scan<uint32_t, OpMax<uint32_t>>(ctx, lastw_in, lastw, P, false);
    uint32_t *cl_start = ctx->get<uint32_t>("cl_start", P + 1);
    launch(ctx, "seg_committed_start", k_seg_committed_start, dim3(grid_for(P + 1, BLOCK)), dim3(BLOCK), 0, P,
           (const uint32_t *)seg_incl, (const uint32_t *)seg_start, (const uint32_t *)cum_c, cl_start);
    CfkView v;
    v.seg_start = seg_start; v.s_rank = cb.s_rank; v.s_exec = s_exec; v.seg_incl = seg_incl; v.pair_pos = cb.pair_pos;
    v.owner = cb.owner; v.rank = cb.dict.rank; v.s_info = s_info; v.cl_start = cl_start; v.cl_exec = cl_exec; v.lastw = lastw;
    v.pmax = pmax; v.cum_u = cum_u; v.u_pos = u_pos; v.tl = cb.tl; v.n = cb.n; v.vseg = nullptr;
    return v;
}

// KeyDeps of a built batch by the exact replay: count -> exclusive scan -> emit over every (T, k) query, then the
// per-T union of the per-key lists by binary search and the Java keysToTxnIds layout. The caller has filled
// cb.pair_pos. The replay columns stay on the record (a mixed batch's range queries reuse them).
void keydeps_replay(acc_ctx *ctx, CfkBuild &cb, acc_keydeps_view *view)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = cb.n;
    const size_t P = cb.P;
    const uint32_t *key_off = cb.key_off, *owner = cb.owner, *txn_of_rank = cb.dict.txn_of_rank;
    const uint64_t *g = cb.g;
    const unsigned gP = grid_for(P, BLOCK);
    // ---- conflict scan: count, scan, emit
    CfkView v = build_v1_cfk(ctx, cb);
    cb.v1 = true;
    cb.v1view = v;
    uint64_t *cnt = ctx->get<uint64_t>("cnt", P);
    uint64_t *dep_off = ctx->get<uint64_t>("dep_off", P + 1);
    launch(ctx, "query_count", k_query_count, dim3(gP), dim3(BLOCK), 0, P, v, cnt);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, cnt, dep_off, P, true, dep_off + P);
    ACC_HIP(hipMemcpyAsync(ctx->pinned, dep_off + P, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ACC_HIP(hipMemcpyAsync(ctx->pinned + 1, g + 4, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ctx->sync();
    const uint64_t E = ctx->pinned[0];
    check_errors(ctx->pinned[1]);
    if (E >= 0xFFFFFFFFull) fail(ACC_E_CAP, "more than 2^32-1 dependency entries in one batch");

    uint32_t *deps = ctx->get<uint32_t>("deps", E);
    uint32_t *list_of = ctx->get<uint32_t>("list_of", E);
    launch(ctx, "query_emit", k_query_emit, dim3(gP), dim3(BLOCK), 0, P, v, (const uint64_t *)dep_off, deps, list_of);

    // ---- KeyDeps assembly
    const unsigned gE = grid_for(E, BLOCK);
    uint32_t *first = ctx->get<uint32_t>("first", E);
    uint32_t *cumf = ctx->get<uint32_t>("cumf", E + 1);
    launch(ctx, "first", k_first, dim3(gE), dim3(BLOCK), 0, E, (const uint32_t *)deps, (const uint32_t *)list_of,
           (const uint32_t *)owner, key_off, (const uint64_t *)dep_off, first);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, first, cumf, E, true, cumf + E);
    uint32_t *nz = ctx->get<uint32_t>("nz", P);
    uint32_t *cnz = ctx->get<uint32_t>("cnz", P + 1);
    launch(ctx, "nonempty", k_nonempty, dim3(gP), dim3(BLOCK), 0, P, (const uint64_t *)cnt, nz);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, nz, cnz, P, true, cnz + P);
    uint64_t *kd_cnt = ctx->get<uint64_t>("kd_cnt", n);
    uint64_t *u_cnt = ctx->get<uint64_t>("u_cnt", n);
    uint64_t *a_cnt = ctx->get<uint64_t>("a_cnt", n);
    launch(ctx, "txn_sizes", k_txn_sizes, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, key_off, (const uint64_t *)dep_off,
           (const uint32_t *)cnz, (const uint32_t *)cumf, kd_cnt, u_cnt, a_cnt);
    uint64_t *kd_off = ctx->get<uint64_t>("kd_off", (size_t)n + 1);
    uint64_t *u_off = ctx->get<uint64_t>("u_off", (size_t)n + 1);
    uint64_t *arena_off = ctx->get<uint64_t>("arena_off", (size_t)n + 1);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, kd_cnt, kd_off, n, true, kd_off + n);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, u_cnt, u_off, n, true, u_off + n);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, a_cnt, arena_off, n, true, arena_off + n);
    // upper bounds: ΣKd <= P, ΣU <= E, Σ(Kd+E) <= P + E
    int32_t *arena = ctx->get<int32_t>("arena", P + E);
    uint32_t *key_idx = ctx->get<uint32_t>("key_idx", P);
    uint32_t *dep_txn = ctx->get<uint32_t>("dep_txn", E);
    launch(ctx, "write_entries", k_write_entries, dim3(gE), dim3(BLOCK), 0, E, (const uint32_t *)deps,
           (const uint32_t *)list_of, (const uint32_t *)owner, key_off, (const uint64_t *)dep_off, (const uint32_t *)cumf,
           (const uint32_t *)first, (const uint32_t *)cnz, (const uint64_t *)arena_off, (const uint64_t *)u_off,
           (const uint32_t *)txn_of_rank, arena, dep_txn);
    launch(ctx, "write_keys", k_write_keys, dim3(gP), dim3(BLOCK), 0, P, (const uint64_t *)cnt, (const uint32_t *)owner,
           key_off, (const uint64_t *)dep_off, (const uint32_t *)cnz, (const uint64_t *)kd_off,
           (const uint64_t *)arena_off, key_idx, arena);
    ACC_HIP(hipMemcpyAsync(ctx->pinned, arena_off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ACC_HIP(hipMemcpyAsync(ctx->pinned + 1, kd_off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ACC_HIP(hipMemcpyAsync(ctx->pinned + 2, u_off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ctx->sync();
    *view = acc_keydeps_view{ n, ctx->pinned[0], ctx->pinned[1], ctx->pinned[2], E, arena_off, arena, kd_off,
                              key_idx, u_off, dep_txn };
    ctx->kd_view = *view;
    ctx->kd_valid = true;
}

}  // namespace acc
