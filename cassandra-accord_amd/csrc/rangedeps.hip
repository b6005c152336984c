// rangedeps.hip — RangeDeps of a mixed key/range batch on CDNA4 (SURVEY.md §8 rows A4, A8 range part, A18).
//
// For every txn T of one CommandStore snapshot, the range-command part of
// InMemorySafeStore.mapReduceActive (impl/InMemoryCommandStore.java:863-870 -> mapReduceRangesInternal :883-1016)
// under PreAccept.calculatePartialDeps (messages/PreAccept.java:245-265):
//   every range command C (range-domain txn, status not erased: INVALID_OR_TRUNCATED here) with
//   C.txnId < T.executeAt (STARTED_BEFORE), T.kind().witnesses(C.kind), C != p1, contributes (r, C) for each
//   of its ranges r that intersects T's keys (Range.contains) or T's ranges (start < that.end && end > that.start);
//   the TreeMap<Range, List> (Range::compare) then RangeDeps.Builder (utils/RelationMultiMap.java:88-260) give the
//   Java layout: ranges sorted unique, txnIds sorted unique, rangesToTxnIds = end-offset header + indices.
//
// Pipeline (one HIP stream):
//   1. prep + dictionary (shared with keydeps.hip): validation, dense order ranks of every TxnId/executeAt.
//   2. range-command entries: the ranges of non-erased range txns; stored-range dictionary (distinct (start, end)
//      in Range::compare order -> range id); entries re-sorted by (width class, start) where class c holds widths
//      in (4^(c-1), 4^c]: a range of class c containing / intersecting a query [lo, hi] starts in [lo - 4^c, hi].
//   3. stabbing: every query (a key of a key txn, or a range of a range txn) sorted by its low bound; a workgroup
//      of 256 consecutive queries streams, per class, the entries starting in its window through LDS (coalesced
//      tiles shared by the 256 queries) and tests each against its own query: count -> scan -> emit of
//      (range id << 32 | TxnId rank) per query, contiguous per txn.
//   4. build: per txn, sort (range id, TxnId rank) = TreeMap order, dedupe, TxnId union + index: one wave per txn
//      (<= 64 raw entries, register bitonic), one workgroup per txn (<= 8192, LDS bitonic), one workgroup on a
//      global scratch region beyond that. Two passes: sizes, then the Java-layout writes.
// Integer work only: HBM/latency bound, no MFMA.
//
// One stage per step over one record (RdBuild, rangedeps.hpp): rd_prepare and rd_range_dict here (1, 2),
// rd_stab_queries in rangedeps_stab.hip (3), rd_build_txns in rangedeps_build.hip (4); a kernel lives in the file of
// the stage that launches it.

#include "rangedeps.hpp"

namespace acc {

namespace rd {

enum : uint64_t {
    ERR_DOMAIN = 1u << 8,
    ERR_RANGE_EMPTY = 1u << 9,
    ERR_RANGES_UNSORTED = 1u << 10,
    ERR_RNG_OFF = 1u << 11,
};

// ---------------------------------------------------------------- prep

// Per txn: domain consistency (TxnId.domain(), primitives/TxnId.java:134-157), Range start < end (Range.java ctor)
// and Ranges.ofSortedAndDeoverlapped (AbstractRanges.java:789-796); range owners; entry flags (non-erased range
// commands); OR-masks of the range bounds and the query low bounds (bit compaction plans).
// g: [0] start mask, [1] end mask, [2] query-lo mask (all relative to ref[]), [3] errors, [4] non-empty ranges.
__global__ __launch_bounds__(BLOCK) void k_rd_prep(uint32_t n, const uint64_t *__restrict__ tl, const uint8_t *__restrict__ status,
                                                   const uint32_t *__restrict__ key_off, const uint64_t *__restrict__ key_code,
                                                   const uint32_t *__restrict__ rng_off, const uint64_t *__restrict__ rs,
                                                   const uint64_t *__restrict__ re, uint64_t ref_s, uint64_t ref_e,
                                                   uint64_t ref_lo, uint32_t *__restrict__ rowner,
                                                   uint32_t *__restrict__ eflag, uint64_t *__restrict__ g)
{
    uint64_t ms = 0, me = 0, ml = 0, errs = 0;
    // RD_TS chunks of BLOCK txns per workgroup: one OR per word and workgroup into g (its 4 words share one line)
    for (int r = 0; r < RD_TS; ++r) {
    const uint32_t t = (blockIdx.x * RD_TS + (uint32_t)r) * BLOCK + threadIdx.x;
    if (t < n) {
        const bool isr = (tl[t] & 1u) != 0;
        const uint32_t k0 = key_off[t], k1 = key_off[t + 1];
        const uint32_t r0 = rng_off[t], r1 = rng_off[t + 1];
        if (r1 < r0) errs |= ERR_RNG_OFF;
        else {
            if (isr && k1 != k0) errs |= ERR_DOMAIN;
            if (!isr && r1 != r0) errs |= ERR_DOMAIN;
            const uint32_t live = status[t] != 7;
            for (uint32_t j = r0; j < r1; ++j) {
                const uint64_t s = rs[j], e = re[j];
                if (s >= e) errs |= ERR_RANGE_EMPTY;
                if (j > r0 && re[j - 1] > s) errs |= ERR_RANGES_UNSORTED;
                rowner[j] = t;
                eflag[j] = live;
                ms |= s ^ ref_s;
                me |= e ^ ref_e;
                ml |= s ^ ref_lo;
            }
        }
        if (k1 >= k0)
            for (uint32_t jb = k0; jb < k1; jb += 8) {   // eight key loads in flight
                uint64_t kc[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) kc[u] = jb + u < k1 ? key_code[jb + u] ^ ref_lo : 0ull;
#pragma unroll
                for (int u = 0; u < 8; ++u) ml |= kc[u];
            }
    }
    }
    __shared__ uint64_t part[WAVES][4];
    uint64_t v[4] = { ms, me, ml, errs };
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        uint64_t x = v[w];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x |= shfl_xor(x, d);
        if (lane_id() == 0) part[threadIdx.x >> 6][w] = x;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint64_t x = 0;
#pragma unroll
        for (int q = 0; q < WAVES; ++q) x |= part[q][threadIdx.x];
        if (x) atomicOr((unsigned long long *)&g[threadIdx.x], (unsigned long long)x);
    }
}

// compacted entry columns (input order) + the (start, end) dictionary sort key
__global__ __launch_bounds__(BLOCK) void k_rd_entries(uint32_t R, uint32_t n, const uint32_t *__restrict__ eflag,
                                                      const uint32_t *__restrict__ eidx, const uint32_t *__restrict__ rowner,
                                                      const uint64_t *__restrict__ rs, const uint64_t *__restrict__ re,
                                                      const uint4 *__restrict__ tinfo, const uint64_t *__restrict__ tl,
                                                      Runs rs_plan, Runs re_plan, int e_bits, int split, uint4 *__restrict__ erec,
                                                      uint64_t *__restrict__ dkey, uint64_t *__restrict__ ekey)
{
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= R || !eflag[j]) return;
    const uint32_t i = eidx[j], t = rowner[j];
    const uint64_t s = rs[j], e = re[j];
    // the entry's 32-B record: start, end | TxnId position, kind, range id (k_rd_dict_write) — the permuted reads of
    // the dictionary and class passes take one record per entry instead of a line per column
    erec[2 * (size_t)i] = make_uint4((uint32_t)s, (uint32_t)(s >> 32), (uint32_t)e, (uint32_t)(e >> 32));
    erec[2 * (size_t)i + 1] = make_uint4(tinfo[t].y, (uint32_t)((tl[t] >> 1) & 7u), 0u, 0u);
    const uint64_t sc = pext_runs(s, rs_plan), ec = pext_runs(e, re_plan);
    if (split) { dkey[i] = sc; ekey[i] = ec; }      // two-key LSD: end first, then start (stable)
    else dkey[i] = (sc << e_bits) | ec;
}

// rid per (start, end)-sorted position; dictionary arrays
__global__ __launch_bounds__(BLOCK) void k_rd_dict_flags(uint32_t ne, const uint32_t *__restrict__ perm,
                                                         const uint4 *__restrict__ erec, uint32_t *__restrict__ flag)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= ne) return;
    uint32_t f = 1;
    if (p > 0) {
        const uint4 a = erec[2 * (size_t)perm[p]], b = erec[2 * (size_t)perm[p - 1]];
        f = a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w;
    }
    flag[p] = f;
}

__global__ __launch_bounds__(BLOCK) void k_rd_dict_write(uint32_t ne, const uint32_t *__restrict__ perm,
                                                         const uint32_t *__restrict__ flag, const uint32_t *__restrict__ incl,
                                                         uint4 *__restrict__ erec, uint64_t *__restrict__ dict_s,
                                                         uint64_t *__restrict__ dict_e, uint64_t *__restrict__ ckey,
                                                         uint32_t *__restrict__ cls_hist)
{
    __shared__ uint32_t h[NCLS];
    if (threadIdx.x < NCLS) h[threadIdx.x] = 0;
    __syncthreads();
    // RD_TS chunks of BLOCK entries per workgroup: one global add per class and workgroup (the 33 counters share two lines)
    for (int r = 0; r < RD_TS; ++r) {
    const uint32_t p = (blockIdx.x * RD_TS + (uint32_t)r) * BLOCK + threadIdx.x;
    uint32_t c = 0xFFu;
    if (p < ne) {
        const uint32_t i = perm[p], rid = incl[p] - 1;
        const uint4 a = erec[2 * (size_t)i];
        const uint64_t es = ((uint64_t)a.y << 32) | a.x, ee = ((uint64_t)a.w << 32) | a.z;
        reinterpret_cast<uint32_t *>(erec + 2 * (size_t)i + 1)[2] = rid;   // the entry's range id
        if (flag[p]) { dict_s[rid] = es; dict_e[rid] = ee; }
        c = width_class(es, ee);
        ckey[p] = c;   // in (start, end) order: one stable pass by class gives the (class, start) order
    }
    // LDS histogram, one add per distinct class of a wave (per-thread atomics on a few hot words serialise); one global
    // atomic per class and block
    {
        const uint32_t lane = lane_id();
        uint64_t rem = __ballot(c != 0xFFu);
        while (rem) {
            const uint32_t leader = (uint32_t)__builtin_ctzll(rem);
            const uint32_t c0 = (uint32_t)__shfl((int)c, (int)leader, 64);
            const uint64_t m = __ballot(c == c0) & rem;
            if (lane == leader) atomicAdd(&h[c0], (uint32_t)__popcll(m));
            rem &= ~m;
        }
    }
    }
    __syncthreads();
    if (threadIdx.x < NCLS && h[threadIdx.x]) atomicAdd(&cls_hist[threadIdx.x], h[threadIdx.x]);
}

__global__ void k_rd_class_off(const uint32_t *__restrict__ hist, uint32_t *__restrict__ off)
{
    if (threadIdx.x != 0) return;
    uint32_t a = 0;
    for (int c = 0; c < NCLS; ++c) { off[c] = a; a += hist[c]; }
    off[NCLS] = a;
}

// class-sorted entry columns
__global__ __launch_bounds__(BLOCK) void k_rd_class_cols(uint32_t ne, const uint32_t *__restrict__ perm,
                                                         const uint4 *__restrict__ erec, uint64_t *__restrict__ cs_s,
                                                         uint64_t *__restrict__ cs_e, uint2 *__restrict__ cs_info,
                                                         uint8_t *__restrict__ cs_kind)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= ne) return;
    const uint32_t i = perm[p];
    const uint4 a = erec[2 * (size_t)i], b = erec[2 * (size_t)i + 1];
    cs_s[p] = ((uint64_t)a.y << 32) | a.x;
    cs_e[p] = ((uint64_t)a.w << 32) | a.z;
    cs_info[p] = make_uint2(b.z, b.x);   // (range id, TxnId position)
    cs_kind[p] = (uint8_t)b.y;
}

// ---------------------------------------------------------------- txn columns

// isT[r] = 1 where r is the rank of a TxnId (the dictionary ranks every TxnId and executeAt of the batch)
__global__ __launch_bounds__(BLOCK) void k_rd_txnflag(uint32_t n, const uint32_t *__restrict__ rank, uint32_t *__restrict__ isT)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < n) isT[rank[t]] = 1;
}

// Per txn {lim, tpos, witness mask, is range}: tpos = position of its TxnId among the batch's TxnIds (TxnId order),
// lim = number of TxnIds below its executeAt, so C.txnId < T.executeAt <=> tpos(C) < lim(T) (STARTED_BEFORE,
// InMemoryCommandStore.java:897-898). txn_of_tpos inverts tpos (identity for a batch given in TxnId order).
__global__ __launch_bounds__(BLOCK) void k_rd_txncols(uint32_t n, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ tcnt,
                                                      const uint64_t *__restrict__ tl, uint4 *__restrict__ tinfo,
                                                      uint32_t *__restrict__ txn_of_tpos)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n) return;
    const uint32_t tpos = tcnt[rank[t]], lim = tcnt[rank[n + t]];
    tinfo[t] = make_uint4(lim, tpos, witnesses((uint32_t)(tl[t] >> 1) & 7u), (uint32_t)(tl[t] & 1u));
    txn_of_tpos[tpos] = t;
}

}  // namespace rd

using namespace rd;

static void rd_check_errors(uint64_t errs)
{
    if (errs & ERR_DOMAIN) fail(ACC_E_ARG, "a range-domain txn lists keys or a key-domain txn lists ranges (TxnId.domain())");
    if (errs & ERR_RANGE_EMPTY) fail(ACC_E_ARG, "range start must be below its end (Range: start >= end)");
    if (errs & ERR_RANGES_UNSORTED) fail(ACC_E_ARG, "ranges of a txn must be sorted and deoverlapped (Ranges.ofSortedAndDeoverlapped)");
    if (errs & ERR_RNG_OFF) fail(ACC_E_ARG, "rng_off must be non-decreasing");
}

// ---- 1. staged inputs, prep + dictionary (also validates keys, statuses, kinds, TxnId order and uniqueness), TxnId
// positions, the range owners and entry flags, the bound masks
void rd_prepare(acc_ctx *ctx, const acc_range_batch_in *in, const SharedDict *shared, RdBuild &b)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = b.n;
    const size_t P = b.P, R = b.R;
    b.key_off = stage_in(ctx, "in_key_off", in->key_off, (size_t)n + 1, in->mem);
    b.rng_off = stage_in(ctx, "in_rng_off", in->rng_off, (size_t)n + 1, in->mem);
    b.tm = stage_in(ctx, "in_tm", in->txn_id.msb, n, in->mem);
    b.tl = stage_in(ctx, "in_tl", in->txn_id.lsb, n, in->mem);
    b.tn = stage_in(ctx, "in_tn", in->txn_id.node, n, in->mem);
    b.em = stage_in(ctx, "in_em", in->execute_at.msb, n, in->mem);
    b.el = stage_in(ctx, "in_el", in->execute_at.lsb, n, in->mem);
    b.en = stage_in(ctx, "in_en", in->execute_at.node, n, in->mem);
    b.status = stage_in(ctx, "in_status", in->status, n, in->mem);
    b.key_code = stage_in(ctx, "in_key_code", in->key_code, P, in->mem);
    b.rs = stage_in(ctx, "in_rng_start", in->rng_start, R, in->mem);
    b.re = stage_in(ctx, "in_rng_end", in->rng_end, R, in->mem);

    // (acc_partial_deps_batch: the KeyDeps half already built the dictionary over the same batch)
    if (shared && shared->valid) {
        b.dict = shared->dict;
        b.owner = shared->owner;
        ctx->stat("rangedeps.shared_dictionary", 1);
    } else {
        uint64_t *g = ctx->get<uint64_t>("g", PREP_G_WORDS);
        uint32_t *own = ctx->get<uint32_t>("owner", P);
        prep_dictionary(ctx, n, P, b.tm, b.tl, b.tn, b.em, b.el, b.en, b.status, b.key_off, b.key_code, own, g, b.dict);
        b.owner = own;
        ctx->stat("rangedeps.shared_dictionary", 0);
    }
    // TxnId positions and STARTED_BEFORE limits
    const size_t m2 = 2 * (size_t)n;
    uint32_t *isT = ctx->get<uint32_t>("rd_isT", m2);
    uint32_t *tcnt = ctx->get<uint32_t>("rd_tcnt", m2 + 1);
    ACC_HIP(hipMemsetAsync(isT, 0, m2 * sizeof(uint32_t), st));
    launch(ctx, "rd_txnflag", k_rd_txnflag, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, (const uint32_t *)b.dict.rank, isT);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, isT, tcnt, m2, true, tcnt + m2);
    b.tinfo = ctx->get<uint4>("rd_tinfo", n);
    b.txn_of_tpos = ctx->get<uint32_t>("rd_txn_of_tpos", n);
    launch(ctx, "rd_txncols", k_rd_txncols, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, (const uint32_t *)b.dict.rank,
           (const uint32_t *)tcnt, b.tl, b.tinfo, b.txn_of_tpos);

    // reference codes for the masks (first range bound / first query bound)
    uint64_t ref_s = 0, ref_e = 0, ref_lo = 0;
    {
        ReadBack rb(ctx);
        const auto last_r = rb.u32(b.rng_off + n);
        ReadBack::Word<uint64_t> s0, e0, k0;
        if (R) { s0 = rb.u64(b.rs); e0 = rb.u64(b.re); }
        if (P) k0 = rb.u64(b.key_code);
        rb.wait();
        if ((uint32_t)last_r != R) fail(ACC_E_ARG, "rng_off[n_txn] must equal n_ranges");
        ref_s = s0; ref_e = e0;
        ref_lo = P ? (uint64_t)k0 : ref_s;
    }
    uint64_t *rg = ctx->get<uint64_t>("rd_g", 8);
    ACC_HIP(hipMemsetAsync(rg, 0, 8 * sizeof(uint64_t), st));
    b.rowner = ctx->get<uint32_t>("rd_rowner", R);
    b.eflag = ctx->get<uint32_t>("rd_eflag", R);
    b.eidx = ctx->get<uint32_t>("rd_eidx", R + 1);
    launch(ctx, "rd_prep", k_rd_prep, dim3(grid_for(n, (size_t)BLOCK * RD_TS)), dim3(BLOCK), 0, n, b.tl, b.status, b.key_off,
           b.key_code, b.rng_off, b.rs, b.re, ref_s, ref_e, ref_lo, b.rowner, b.eflag, rg);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, b.eflag, b.eidx, R, true, b.eidx + R);
    ReadBack rb(ctx);
    const auto hm = rb.words((const uint64_t *)rg, 4);   // start, end, query-lo masks; errors
    ReadBack::Word<uint32_t> ne;
    if (R) ne = rb.u32(b.eidx + R);
    rb.wait();
    rd_check_errors(hm[3]);
    b.mask_s = hm[0]; b.mask_e = hm[1]; b.mask_lo = hm[2];
    b.NE = ne;
}

// ---- 2. range-command entries, stored-range dictionary, class order
void rd_range_dict(acc_ctx *ctx, RdBuild &b)
{
    hipStream_t st = ctx->stream;
    const uint32_t NE = b.NE;
    const Runs rs_plan = make_runs(b.mask_s), re_plan = make_runs(b.mask_e);
    uint4 *erec = ctx->get<uint4>("rd_erec", 2 * (size_t)NE);
    uint64_t *dkey = ctx->get<uint64_t>("rd_dkey", NE), *ekey = ctx->get<uint64_t>("rd_ekey", NE);
    const bool split = rs_plan.bits + re_plan.bits > 64;
    ctx->stat("rangedeps.dict_bits", (uint64_t)(rs_plan.bits + re_plan.bits));
    ctx->stat("rangedeps.dict_split", split ? 1 : 0);
    launch(ctx, "rd_entries", k_rd_entries, dim3(grid_for(b.R, BLOCK)), dim3(BLOCK), 0, (uint32_t)b.R, b.n, (const uint32_t *)b.eflag,
           (const uint32_t *)b.eidx, (const uint32_t *)b.rowner, b.rs, b.re, (const uint4 *)b.tinfo, b.tl, rs_plan, re_plan,
           re_plan.bits, split ? 1 : 0, erec, dkey, ekey);
    Sorted ds;
    if (!split) {
        ds = radix_sort(ctx, "rs_rd_dict", dkey, nullptr, NE, rs_plan.bits + re_plan.bits);
    } else {
        // two-key LSD: stable sort by end, then by start
        Sorted by_e = radix_sort(ctx, "rs_rd_e", ekey, nullptr, NE, re_plan.bits);
        uint64_t *dk3 = ctx->get<uint64_t>("rd_dkey3", NE);
        launch(ctx, "rd_permute", k_permute_u64, dim3(grid_for(NE, BLOCK)), dim3(BLOCK), 0, (size_t)NE,
               (const uint32_t *)by_e.vals, (const uint64_t *)dkey, dk3);
        ds = radix_sort(ctx, "rs_rd_dict", dk3, by_e.vals, NE, rs_plan.bits);
    }
    uint32_t *dflag = ctx->get<uint32_t>("rd_dflag", NE);
    b.dincl = ctx->get<uint32_t>("rd_dincl", NE + 1);
    launch(ctx, "rd_dict_flags", k_rd_dict_flags, dim3(grid_for(NE, BLOCK)), dim3(BLOCK), 0, NE, (const uint32_t *)ds.vals,
           (const uint4 *)erec, dflag);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, dflag, b.dincl, NE, false, b.dincl + NE);
    b.dict_s = ctx->get<uint64_t>("rd_dict_s", NE);
    b.dict_e = ctx->get<uint64_t>("rd_dict_e", NE);
    uint64_t *ckey = ctx->get<uint64_t>("rd_ckey", NE);
    uint32_t *cls = ctx->get<uint32_t>("rd_cls", 2 * (NCLS + 1));
    uint32_t *cls_hist = cls;
    b.class_off = cls + (NCLS + 1);
    ACC_HIP(hipMemsetAsync(cls_hist, 0, (NCLS + 1) * sizeof(uint32_t), st));
    launch(ctx, "rd_dict_write", k_rd_dict_write, dim3(grid_for(NE, (size_t)BLOCK * RD_TS)), dim3(BLOCK), 0, NE, (const uint32_t *)ds.vals,
           (const uint32_t *)dflag, (const uint32_t *)b.dincl, erec, b.dict_s, b.dict_e, ckey, cls_hist);
    launch(ctx, "rd_class_off", k_rd_class_off, dim3(1), dim3(64), 0, (const uint32_t *)cls_hist, b.class_off);
    // (class, start) order: the (start, end)-sorted entries partitioned stably by class, one 8-bit pass
    const Sorted cs = radix_sort(ctx, "rs_rd_cls", ckey, ds.vals, NE, 6);
    b.cs_s = ctx->get<uint64_t>("rd_cs_s", NE);
    b.cs_e = ctx->get<uint64_t>("rd_cs_e", NE);
    b.cs_info = ctx->get<uint2>("rd_cs_info", NE);
    b.cs_kind = ctx->get<uint8_t>("rd_cs_kind", NE);
    launch(ctx, "rd_class_cols", k_rd_class_cols, dim3(grid_for(NE, BLOCK)), dim3(BLOCK), 0, NE, (const uint32_t *)cs.vals,
           (const uint4 *)erec, b.cs_s, b.cs_e, b.cs_info, b.cs_kind);
}

void rangedeps_batch(acc_ctx *ctx, const acc_range_batch_in *in, acc_rangedeps_view *view, const SharedDict *shared)
{
    if (!in || !view) fail(ACC_E_ARG, "null argument");
    if (in->mem != ACC_MEM_HOST && in->mem != ACC_MEM_DEVICE) fail(ACC_E_ARG, "mem must be ACC_MEM_HOST or ACC_MEM_DEVICE");
    if (in->end_inclusive > 1) fail(ACC_E_ARG, "end_inclusive must be 0 (StartInclusive) or 1 (EndInclusive)");
    RdBuild b;
    b.n = in->n_txn;
    b.P = (size_t)in->n_pairs;
    b.R = (size_t)in->n_ranges;
    if (b.P + b.R >= 0xFFFFFFFFull) fail(ACC_E_ARG, "n_pairs + n_ranges must be < 2^32");
    b.Q = (uint32_t)(b.P + b.R);
    b.end_inclusive = (int)in->end_inclusive;
    hipStream_t st = ctx->stream;
    ctx->rd_valid = false;
    const uint32_t n = b.n;

    b.arena_off = ctx->get<uint64_t>("rd_arena_off", (size_t)n + 1);
    b.rd_off = ctx->get<uint64_t>("rd_rd_off", (size_t)n + 1);
    b.u_off = ctx->get<uint64_t>("rd_u_off", (size_t)n + 1);
    if (n == 0) {
        ACC_HIP(hipMemsetAsync(b.arena_off, 0, 8, st));
        ACC_HIP(hipMemsetAsync(b.rd_off, 0, 8, st));
        ACC_HIP(hipMemsetAsync(b.u_off, 0, 8, st));
        *view = acc_rangedeps_view{ n, 0, 0, 0, 0, 0, ctx->get<uint64_t>("rd_dict_s", 1), ctx->get<uint64_t>("rd_dict_e", 1),
                                    b.arena_off, ctx->get<int32_t>("rd_arena", 1), b.rd_off, ctx->get<uint32_t>("rd_range_id", 1),
                                    b.u_off, ctx->get<uint32_t>("rd_dep_txn", 1) };
        ctx->rd_view = *view;
        ctx->rd_valid = true;
        ctx->sync();
        return;
    }

    rd_prepare(ctx, in, shared, b);
    rd_range_dict(ctx, b);
    rd_stab_queries(ctx, b);
    rd_build_txns(ctx, b);

    ctx->stat("rangedeps.entries", b.NE);
    ctx->stat("rangedeps.stored_ranges", b.n_dict);
    ctx->stat("rangedeps.queries", b.Q);
    ctx->stat("rangedeps.raw_entries", b.E);
    ctx->stat("rangedeps.stab_passes", b.stab_passes);
    ctx->stat("rangedeps.s16_txns", b.tier_txns[1]);
    ctx->stat("rangedeps.s32_txns", b.tier_txns[11]);
    ctx->stat("rangedeps.s64_txns", b.tier_txns[2]);
    ctx->stat("rangedeps.block_txns", b.block_txns);
    ctx->stat("rangedeps.global_txns", b.tier_txns[10]);
    ctx->sync();
    *view = acc_rangedeps_view{ n, b.n_dict, b.tot_arena, b.tot_rd, b.tot_u, b.tot_arena - b.tot_rd, b.dict_s, b.dict_e, b.arena_off,
                                b.o.arena, b.rd_off, b.o.range_id, b.u_off, b.o.dep_txn };
    ctx->rd_view = *view;
    ctx->rd_valid = true;
}

}  // namespace acc
