// rcmd_partial.hip — acc_rcmd_partial_rangedeps: the range half of PreAccept.calculatePartialDeps from the resident
// range-command store, builder.build().with(redundant) (messages/PreAccept.java:245-265).
//
// The stab result of acc_rcmd_rangedeps (rcmd.hip) is the builder's side. The other side, RedundantBefore.collectDeps
// (local/RedundantBefore.java:181-190, 418-421), holds one (entry.range, shardAppliedOrInvalidatedBefore) range dep per
// RedundantBefore entry a participant of the txn touches (ReducingRangeMap.foldl, utils/ReducingRangeMap.java:120-196):
// here one per interval m of the store's map with bound[m] > TxnId.NONE, Range(m) = (st - 1, en] or [st, en + 1) by the
// store's bound type. RangeDeps.with (primitives/RangeDeps.java:567-581) is a linearUnion of ranges, TxnIds and pairs.
//
// Both sides reach rd_build_txns as raw (range id << 32 | TxnId position) pairs over one id space, so the build's own
// sort and dedup of a txn's pairs is the union:
//   the union index (cached in the store, rebuilt by the first call after the table or the map changed):
//     1. k_pu_keys: the compare words of every interval's bound, live = bound > NONE; dense_rank groups the bounds
//        (Timestamp.equals bounds are one group, first[] = the lowest interval holding it);
//     2. k_pu_gloc, a thread per group: its lower bound among the stored TxnIds, absent = live and no row equals it;
//        k_pu_iloc, a thread per interval: the lower bound of Range(m) in the dictionary (Range::compare: start, then
//        end), absent = live and no stored range equals it; one scan of each absent flag, one read-back of the totals;
//     3. both maps are monotone: row j lies at j + #absent groups located at or below j, dictionary id d at d + #absent
//        intervals located at or below d, each by one upper-bound search in the located positions (k_pu_rows: ids,
//        id_row and rowpos; k_pu_dict: the union dictionary and dmap); k_pu_gwrite / k_pu_iwrite place the absent
//        bounds and ranges and leave per interval its union TxnId position, range id and the shared-pair flag;
//     4. k_pu_info: the stabbing index's (range id, row) column renamed through dmap and rowpos.
//   per call:
//     5. k_pu_tinfo: lim and tpos of every query renamed through rowpos (rows below lim are the positions below
//        rowpos[lim]); k_pu_collect<false>, a thread per participant: the run of intervals it touches (a key: one
//        lower-bound search over en; a range: the intervals it intersects), less the first one when the previous
//        participant of the same query ended in it, less the NONE bounds: its count; one scan, one read-back;
//     6. rd_stab_queries as it is over the renamed column; its E raw pairs copied to the front of a buffer of E + C;
//        k_pu_collect<true> writes the C collected pairs behind them; k_pu_records gives every query one more
//        participant record, the span of its collected pairs, behind the records of its own participants;
//     7. rd_build_txns as it is over those records (every query a "key txn" of participants + 1 records).
// A store without a bound above NONE takes acc_rcmd_rangedeps itself. Integer work only: HBM/latency bound, no MFMA.

#include "rcmd_partial.hpp"

namespace acc {

namespace pu {

constexpr uint32_t NONE = 0xFFFFFFFFu;

struct MapCols {
    const uint64_t *st, *en, *vm, *vl;
    const int32_t *vn;
    uint32_t nv, ei;
};

// Range(m) of the closed interval [st, en] in the store's bound type (k_rt_trim, rcmd.hip, reads them the same way)
__device__ __forceinline__ uint64_t iv_start(const MapCols &m, uint32_t i) { return m.ei ? m.st[i] - 1 : m.st[i]; }
__device__ __forceinline__ uint64_t iv_end(const MapCols &m, uint32_t i)
{
    const uint64_t en = m.en[i];
    return m.ei ? en : (en == ~0ull ? en : en + 1);
}

// ---------------------------------------------------------------- the union index

// per interval: the compare words of its bound (k_rc_validate's), live = bound > TxnId.NONE; g[0] counts the live ones
__global__ __launch_bounds__(BLOCK) void k_pu_keys(MapCols m, uint64_t *__restrict__ w0, uint64_t *__restrict__ w1, uint64_t *__restrict__ w2,
                                                   uint32_t *__restrict__ live, uint64_t *__restrict__ g)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool lv = false;
    if (i < m.nv) {
        w0[i] = m.vm[i];
        w1[i] = ts_w1(m.vl[i]);
        w2[i] = ts_w2(m.vn[i]);
        lv = ts_cmp(m.vm[i], m.vl[i], m.vn[i], 0ull, 0ull, 0) > 0;
        live[i] = lv ? 1u : 0u;
    }
    const unsigned long long bal = __ballot(lv);
    if (bal && lane_id() == 0) atomicAdd((unsigned long long *)&g[0], (unsigned long long)__popcll(bal));
}

// group r (one bound): gpos = its lower bound among the stored TxnIds, gfound = a row equals it, gabs = live and none does
__global__ __launch_bounds__(BLOCK) void k_pu_gloc(uint32_t G, MapCols m, const uint32_t *__restrict__ first, const uint32_t *__restrict__ live,
                                                   uint32_t n, const uint64_t *__restrict__ tm, const uint64_t *__restrict__ tl,
                                                   const int32_t *__restrict__ tn, uint32_t *__restrict__ gpos,
                                                   uint32_t *__restrict__ gfound, uint32_t *__restrict__ gabs)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= G) return;
    const uint32_t i0 = first[r];
    const uint64_t xm = m.vm[i0], xl = m.vl[i0];
    const int32_t xn = m.vn[i0];
    const uint32_t lo = lower_bound_ts(tm, tl, tn, 0, n, Ts{ xm, xl, xn });
    const bool found = lo < n && ts_cmp(tm[lo], tl[lo], tn[lo], xm, xl, xn) == 0;
    gpos[r] = lo;
    gfound[r] = found ? 1u : 0u;
    gabs[r] = live[i0] && !found ? 1u : 0u;
}

// interval i: idp = the lower bound of Range(i) in the dictionary by (start, end), iabs = live and no stored range
// equals it. The intervals ascend and are disjoint, so idp does not decrease.
__global__ __launch_bounds__(BLOCK) void k_pu_iloc(MapCols m, const uint32_t *__restrict__ live, uint32_t nd,
                                                   const uint64_t *__restrict__ ds, const uint64_t *__restrict__ de,
                                                   uint32_t *__restrict__ idp, uint32_t *__restrict__ iabs)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m.nv) return;
    const uint64_t s = iv_start(m, i), e = iv_end(m, i);
    const uint32_t lo = partition_point(0u, nd, [&](uint32_t md) { return ds[md] < s || (ds[md] == s && de[md] < e); });
    const bool found = lo < nd && ds[lo] == s && de[lo] == e;
    idp[i] = lo;
    iabs[i] = live[i] && !found ? 1u : 0u;
}

// row j < n: its union position j + #absent bounds located at or below it (an absent bound located at j compares below
// row j), the id and id_row there; j == n: rowpos[n] = n_ids
__global__ __launch_bounds__(BLOCK) void k_pu_rows(uint32_t n, uint32_t G, const uint32_t *__restrict__ gpos, const uint32_t *__restrict__ gax,
                                                   const uint64_t *__restrict__ tm, const uint64_t *__restrict__ tl,
                                                   const int32_t *__restrict__ tn, uint32_t *__restrict__ rowpos,
                                                   uint64_t *__restrict__ im, uint64_t *__restrict__ il, int32_t *__restrict__ in,
                                                   uint32_t *__restrict__ id_row)
{
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j > n) return;
    const uint32_t u = j + gax[upper_bound(gpos, 0, G, j)];
    rowpos[j] = u;
    if (j == n) return;
    im[u] = tm[j]; il[u] = tl[j]; in[u] = tn[j];
    id_row[u] = j;
}

// an absent bound: its raw bits (those of the lowest interval holding it) at gpos + #absent bounds below it
__global__ __launch_bounds__(BLOCK) void k_pu_gwrite(uint32_t G, MapCols m, const uint32_t *__restrict__ first, const uint32_t *__restrict__ gpos,
                                                     const uint32_t *__restrict__ gabs, const uint32_t *__restrict__ gax,
                                                     uint64_t *__restrict__ im, uint64_t *__restrict__ il, int32_t *__restrict__ in,
                                                     uint32_t *__restrict__ id_row)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= G || !gabs[r]) return;
    const uint32_t i0 = first[r], u = gpos[r] + gax[r];
    im[u] = m.vm[i0]; il[u] = m.vl[i0]; in[u] = m.vn[i0];
    id_row[u] = NONE;
}

// dictionary id d at d + #absent interval ranges located at or below it
__global__ __launch_bounds__(BLOCK) void k_pu_dict(uint32_t nd, uint32_t nv, const uint32_t *__restrict__ idp, const uint32_t *__restrict__ iax,
                                                   const uint64_t *__restrict__ ds, const uint64_t *__restrict__ de,
                                                   uint32_t *__restrict__ dmap, uint64_t *__restrict__ us, uint64_t *__restrict__ ue)
{
    const uint32_t d = blockIdx.x * BLOCK + threadIdx.x;
    if (d >= nd) return;
    const uint32_t u = d + iax[upper_bound(idp, 0, nv, d)];
    dmap[d] = u;
    us[u] = ds[d]; ue[u] = de[d];
}

// interval i, live: its union range id (Range(i) written there when absent), the union position of its bound, and
// ishare = a non-erased row equals the bound and holds exactly Range(i) (the sync point stored as a range command: the
// stab returns the same pair to every query that admits the row). Not live: no dep.
__global__ __launch_bounds__(BLOCK) void k_pu_iwrite(MapCols m, const uint32_t *__restrict__ live, const uint32_t *__restrict__ rank,
                                                     const uint32_t *__restrict__ gpos, const uint32_t *__restrict__ gfound,
                                                     const uint32_t *__restrict__ gax, const uint32_t *__restrict__ idp,
                                                     const uint32_t *__restrict__ iabs, const uint32_t *__restrict__ iax,
                                                     const uint8_t *__restrict__ flags, const uint32_t *__restrict__ rng_off,
                                                     const uint64_t *__restrict__ rs, const uint64_t *__restrict__ re,
                                                     uint64_t *__restrict__ us, uint64_t *__restrict__ ue, uint32_t *__restrict__ ipos,
                                                     uint32_t *__restrict__ irid, uint32_t *__restrict__ ishare)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m.nv) return;
    if (!live[i]) { ipos[i] = NONE; irid[i] = NONE; ishare[i] = 0; return; }
    const uint64_t s = iv_start(m, i), e = iv_end(m, i);
    const uint32_t rid = idp[i] + iax[i];
    if (iabs[i]) { us[rid] = s; ue[rid] = e; }
    const uint32_t r = rank[i], row = gpos[r];
    irid[i] = rid;
    ipos[i] = row + gax[r];
    uint32_t sh = 0;
    if (gfound[r] && !(flags[row] & ACC_RCMD_ERASED)) {
        const uint32_t a = rng_off[row], b = rng_off[row + 1];
        const uint32_t k = lower_bound(rs, a, b, s);   // a command's ranges are sorted and disjoint
        sh = k < b && rs[k] == s && re[k] == e ? 1u : 0u;
    }
    ishare[i] = sh;
}

__global__ __launch_bounds__(BLOCK) void k_pu_info(uint32_t NE, const uint2 *__restrict__ info, const uint32_t *__restrict__ dmap,
                                                   const uint32_t *__restrict__ rowpos, uint2 *__restrict__ out)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= NE) return;
    const uint2 v = info[k];
    out[k] = make_uint2(dmap[v.x], rowpos[v.y]);
}

// ---------------------------------------------------------------- collect

// lim (rows below it) and tpos (the query's own row) as union positions
__global__ __launch_bounds__(BLOCK) void k_pu_tinfo(uint32_t nq, const uint32_t *__restrict__ rowpos, uint4 *__restrict__ tinfo)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= nq) return;
    uint4 t = tinfo[q];
    t.x = rowpos[t.x];
    if (t.y != NONE) t.y = rowpos[t.y];
    tinfo[q] = t;
}

struct Parts {
    uint32_t P, Q;
    const uint32_t *owner, *rowner, *key_off, *rng_off;
    const uint64_t *key, *rs, *re;
};

// the run [i0, i1) of intervals participant w touches, and the last interval the previous participant of its query
// touched (NONE: none, or w is the query's first)
__device__ __forceinline__ void touched(const MapCols &m, const Parts &p, uint32_t w, uint32_t &i0, uint32_t &i1, uint32_t &prev)
{
    prev = NONE;
    if (w < p.P) {
        const uint64_t k = p.key[w];
        i0 = lower_bound(m.en, 0, m.nv, k);
        i1 = i0 < m.nv && m.st[i0] <= k ? i0 + 1 : i0;
        if (w > p.key_off[p.owner[w]]) {
            const uint64_t kp = p.key[w - 1];
            const uint32_t j = lower_bound(m.en, 0, m.nv, kp);
            if (j < m.nv && m.st[j] <= kp) prev = j;
        }
        return;
    }
    const uint32_t r = w - p.P;
    // the intervals (is, ie) with ie > a and is < b: two ranges of one bound type intersect as sets of keys, touching
    // ends do not. ie > a: en > a (EndInclusive), en + 1 > a; is < b: st - 1 < b, st < b
    auto run = [&](uint64_t a, uint64_t b, uint32_t &f, uint32_t &l) {
        f = m.ei ? (a == ~0ull ? m.nv : lower_bound(m.en, 0, m.nv, a + 1)) : lower_bound(m.en, 0, m.nv, a);
        l = m.ei ? (b == ~0ull ? m.nv : lower_bound(m.st, 0, m.nv, b + 1)) : lower_bound(m.st, 0, m.nv, b);
        if (l < f) l = f;
    };
    run(p.rs[r], p.re[r], i0, i1);
    if (r > p.rng_off[p.rowner[r]]) {
        uint32_t f, l;
        run(p.rs[r - 1], p.re[r - 1], f, l);
        if (l > f) prev = l - 1;
    }
}

// Participant w: the live intervals of its run, the first left out when the previous participant of its query ended in
// it (a query's participants ascend, so do the intervals it meets: each counts once per query). WRITE == false: cnt[w].
// WRITE: the pairs (union range id << 32 | union TxnId position) from ent[base + coff[w]]; g[1] counts the pairs the
// stab side returns too: ishare, and the row passes the query's tests (below lim, not its own, of a witnessed kind;
// il: the lsb column of the union ids, the row's own bits where a row equals the bound).
template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_pu_collect(MapCols m, Parts p, const uint32_t *__restrict__ ipos, const uint32_t *__restrict__ irid,
                                                      const uint32_t *__restrict__ ishare, const uint4 *__restrict__ tinfo,
                                                      const uint64_t *__restrict__ il,
                                                      uint64_t *__restrict__ cnt, const uint64_t *__restrict__ coff, uint64_t base,
                                                      uint64_t *__restrict__ ent, uint64_t *__restrict__ g)
{
    const uint32_t w = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t shared = 0;
    if (w < p.Q) {
        uint32_t i0, i1, prev;
        touched(m, p, w, i0, i1, prev);
        if (i0 < i1 && prev == i0) ++i0;
        uint64_t c = 0;
        uint4 t = make_uint4(0, 0, 0, 0);
        uint64_t dst = 0;
        if constexpr (WRITE) {
            t = tinfo[w < p.P ? p.owner[w] : p.rowner[w - p.P]];
            dst = base + coff[w];
        }
        for (uint32_t i = i0; i < i1; ++i) {
            const uint32_t u = ipos[i];
            if (u == NONE) continue;
            if constexpr (WRITE) {
                ent[dst + c] = ((uint64_t)irid[i] << 32) | u;
                if (ishare[i] && u < t.x && u != t.y && ((t.z >> ((uint32_t)(il[u] >> 1) & 7u)) & 1u)) ++shared;
            }
            ++c;
        }
        if constexpr (!WRITE) cnt[w] = c;
    }
    if constexpr (WRITE) {
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) shared += shfl_xor(shared, dd);
        if (lane_id() == 0 && shared) atomicAdd((unsigned long long *)&g[1], (unsigned long long)shared);
    }
}

// The build's participant records: query q owns records [koff2[q], koff2[q + 1]), koff2[q] = key_off[q] + rng_off[q] + q:
// those of its own participants as the stab left them, then one for the span of its collected pairs.
__global__ __launch_bounds__(BLOCK) void k_pu_records(uint32_t nq, Parts p, const ulonglong2 *__restrict__ q_out, const uint64_t *__restrict__ coff,
                                                      uint64_t base, uint32_t *__restrict__ koff2, ulonglong2 *__restrict__ out)
{
    const uint32_t x = blockIdx.x * BLOCK + threadIdx.x;
    if (x < p.Q) {
        const bool key = x < p.P;
        const uint32_t q = key ? p.owner[x] : p.rowner[x - p.P];
        const uint32_t idx = key ? x + p.rng_off[q] + q : (x - p.P) + p.key_off[q] + q;
        out[idx] = q_out ? q_out[x] : make_ulonglong2(0, 0);
    }
    if (x <= nq) {
        const uint32_t k0 = p.key_off[x], r0 = p.rng_off[x];
        koff2[x] = k0 + r0 + x;
        if (x < nq) {
            const uint32_t k1 = p.key_off[x + 1], r1 = p.rng_off[x + 1];
            // its participants are its keys, or its ranges (validated: never both)
            const uint32_t w0 = k1 > k0 ? k0 : p.P + r0, w1 = k1 > k0 ? k1 : p.P + r1;
            out[k1 + r1 + x] = make_ulonglong2(base + coff[w0], coff[w1] - coff[w0]);
        }
    }
}

}  // namespace pu

using namespace pu;

// ---- the store's own arrays: grown with headroom, contents not kept. Every call on the store has synchronised its
// context before it returned, so nothing reads an array freed here.
template <class T>
static T *fit(T *&p, size_t &cap, size_t count)
{
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    if (cap < bytes) {
        if (p) ACC_HIP(hipFree(p));
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 2;
        ACC_HIP(hipMalloc(reinterpret_cast<void **>(&p), want));
        cap = want;
    }
    return p;
}

void rcmd_union_free(acc_rcmd *s)
{
    acc_rcmd_union &u = s->u;
    for (void *p : { (void *)u.im, (void *)u.il, (void *)u.in, (void *)u.id_row, (void *)u.dict_s, (void *)u.dict_e, (void *)u.cs_info,
                     (void *)u.rowpos, (void *)u.ipos, (void *)u.irid, (void *)u.ishare, (void *)u.arange })
        (void)hipFree(p);
    u = acc_rcmd_union{};
}

static MapCols map_cols(const acc_rcmd *store)
{
    const acc_maxconflicts *m = store->rb;
    return MapCols{ m->st, m->en, m->vm, m->vl, m->vn, (uint32_t)m->nv, store->end_inclusive };
}

// steps 1-4 of the file comment; leaves u.valid set (u.live == 0: no interval holds a bound above NONE, nothing built)
static void build_union(acc_ctx *ctx, acc_rcmd *store)
{
    acc_rcmd_union &u = store->u;
    u.valid = false;
    u.live = 0;
    const acc_maxconflicts *mp = store->rb;
    if (!mp || mp->nv == 0) { u.valid = true; return; }
    if (mp->nv >= 0xFFFFFFFFull) fail(ACC_E_CAP, "RedundantBefore map too large (intervals >= 2^32 - 1)");
    hipStream_t st = ctx->stream;
    const MapCols m = map_cols(store);
    const uint32_t nv = m.nv, n = store->n, nd = store->n_dict, NE = store->NE;
    u.builds += 1;

    // ---- 1. the bounds grouped
    uint64_t *g = ctx->get<uint64_t>("pu_g", 8);
    ACC_HIP(hipMemsetAsync(g, 0, 8 * sizeof(uint64_t), st));
    uint64_t *w[3] = { ctx->get<uint64_t>("pu_w0", nv), ctx->get<uint64_t>("pu_w1", nv), ctx->get<uint64_t>("pu_w2", nv) };
    uint32_t *live = ctx->get<uint32_t>("pu_live", nv);
    launch(ctx, "pu_keys", k_pu_keys, dim3(grid_for(nv, BLOCK)), dim3(BLOCK), 0, m, w[0], w[1], w[2], live, g);
    const uint64_t *words[3] = { w[0], w[1], w[2] };
    const DenseRank dr = dense_rank(ctx, "pu_dr", nv, 3, words, nullptr, nullptr, true);
    uint32_t G, nlive;
    {
        ReadBack rb(ctx);
        const auto hg = rb.u64(g);
        const auto cnt = rb.u64(dr.count_dev);
        rb.wait();
        nlive = (uint32_t)(uint64_t)hg;
        G = (uint32_t)(uint64_t)cnt;
    }
    if (nlive == 0) { u.valid = true; return; }

    // ---- 2. both sides located, the absent ones counted
    uint32_t *gpos = ctx->get<uint32_t>("pu_gpos", G), *gfound = ctx->get<uint32_t>("pu_gfound", G), *gabs = ctx->get<uint32_t>("pu_gabs", G);
    uint32_t *gax = ctx->get<uint32_t>("pu_gax", (size_t)G + 1);
    uint32_t *idp = ctx->get<uint32_t>("pu_idp", nv), *iabs = ctx->get<uint32_t>("pu_iabs", nv);
    uint32_t *iax = ctx->get<uint32_t>("pu_iax", (size_t)nv + 1);
    launch(ctx, "pu_gloc", k_pu_gloc, dim3(grid_for(G, BLOCK)), dim3(BLOCK), 0, G, m, (const uint32_t *)dr.first, (const uint32_t *)live, n,
           (const uint64_t *)store->tm, (const uint64_t *)store->tl, (const int32_t *)store->tn, gpos, gfound, gabs);
    launch(ctx, "pu_iloc", k_pu_iloc, dim3(grid_for(nv, BLOCK)), dim3(BLOCK), 0, m, (const uint32_t *)live, nd,
           (const uint64_t *)store->dict_s, (const uint64_t *)store->dict_e, idp, iabs);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, gabs, gax, G, true, gax + G);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, iabs, iax, nv, true, iax + nv);
    uint32_t na, ra;
    {
        ReadBack rb(ctx);
        const auto a = rb.u32(gax + G);
        const auto b = rb.u32(iax + nv);
        rb.wait();
        na = a; ra = b;
    }
    if ((uint64_t)n + na >= 0xFFFFFFFFull) fail(ACC_E_CAP, "union of TxnIds too large (>= 2^32 - 1)");
    if ((uint64_t)nd + ra >= 0xFFFFFFFFull) fail(ACC_E_CAP, "union of ranges too large (>= 2^32 - 1)");
    const uint32_t n_ids = n + na, n_dict = nd + ra;

    // ---- 3, 4. the union's arrays, in the store
    fit(u.im, u.cap[0], n_ids); fit(u.il, u.cap[1], n_ids); fit(u.in, u.cap[2], n_ids); fit(u.id_row, u.cap[3], n_ids);
    fit(u.dict_s, u.cap[4], n_dict); fit(u.dict_e, u.cap[5], n_dict);
    fit(u.cs_info, u.cap[6], NE);
    fit(u.rowpos, u.cap[7], (size_t)n + 1);
    fit(u.ipos, u.cap[8], nv); fit(u.irid, u.cap[9], nv); fit(u.ishare, u.cap[10], nv);
    uint32_t *dmap = ctx->get<uint32_t>("pu_dmap", nd);
    launch(ctx, "pu_rows", k_pu_rows, dim3(grid_for((size_t)n + 1, BLOCK)), dim3(BLOCK), 0, n, G, (const uint32_t *)gpos, (const uint32_t *)gax,
           (const uint64_t *)store->tm, (const uint64_t *)store->tl, (const int32_t *)store->tn, u.rowpos, u.im, u.il, u.in, u.id_row);
    launch(ctx, "pu_gwrite", k_pu_gwrite, dim3(grid_for(G, BLOCK)), dim3(BLOCK), 0, G, m, (const uint32_t *)dr.first, (const uint32_t *)gpos,
           (const uint32_t *)gabs, (const uint32_t *)gax, u.im, u.il, u.in, u.id_row);
    if (nd)
        launch(ctx, "pu_dict", k_pu_dict, dim3(grid_for(nd, BLOCK)), dim3(BLOCK), 0, nd, nv, (const uint32_t *)idp, (const uint32_t *)iax,
               (const uint64_t *)store->dict_s, (const uint64_t *)store->dict_e, dmap, u.dict_s, u.dict_e);
    launch(ctx, "pu_iwrite", k_pu_iwrite, dim3(grid_for(nv, BLOCK)), dim3(BLOCK), 0, m, (const uint32_t *)live, (const uint32_t *)dr.rank,
           (const uint32_t *)gpos, (const uint32_t *)gfound, (const uint32_t *)gax, (const uint32_t *)idp, (const uint32_t *)iabs,
           (const uint32_t *)iax, (const uint8_t *)store->flags, (const uint32_t *)store->rng_off, (const uint64_t *)store->rs,
           (const uint64_t *)store->re, u.dict_s, u.dict_e, u.ipos, u.irid, u.ishare);
    if (NE)
        launch(ctx, "pu_info", k_pu_info, dim3(grid_for(NE, BLOCK)), dim3(BLOCK), 0, NE, (const uint2 *)store->cs_info, (const uint32_t *)dmap,
               (const uint32_t *)u.rowpos, u.cs_info);
    ctx->sync();   // the index is complete before the store calls it valid
    u.n_ids = n_ids;
    u.n_dict = n_dict;
    u.live = nlive;
    u.valid = true;
}

// id_row of a store without a bound above NONE: 0, 1, .., n - 1, copied in once per table size (no kernel)
static const uint32_t *arange_rows(acc_ctx *ctx, acc_rcmd *store)
{
    acc_rcmd_union &u = store->u;
    const uint32_t n = store->n;
    if (u.arange && u.arange_n >= n && n) return u.arange;
    fit(u.arange, u.cap[11], n);
    std::vector<uint32_t> h(n);
    for (uint32_t i = 0; i < n; ++i) h[i] = i;
    if (n) ACC_HIP(hipMemcpy(u.arange, h.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    u.arange_n = n;
    return u.arange;
}

void rcmd_partial_rangedeps(acc_ctx *ctx, acc_rcmd *store, const acc_cfk_mixed_queries *in, acc_rcmd_partial_view *out)
{
    if (!store || !in || !out) fail(ACC_E_ARG, "null argument");
    acc_rcmd_union &u = store->u;
    auto union_stats = [&](uint64_t intervals, uint64_t shared) {
        ctx->stat("rcmd.partial_intervals", intervals);
        ctx->stat("rcmd.partial_pairs_shared", shared);
        ctx->stat("rcmd.union_builds", u.builds);
        ctx->stat("rcmd.union_ids", u.live ? u.n_ids : store->n);
        ctx->stat("rcmd.union_ranges", u.live ? u.n_dict : store->n_dict);
    };
    // a store never marked: acc_rcmd_rangedeps, its kernels and no others
    if (!store->rb || store->rb->nv == 0) { u.valid = true; u.live = 0; }
    if (u.valid && u.live == 0) {
        rcmd_rangedeps(ctx, store, in, &out->rd);
        out->n_ids = out->n_cmd = store->n;
        out->ids = acc_ts_cols{ store->tm, store->tl, store->tn };
        out->id_row = arange_rows(ctx, store);
        union_stats(0, 0);
        return;
    }

    // ---- the front end of acc_rcmd_rangedeps: the same checks in the same order
    RdBuild b = rcmd_begin_rangedeps(ctx, store, in);
    const uint32_t nq = in->n_query;
    uint32_t *owner = nullptr;
    rc::Queries Q{};
    if (nq) Q = rcmd_prep_rangedeps(ctx, store, in, b, owner);
    if (!u.valid) {
        build_union(ctx, store);
        if (u.live == 0) {   // only NONE bounds: from here on the store is as one never marked
            rcmd_rangedeps(ctx, store, in, &out->rd);
            out->n_ids = out->n_cmd = store->n;
            out->ids = acc_ts_cols{ store->tm, store->tl, store->tn };
            out->id_row = arange_rows(ctx, store);
            union_stats(0, 0);
            return;
        }
    }
    hipStream_t st = ctx->stream;
    auto publish_ids = [&] {
        out->n_ids = u.n_ids;
        out->n_cmd = store->n;
        out->ids = acc_ts_cols{ u.im, u.il, u.in };
        out->id_row = u.id_row;
    };
    if (nq == 0) {   // no query: the empty view over the union dictionary
        ACC_HIP(hipMemsetAsync(b.arena_off, 0, 8, st));
        ACC_HIP(hipMemsetAsync(b.rd_off, 0, 8, st));
        ACC_HIP(hipMemsetAsync(b.u_off, 0, 8, st));
        out->rd = acc_rangedeps_view{ 0, u.n_dict, 0, 0, 0, 0, u.dict_s, u.dict_e, b.arena_off, ctx->get<int32_t>("rd_arena", 1),
                                      b.rd_off, ctx->get<uint32_t>("rd_range_id", 1), b.u_off, ctx->get<uint32_t>("rd_dep_txn", 1) };
        ctx->rd_view = out->rd;
        ctx->rd_valid = true;
        rcmd_rangedeps_stats(ctx, store, b, false);
        union_stats(0, 0);
        ctx->sync();
        publish_ids();
        return;
    }

    // ---- 5. the queries' rows in union positions; the collected pairs counted
    const MapCols m = map_cols(store);
    const Parts parts{ (uint32_t)b.P, b.Q, owner, b.rowner, Q.key_off, Q.rng_off, Q.key, Q.rs, Q.re };
    launch(ctx, "pu_tinfo", k_pu_tinfo, dim3(grid_for(nq, BLOCK)), dim3(BLOCK), 0, nq, (const uint32_t *)u.rowpos, b.tinfo);
    uint64_t *g = ctx->get<uint64_t>("pu_g", 8);
    ACC_HIP(hipMemsetAsync(g, 0, 8 * sizeof(uint64_t), st));
    uint64_t *cnt = ctx->get<uint64_t>("pu_cnt", b.Q), *coff = ctx->get<uint64_t>("pu_coff", (size_t)b.Q + 1);
    if (b.Q)
        launch(ctx, "pu_count", k_pu_collect<false>, dim3(grid_for(b.Q, BLOCK)), dim3(BLOCK), 0, m, parts, (const uint32_t *)u.ipos,
               (const uint32_t *)u.irid, (const uint32_t *)u.ishare, (const uint4 *)b.tinfo,
               (const uint64_t *)u.il, cnt, (const uint64_t *)nullptr, 0ull, (uint64_t *)nullptr, g);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, cnt, coff, b.Q, true, coff + b.Q);
    uint64_t C;
    {
        ReadBack rb(ctx);
        const auto c = rb.u64(coff + b.Q);
        rb.wait();
        C = c;
    }

    // ---- 6. the stab over the renamed column, its pairs and the collected ones in one buffer
    const bool stab = store->NE != 0;
    if (stab) {
        rcmd_bind_store_index(b, store, Q, owner);
        b.cs_info = u.cs_info;
        rd_stab_queries(ctx, b);
    } else {
        b.key_off = Q.key_off; b.rng_off = Q.rng_off;
        b.dict.batch_sorted = true;
        b.NE = 0;
        b.dincl = ctx->get<uint32_t>("pu_dincl0", 1);
        ACC_HIP(hipMemsetAsync(b.dincl, 0, 4, st));
        b.E = 0;
    }
    const uint64_t E = b.E, tot = E + C;
    if (tot >= (1ull << 40)) fail(ACC_E_CAP, "too many raw range deps");
    uint64_t *ent = ctx->get<uint64_t>("pu_ent", tot);
    if (E) ACC_HIP(hipMemcpyAsync(ent, b.v.ent, E * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    if (b.Q && C)
        launch(ctx, "pu_collect", k_pu_collect<true>, dim3(grid_for(b.Q, BLOCK)), dim3(BLOCK), 0, m, parts, (const uint32_t *)u.ipos,
               (const uint32_t *)u.irid, (const uint32_t *)u.ishare, (const uint4 *)b.tinfo,
               (const uint64_t *)u.il, (uint64_t *)nullptr, (const uint64_t *)coff, E, ent, g);
    const size_t nrec = (size_t)b.Q + nq;
    uint32_t *koff2 = ctx->get<uint32_t>("pu_koff2", (size_t)nq + 1), *zoff = ctx->get<uint32_t>("pu_zoff", (size_t)nq + 1);
    ulonglong2 *rec = ctx->get<ulonglong2>("pu_rec", nrec);
    ACC_HIP(hipMemsetAsync(zoff, 0, ((size_t)nq + 1) * sizeof(uint32_t), st));
    launch(ctx, "pu_records", k_pu_records, dim3(grid_for(std::max<size_t>(b.Q, (size_t)nq + 1), BLOCK)), dim3(BLOCK), 0, nq, parts,
           (const ulonglong2 *)(stab ? b.v.q_out : nullptr), (const uint64_t *)coff, E, koff2, rec);

    // ---- 7. the build as it is: every query a txn of participants + 1 records; TxnId positions and range ids are the
    // union's (its 32-bit sort keys are decided from npos and NE: the union's counts stand in where they are larger)
    b.key_off = koff2;
    b.rng_off = zoff;
    b.P = nrec;
    b.v.q_out = rec;
    b.v.ent = ent;
    b.E = tot;
    b.npos = u.n_ids;
    const uint32_t saved_flags = ctx->flags;
    if (u.n_dict >= (1u << 26)) ctx->flags |= ACC_OPT_RD_WIDE_SORT;
    struct Restore { acc_ctx *c; uint32_t f; ~Restore() { c->flags = f; } } restore{ ctx, saved_flags };
    rd_build_txns(ctx, b);
    b.n_dict = u.n_dict;
    b.dict_s = u.dict_s;
    b.dict_e = u.dict_e;
    b.P = parts.P;
    b.E = E;
    b.NE = store->NE;
    rcmd_rangedeps_stats(ctx, store, b, stab);
    uint64_t shared;
    {
        ReadBack rb(ctx);
        const auto s = rb.u64(g + 1);
        rb.wait();
        shared = s;
    }
    union_stats(C, shared);
    rcmd_publish_view(ctx, b, &out->rd);
    publish_ids();
}

}  // namespace acc
