// rangedeps_stab.hip — stage 3 of RangeDeps (rangedeps.hip has the pipeline): the query records sorted by low bound and
// the stabbing pass over the class-ordered entries, which leaves every query's (range id, TxnId position) pairs in
// View::ent.

#include "rangedeps.hpp"
#include "search.hpp"

namespace acc {

namespace rd {

// ---------------------------------------------------------------- queries

__global__ __launch_bounds__(BLOCK) void k_rd_qrec(uint32_t P, uint32_t R, const uint64_t *__restrict__ key_code,
                                                   const uint32_t *__restrict__ owner, const uint64_t *__restrict__ rs,
                                                   const uint64_t *__restrict__ re, const uint32_t *__restrict__ rowner,
                                                   const uint4 *__restrict__ tinfo, Runs plan, QRec *__restrict__ rec,
                                                   uint64_t *__restrict__ qkey, uint32_t rbit, int ibits, int qdrop)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P + R) return;
    QRec r;
    uint32_t t;
    if (q < P) { r.lo = r.hi = key_code[q]; t = owner[q]; }
    else { r.lo = rs[q - P]; r.hi = re[q - P]; t = rowner[q - P]; }
    const uint4 ti = tinfo[t];
    r.lim = ti.x; r.tpos = ti.y; r.flags = ti.z | (ti.w << 8); r.q = q;
    rec[q] = r;
    // range queries after the key queries (rbit < 64): a range query scans its whole span, so mixing the two in one
    // wave would leave the key lanes idle behind it
    // ibits > 0: the query index packed under the key (a keys-only sort, 8 B per element moved instead of 12)
    // rbit < 62: range queries also grouped by width (2 bits under the range bit: widths below 2^4, 2^8, 2^12, beyond),
    // so a block's lanes scan spans of similar length — a wave waits for its widest lane
    uint64_t k = pext_runs(r.lo, plan);
    if (q >= P && rbit < 64) {
        if (rbit < 62) {
            const uint64_t w = r.hi - r.lo;
            const uint32_t g = min(3u, (63u - (uint32_t)__builtin_clzll(w | 1)) / 4u);
            k |= (4ull | g) << rbit;
        } else {
            k |= 1ull << rbit;
        }
    }
    // qdrop: the low key bits the sort leaves out (the stabbing blocks need neighbouring queries, not an exact order)
    qkey[q] = ibits ? ((k >> qdrop) << ibits) | q : k >> qdrop;
}

// The sorted runs' bounds bnd[0..4]: key queries [0, bnd[0] = P), range queries of width group g at [bnd[g], bnd[g + 1])
// (the group in the top 3 sorted key bits: 4 | g). One thread per group boundary, a binary search over the sorted keys.
__global__ void k_rd_qgroups(const uint64_t *__restrict__ keys, uint32_t P, uint32_t Q, int top_shift, int groups,
                             uint32_t *__restrict__ bnd)
{
    const uint32_t g = threadIdx.x;
    if (g > 4) return;
    uint32_t b = g == 0 ? P : Q;
    if (groups && g >= 1 && g <= 3) {
        // first sorted position whose group field is >= 4 | g
        b = partition_point(P, Q, [&](uint32_t m) { return (keys[m] >> top_shift) < (4u | g); });
    }
    bnd[g] = b;
}

// sorted records, and per block of BLOCK sorted queries (the stabbing blocks) the largest high bound
// Each sorted run (the key queries, then each width group of range queries) starts at a block boundary: no block mixes
// two runs, so no block's window spans the key space between them. Run g of c_g queries at padded position base_g
// (base_0 = Pp = P rounded up to a block, base_{g+1} = base_g + c_g rounded up); the gaps hold PAD records.
constexpr uint32_t QPAD = 1u << 31;
// perm: the sorted query indices, or (perm null) the low bits (imask) of the sorted packed keys pk
__global__ __launch_bounds__(BLOCK) void k_rd_qsort(uint32_t Qp, uint32_t P, uint32_t Pp, const uint32_t *__restrict__ bnd,
                                                    const uint32_t *__restrict__ perm,
                                                    const uint64_t *__restrict__ pk, uint64_t imask,
                                                    const QRec *__restrict__ rec, QRec *__restrict__ srec,
                                                    uint64_t *__restrict__ blo, uint64_t *__restrict__ bhi)
{
    __shared__ uint64_t wh[WAVES], wl[WAVES];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint64_t h = 0, l = ~0ull;
    if (i < Qp) {
        uint32_t j = 0xFFFFFFFFu;   // sorted position of padded position i (none: PAD)
        if (i < P) {
            j = i;
        } else {
            uint32_t base = Pp;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t c = bnd[g + 1] - bnd[g];
                if (i >= base && i < base + c) j = bnd[g] + (i - base);
                base += (c + BLOCK - 1) / BLOCK * BLOCK;
            }
        }
        if (j == 0xFFFFFFFFu) {
            QRec r{};
            r.flags = QPAD;
            srec[i] = r;
        } else {
            const QRec r = rec[perm ? perm[j] : (uint32_t)(pk[j] & imask)];
            srec[i] = r; h = r.hi; l = r.lo;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = shfl_xor(h, d), p = shfl_xor(l, d);
        h = o > h ? o : h;
        l = p < l ? p : l;
    }
    if (lane_id() == 0) { wh[threadIdx.x >> 6] = h; wl[threadIdx.x >> 6] = l; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t m = 0, n = ~0ull;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) { m = wh[w] > m ? wh[w] : m; n = wl[w] < n ? wl[w] : n; }
        bhi[blockIdx.x] = m;
        blo[blockIdx.x] = n;
    }
}

// ---------------------------------------------------------------- stabbing

struct StabTile {
    uint64_t s[TILE], e[TILE];
    uint32_t s32[TILE], e32[TILE];  // flat tile, rel: bounds - rbase (ends clamped to 2^32 - 1)
    uint2 info[TILE];
    uint8_t kind[TILE];
    uint64_t rbase;
    uint32_t rel;                  // flat tile: the block's window spans less than 2^32 - 1 above rbase
    uint32_t b0[NCLS], b1[NCLS];   // the block's window per width class
    uint32_t pre[NCLS + 1];        // flat tile: class c at [pre[c], pre[c + 1])
    uint32_t red[WAVES];
    uint64_t base;
};

// One pass over the block's windows: EMIT = false counts this query's pairs, EMIT = true writes them at out. The
// (class, tile) sequence is software-pipelined: the next tile's entries are loaded into registers while the current
// one is scanned from LDS, so a block pays one memory latency per pass instead of one per tile.
constexpr int ST_PT = TILE / BLOCK;   // tile entries per thread
static_assert(TILE >= BLOCK && TILE % BLOCK == 0, "a tile is whole rounds of the block");

struct StabRegs {
    uint64_t s[ST_PT], e[ST_PT];
    uint2 info[ST_PT];
    uint32_t kind[ST_PT];
};

__device__ __forceinline__ void stab_load(const View &v, StabRegs &g, uint32_t base, uint32_t len)
{
#pragma unroll
    for (int u = 0; u < ST_PT; ++u) {
        const uint32_t k = threadIdx.x + (uint32_t)u * BLOCK;
        if (k < len) {
            g.s[u] = v.cs_s[base + k];
            g.e[u] = v.cs_e[base + k];
            g.info[u] = v.cs_info[base + k];
            g.kind[u] = v.cs_kind[base + k];
        }
    }
}

// next non-empty (class, tile) after (c, base) (c = NCLS: none)
__device__ __forceinline__ void stab_next(const StabTile &T, uint32_t &c, uint32_t &base)
{
    base += TILE;
    if (c < (uint32_t)NCLS && base < T.b1[c]) return;
    for (++c; c < (uint32_t)NCLS; ++c)
        if (T.b0[c] < T.b1[c]) { base = T.b0[c]; return; }
}

// REL: the probes on 32-bit offsets above the block's rbase (as stab_flat_rel)
template <bool EMIT, bool REL>
__device__ __forceinline__ uint32_t stab_pass(const View &v, StabTile &T, bool valid, const QRec &r, uint64_t out,
                                              uint64_t *stage)
{
    const uint32_t tid = threadIdx.x;
    const bool isr = (r.flags >> 8) & 1u;
    const uint32_t wm = r.flags & 0xFFu;
    const uint64_t rb = REL ? T.rbase : 0;
    const uint32_t qlo = (uint32_t)(r.lo - rb), qhi = (uint32_t)(r.hi - rb);   // (REL)
    uint32_t count = 0;
    uint32_t c = 0, base = 0;
    while (c < (uint32_t)NCLS && T.b0[c] >= T.b1[c]) ++c;
    if (c < (uint32_t)NCLS) base = T.b0[c];
    StabRegs g;
    if (c < (uint32_t)NCLS) stab_load(v, g, base, min((uint32_t)TILE, T.b1[c] - base));
    while (c < (uint32_t)NCLS) {
        const uint32_t len = min((uint32_t)TILE, T.b1[c] - base);
#pragma unroll
        for (int u = 0; u < ST_PT; ++u) {
            const uint32_t k = tid + (uint32_t)u * BLOCK;
            if (k < len) {
                if (REL) {
                    T.s32[k] = (uint32_t)(g.s[u] - rb);
                    T.e32[k] = g.e[u] - rb < 0xFFFFFFFFull ? (uint32_t)(g.e[u] - rb) : 0xFFFFFFFFu;
                } else {
                    T.s[k] = g.s[u]; T.e[k] = g.e[u];
                }
                T.info[k] = g.info[u]; T.kind[k] = (uint8_t)g.kind[u];
            }
        }
        __syncthreads();
        uint32_t c2 = c, base2 = base;
        stab_next(T, c2, base2);
        if (c2 < (uint32_t)NCLS) stab_load(v, g, base2, min((uint32_t)TILE, T.b1[c2] - base2));
        if (valid) {
            const uint64_t W = class_width(c);
            // this query's own window inside the tile: starts in [lo - W, hi]
            uint32_t k;
            if (REL) k = lower_bound(T.s32, 0, len, (uint64_t)qlo > W ? qlo - (uint32_t)W : 0u);
            else k = lower_bound(T.s, 0, len, r.lo > W ? r.lo - W : 0);
            for (; k < len; ++k) {
                bool hit;
                if (REL) {
                    const uint32_t s = T.s32[k];
                    if (s > qhi) break;
                    const uint32_t e = T.e32[k];
                    if (isr) hit = s < qhi && e > qlo;                         // Range.compareIntersecting == 0
                    else if (v.end_inclusive) hit = s < qlo && qlo <= e;       // EndInclusive.contains (s, e]
                    else hit = s <= qlo && qlo < e;                            // StartInclusive.contains [s, e)
                } else {
                    const uint64_t s = T.s[k];
                    if (s > r.hi) break;
                    const uint64_t e = T.e[k];
                    if (isr) hit = s < r.hi && e > r.lo;
                    else if (v.end_inclusive) hit = s < r.lo && r.lo <= e;
                    else hit = s <= r.lo && r.lo < e;
                }
                if (!hit) continue;
                const uint2 info = T.info[k];
                if (info.y >= r.lim || info.y == r.tpos) continue;            // STARTED_BEFORE; p1
                if (!((wm >> T.kind[k]) & 1u)) continue;                      // testKind
                if (EMIT) {
                    const uint64_t x = ((uint64_t)info.x << 32) | info.y;
                    if (stage) stage[out + count] = x; else v.ent[out + count] = x;
                }
                ++count;
            }
        }
        __syncthreads();
        c = c2; base = base2;
    }
    return count;
}

// The stabbing blocks' windows: one thread per (block, width class) and bound, a plain binary search over the class's
// starts (starts in [lo_min - 4^c, hi_max] for the block's sorted queries). Thousands of independent searches keep the
// loads in flight, where a search inside the stabbing block would stall it for every dependent round.
__global__ __launch_bounds__(BLOCK) void k_rd_stab_win(uint32_t nsb, const uint64_t *__restrict__ blo,
                                                       const uint64_t *__restrict__ bhi, View v, uint32_t *__restrict__ win)
{
    const uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= (uint64_t)nsb * NCLS) return;
    const uint32_t blk = (uint32_t)(g / NCLS), c = (uint32_t)(g % NCLS);
    const uint32_t a0 = v.class_off[c], a1 = v.class_off[c + 1];
    uint32_t b0 = a0, b1 = a0;
    if (a1 > a0) {
        const uint64_t lo = blo[blk], hi = bhi[blk], W = class_width(c);
        b0 = lower_bound(v.cs_s, a0, a1, lo > W ? lo - W : 0);
        b1 = upper_bound(v.cs_s, b0, a1, hi);
    }
    win[(size_t)blk * 2 * NCLS + c] = b0;
    win[(size_t)blk * 2 * NCLS + NCLS + c] = b1;
}

// Every class's window of the block in one tile (when they fit TILE together): one load round for the block.
// Count pass (hv != null): the query's first STAB_RH hits are kept in registers. Emit pass: hits to ent at out.
// REL: bounds as 32-bit offsets above the block's rbase (half the LDS bytes per probe and per candidate: the pass is
// bound by LDS reads); a candidate's TxnId position and kind are read only when its bounds hit.
constexpr int STAB_RH = 16;   // hits a query keeps in registers through the count pass (flat blocks)

template <bool EMIT>
__device__ __forceinline__ uint32_t stab_flat_rel(const View &v, StabTile &T, bool valid, const QRec &r, uint64_t out,
                                                  uint64_t (*hv)[STAB_RH])
{
    uint32_t count = 0;
    if (!valid) return 0;
    const bool isr = (r.flags >> 8) & 1u;
    const uint32_t wm = r.flags & 0xFFu;
    const uint32_t qlo = (uint32_t)(r.lo - T.rbase), qhi = (uint32_t)(r.hi - T.rbase);
    for (uint32_t c = 0; c < (uint32_t)NCLS; ++c) {
        const uint32_t p0 = T.pre[c], p1 = T.pre[c + 1];
        if (p0 == p1) continue;
        const uint64_t W = class_width(c);
        const uint32_t qwlo = (uint64_t)qlo > W ? qlo - (uint32_t)W : 0u;
        for (uint32_t k = lower_bound(T.s32, p0, p1, qwlo); k < p1; ++k) {
            const uint32_t s = T.s32[k];
            if (s > qhi) break;
            const uint32_t e = T.e32[k];
            bool hit;
            if (isr) hit = s < qhi && e > qlo;                             // Range.compareIntersecting == 0
            else if (v.end_inclusive) hit = s < qlo && qlo <= e;           // EndInclusive.contains (s, e]
            else hit = s <= qlo && qlo < e;                                // StartInclusive.contains [s, e)
            if (hit) {
                const uint2 info = T.info[k];
                hit = info.y < r.lim && info.y != r.tpos                   // STARTED_BEFORE; p1
                      && ((wm >> T.kind[k]) & 1u);                         // testKind
                if (hit) {
                    const uint64_t x = ((uint64_t)info.x << 32) | info.y;
                    if (EMIT) {
                        v.ent[out + count] = x;
                    } else if (hv) {
#pragma unroll
                        for (int u = 0; u < STAB_RH; ++u)
                            if ((uint32_t)u == count) (*hv)[u] = x;
                    }
                    ++count;
                }
            }
        }
    }
    return count;
}

template <bool EMIT>
__device__ __forceinline__ uint32_t stab_flat(const View &v, StabTile &T, bool valid, const QRec &r, uint64_t out,
                                              uint64_t (*hv)[STAB_RH])
{
    uint32_t count = 0;
    if (!valid) return 0;
    const bool isr = (r.flags >> 8) & 1u;
    const uint32_t wm = r.flags & 0xFFu;
    for (uint32_t c = 0; c < (uint32_t)NCLS; ++c) {
        const uint32_t p0 = T.pre[c], p1 = T.pre[c + 1];
        if (p0 == p1) continue;
        const uint64_t W = class_width(c);
        const uint64_t qwlo = r.lo > W ? r.lo - W : 0;
        for (uint32_t k = lower_bound(T.s, p0, p1, qwlo); k < p1; ++k) {
            const uint64_t s = T.s[k];
            if (s > r.hi) break;
            const uint64_t e = T.e[k];
            bool hit;
            if (isr) hit = s < r.hi && e > r.lo;                           // Range.compareIntersecting == 0
            else if (v.end_inclusive) hit = s < r.lo && r.lo <= e;         // EndInclusive.contains (s, e]
            else hit = s <= r.lo && r.lo < e;                              // StartInclusive.contains [s, e)
            const uint2 info = T.info[k];
            hit = hit && info.y < r.lim && info.y != r.tpos                // STARTED_BEFORE; p1
                  && ((wm >> T.kind[k]) & 1u);                             // testKind
            const uint64_t x = ((uint64_t)info.x << 32) | info.y;
            if (EMIT) {
                if (hit) v.ent[out + count] = x;
            } else if (hv) {
#pragma unroll
                for (int u = 0; u < STAB_RH; ++u)
                    if (hit && (uint32_t)u == count) (*hv)[u] = x;
            }
            count += hit ? 1u : 0u;
        }
    }
    return count;
}

#ifdef ACC_PHASE_PROF
// tuning build only: per-block phase cycles of k_rd_stab (thread 0, each phase closed by a barrier and a full waitcnt)
__device__ unsigned long long *g_stab_prof;
#define SB_PH(i) do { __syncthreads(); __builtin_amdgcn_s_waitcnt(0); ph[i] = clock64(); } while (0)
#else
#define SB_PH(i) ((void)0)
#endif

// A workgroup of BLOCK consecutive (sorted) queries over its precomputed windows: count every query's pairs, take the
// block's output slice with one atomic, write them. When the windows fit one tile they are loaded once and each query
// keeps its first STAB_RH hits in registers through the count pass: a query with no more than that writes them from
// there, a query with more scans the tile again. Otherwise the (class, tile) sequence is scanned again to emit.
// (A config-4 key block holds ~1,400 hits: an LDS pool of them would cost the occupancy, a per-hit slot claim the
// count pass's time.)
__global__ __launch_bounds__(BLOCK) void k_rd_stab(View v)
{
#ifdef ACC_PHASE_PROF
    uint64_t ph[6];
#endif
    SB_PH(0);
    __shared__ StabTile T;
    const uint32_t tid = threadIdx.x;
    const uint32_t i = blockIdx.x * BLOCK + tid;
    QRec r{};
    if (i < v.Q) r = v.srec[i];
    const bool valid = i < v.Q && !(r.flags & QPAD);
    if (tid < (uint32_t)NCLS) {
        T.b0[tid] = v.win[(size_t)blockIdx.x * 2 * NCLS + tid];
        T.b1[tid] = v.win[(size_t)blockIdx.x * 2 * NCLS + NCLS + tid];
    }
    __syncthreads();
    if (tid < 64) {   // wave 0: the classes' tile offsets by one wave scan (a serial loop over 33 classes cost ~3K cycles)
        const uint32_t len = tid < (uint32_t)NCLS ? T.b1[tid] - T.b0[tid] : 0u;
        const uint32_t incl = wave_inclusive(len, OpAdd<uint32_t>());
        if (tid < (uint32_t)NCLS) T.pre[tid] = incl - len;
        if (tid == (uint32_t)NCLS - 1) T.pre[NCLS] = incl;
        const uint64_t ne = __ballot(len != 0);
        if (tid == 0) {
            const uint32_t cmax = ne ? 63u - (uint32_t)__builtin_clzll(ne) : 0u;
            // every windowed start is at least the block's lowest bound less its widest class; the highest probe
            // bound is bhi
            const uint64_t W = class_width(cmax), lo = v.blo[blockIdx.x], hi = v.bhi[blockIdx.x];
            T.rbase = lo > W ? lo - W : 0;
            T.rel = hi >= T.rbase && hi - T.rbase < 0xFFFFFFFFull;
        }
    }
    __syncthreads();
    SB_PH(1);
    const uint32_t wtot = T.pre[NCLS];
    const bool flat = wtot <= (uint32_t)TILE;
    uint32_t count;
    uint64_t hv[STAB_RH];
    if (flat) {
        for (uint32_t k = tid; k < wtot; k += BLOCK) {
            const uint32_t lo = seg_of(T.pre, NCLS, k);   // the class holding flat position k: last c with pre[c] <= k
            const uint32_t src = T.b0[lo] + (k - T.pre[lo]);
            const uint64_t cs = v.cs_s[src], ce = v.cs_e[src];
            T.s[k] = cs; T.e[k] = ce; T.info[k] = v.cs_info[src]; T.kind[k] = v.cs_kind[src];
            T.s32[k] = (uint32_t)(cs - T.rbase);
            T.e32[k] = ce - T.rbase < 0xFFFFFFFFull ? (uint32_t)(ce - T.rbase) : 0xFFFFFFFFu;
        }
        __syncthreads();
        SB_PH(2);
        count = T.rel ? stab_flat_rel<false>(v, T, valid, r, 0, &hv) : stab_flat<false>(v, T, valid, r, 0, &hv);
    } else {
        SB_PH(2);
        count = T.rel ? stab_pass<false, true>(v, T, valid, r, 0, nullptr) : stab_pass<false, false>(v, T, valid, r, 0, nullptr);
    }
    SB_PH(3);
    uint32_t total;
    const uint32_t mine = block_exclusive(count, OpAdd<uint32_t>(), T.red, total);
    if (tid == 0) T.base = atomicAdd((unsigned long long *)v.cursor, (unsigned long long)total);
    __syncthreads();
    SB_PH(4);
    const uint64_t base = T.base;
    if (valid) v.q_out[r.q] = make_ulonglong2(base + mine, count);
    if (base + total > v.cap) return;   // uniform: the host re-runs with a larger capacity
    if (flat && count <= (uint32_t)STAB_RH) {
#pragma unroll
        for (int u = 0; u < STAB_RH; ++u)
            if ((uint32_t)u < count) v.ent[base + mine + u] = hv[u];
    } else if (flat) {
        if (T.rel) stab_flat_rel<true>(v, T, valid, r, base + mine, nullptr);
        else stab_flat<true>(v, T, valid, r, base + mine, nullptr);
    } else {
        if (T.rel) stab_pass<true, true>(v, T, valid, r, base + mine, nullptr);
        else stab_pass<true, false>(v, T, valid, r, base + mine, nullptr);
    }
#ifdef ACC_PHASE_PROF
    SB_PH(5);
    if (tid == 0) {
        unsigned long long *row = g_stab_prof + 8 * (size_t)blockIdx.x;
        for (int k = 0; k < 5; ++k) row[k] = ph[k + 1] - ph[k];
        row[6] = flat ? 1 : 2;
        row[5] = total;
        row[7] = 1;
    }
#endif
}

}  // namespace rd

using namespace rd;

#ifdef ACC_PHASE_PROF
// tuning build: the phase rows of one k_rd_stab launch of nsb workgroups (stab_prof_arm before it, the print after)
static unsigned long long *stab_prof_arm(acc_ctx *ctx, uint32_t nsb)
{
    return prof_arm(ctx, "stab_prof", HIP_SYMBOL(g_stab_prof), 8 * (size_t)nsb, ctx->stream);
}
static void stab_prof_print(acc_ctx *ctx, unsigned long long *buf, uint32_t nsb)
{
    const std::vector<unsigned long long> h = prof_read(buf, 8 * (size_t)nsb, ctx->stream);
    for (int f = 1; f <= 2; ++f) {
        double sum[6] = {};
        size_t nb = 0;
        for (size_t b = 0; b < nsb; ++b) {
            if (!h[8 * b + 7] || h[8 * b + 6] != (unsigned long long)f) continue;
            ++nb;
            for (int k = 0; k < 6; ++k) sum[k] += (double)h[8 * b + k];
        }
        const double d = nb ? (double)nb : 1.0;
        fprintf(stderr, "[stab_phase] %s blocks=%zu avg cycles: head %.0f tile %.0f count %.0f scan+claim %.0f write %.0f | hits %.0f\n",
                f == 1 ? "flat" : "tiled", nb, sum[0] / d, sum[1] / d, sum[2] / d, sum[3] / d, sum[4] / d, sum[5] / d);
    }
}
#endif

// ---- 3. query records sorted by low bound; stabbing (one pass, block-sliced output)
void rd_stab_queries(acc_ctx *ctx, RdBuild &b)
{
    hipStream_t st = ctx->stream;
    const size_t P = b.P, R = b.R;
    const uint32_t Q = b.Q;
    const Runs q_plan = make_runs(b.mask_lo);
    ctx->stat("rangedeps.query_bits", (uint64_t)q_plan.bits);
    QRec *rec = ctx->get<QRec>("rd_qrec", Q), *srec = nullptr;
    uint64_t *qkey = ctx->get<uint64_t>("rd_qkey", Q);
    const int qbits_full = q_plan.bits < 62 ? q_plan.bits + 3 : q_plan.bits < 64 ? q_plan.bits + 1 : 64;
    // Only the high bits of the low bound are sorted: a stabbing block needs BLOCK queries with neighbouring low bounds
    // (its windows span their lowest to highest bound), and each query's scan is independent of its place in the block.
    // 2^(bits_for(Q) - 2) buckets hold ~4 queries each on spread keys, so a block spans ~64 buckets — about the span of
    // an exact sort — in whole 8-bit passes (config 4: 3 passes instead of 5).
    const int qsort_bits = std::min(qbits_full, std::max(8, (bits_for(Q) - 2 + 7) / 8 * 8));
    const int qdrop = qbits_full - qsort_bits;
    const int qbits = qsort_bits;
    const int ibits = qbits + bits_for(Q) <= 64 && Q < OS_VAL ? std::max(1, bits_for(Q)) : 0;
    launch(ctx, "rd_qrec", k_rd_qrec, dim3(grid_for(Q, BLOCK)), dim3(BLOCK), 0, (uint32_t)P, (uint32_t)R, b.key_code,
           (const uint32_t *)b.owner, b.rs, b.re, (const uint32_t *)b.rowner, (const uint4 *)b.tinfo, q_plan, rec, qkey,
           (uint32_t)q_plan.bits, ibits, qdrop);
    Sorted qs{ nullptr, nullptr };
    const uint64_t *qpk = nullptr;
    if (ibits) qpk = radix_sort_keys(ctx, "rs_rd_q", qkey, Q, ibits, qbits);
    else qs = radix_sort(ctx, "rs_rd_q", qkey, nullptr, Q, qbits);
    const uint32_t Pp = q_plan.bits < 64 && P && R ? (uint32_t)((P + BLOCK - 1) / BLOCK * BLOCK) : (uint32_t)P;
    // the range queries' width groups (q_plan.bits < 62) each from a block boundary: their sizes stay on the device, so
    // the padded length is bounded (three more gaps of under a block)
    const int wgroups = q_plan.bits < 62 && R ? 1 : 0;
    const uint32_t Qp = Q + (Pp - (uint32_t)P) + (wgroups ? 3u * BLOCK : 0u);
    uint32_t *qbnd = ctx->get<uint32_t>("rd_qbnd", 8);
    launch(ctx, "rd_qgroups", k_rd_qgroups, dim3(1), dim3(64), 0, ibits ? qpk : (const uint64_t *)qs.keys, (uint32_t)P, Q,
           ibits + qbits - 3, wgroups, qbnd);
    const uint32_t nsb = (uint32_t)grid_for(Qp, BLOCK);
    uint64_t *bhi = ctx->get<uint64_t>("rd_bhi", nsb), *blo = ctx->get<uint64_t>("rd_blo", nsb);
    srec = ctx->get<QRec>("rd_qrec_sorted", Qp);
    launch(ctx, "rd_qsort", k_rd_qsort, dim3(nsb), dim3(BLOCK), 0, Qp, (uint32_t)P, Pp, (const uint32_t *)qbnd,
           (const uint32_t *)qs.vals, qpk,
           ibits ? (1ull << ibits) - 1 : 0ull, (const QRec *)rec, srec, blo, bhi);
    View &v = b.v;
    v.Q = Qp; v.end_inclusive = b.end_inclusive; v.srec = srec;
    v.cs_s = b.cs_s; v.cs_e = b.cs_e; v.cs_info = b.cs_info; v.cs_kind = b.cs_kind; v.class_off = b.class_off;
    v.q_out = ctx->get<ulonglong2>("rd_q_out", Q);
    v.cursor = ctx->get<uint64_t>("rd_cursor", 1);
    uint32_t *win = ctx->get<uint32_t>("rd_win", (size_t)nsb * 2 * NCLS);
    v.win = win;
    v.blo = blo; v.bhi = bhi;
    if (!Q) {
        v.ent = ctx->get<uint64_t>("rd_ent", 0);
        return;
    }
    launch(ctx, "rd_stab_win", k_rd_stab_win, dim3(grid_for((uint64_t)nsb * NCLS, BLOCK)), dim3(BLOCK), 0, nsb,
           (const uint64_t *)blo, (const uint64_t *)bhi, v, win);
    for (int attempt = 0; attempt < 2; ++attempt) {
        // capacity: the last batch's need on this context, at least 16 per query
        const uint64_t want = std::max<uint64_t>(ctx->rd_ent_hint, 16ull * Q + 1024);
        v.ent = ctx->get<uint64_t>("rd_ent", want);
        v.cap = ctx->bufs["rd_ent"].bytes / sizeof(uint64_t);
        ACC_HIP(hipMemsetAsync(v.cursor, 0, 8, st));
#ifdef ACC_PHASE_PROF
        unsigned long long *sbp = stab_prof_arm(ctx, nsb);
#endif
        launch(ctx, "rd_stab", k_rd_stab, dim3(nsb), dim3(BLOCK), 0, v);
#ifdef ACC_PHASE_PROF
        stab_prof_print(ctx, sbp, nsb);
#endif
        ReadBack rb(ctx);
        const auto total = rb.u64(v.cursor);
        rb.wait();
        b.E = total;
        b.stab_passes = (uint32_t)attempt + 1;
        ctx->rd_ent_hint = std::max(ctx->rd_ent_hint, b.E);
        if (b.E <= v.cap) break;
        if (attempt == 1) fail(ACC_E_STATE, "internal: range-deps output grew between passes");
    }
}

}  // namespace acc
