// rangedeps_build.hip — stage 4 of RangeDeps (rangedeps.hip has the pipeline): per txn, the stabbing pass's raw
// (range id, TxnId position) pairs sorted, deduplicated and indexed into scratch by a tier of the txn's size, then
// compacted into the Java-layout CSR.

#include "rangedeps.hpp"
#include "search.hpp"

namespace acc {

namespace rd {

// ---------------------------------------------------------------- per-txn build

__device__ __forceinline__ void txn_queries(const Out &o, uint32_t t, uint32_t &q0, uint32_t &q1)
{
    const uint32_t k0 = o.key_off[t], k1 = o.key_off[t + 1];
    if (k1 > k0) { q0 = k0; q1 = k1; return; }
    q0 = o.P + o.rng_off[t];
    q1 = o.P + o.rng_off[t + 1];
}

__device__ __forceinline__ uint32_t dep_of(const Out &o, uint32_t tpos) { return o.txn_of_tpos ? o.txn_of_tpos[tpos] : tpos; }

// per txn: raw entry count and tier; the tier counts of the batch (hist, zeroed before): one ballot per tier value and
// wave, summed over RD_TS chunks of BLOCK txns per workgroup, one global add per tier and workgroup (the 12 counters
// share one line: per-256-txn adds serialised there, and per-thread LDS atomics on 12 words before that)
constexpr int RD_TIERS = 12;
__global__ __launch_bounds__(BLOCK) void k_rd_tsize(uint32_t n, Out o, uint64_t *__restrict__ m_raw, uint32_t *__restrict__ tier,
                                                    uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[WAVES][RD_TIERS];
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    uint32_t acc[RD_TIERS] = {};   // this wave's counts (lane 0)
    for (int r = 0; r < RD_TS; ++r) {
        const uint32_t t = (blockIdx.x * RD_TS + (uint32_t)r) * BLOCK + threadIdx.x;
        uint32_t tr = 0xFFu;
        if (t < n) {
            uint32_t q0, q1;
            txn_queries(o, t, q0, q1);
            uint64_t m = 0;
            for (uint32_t qb = q0; qb < q1; qb += 8) {   // eight count loads in flight, not one dependent add per load
                uint32_t c[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) c[u] = qb + u < q1 ? (uint32_t)o.q_out[qb + u].y : 0u;
#pragma unroll
                for (int u = 0; u < 8; ++u) m += c[u];
            }
            m_raw[t] = m;
            // tiers: 0 none, 1 <= 16 (16-lane groups), 11 <= 32 (half waves), 2 <= 64 (wave), 3..9 LDS workgroups of
            // 128..8192, 10 global
            if (m == 0) tr = 0;
            else if (m <= 16) tr = 1;
            else if (m <= 32) tr = 11;
            else if (m <= 64) tr = 2;
            else if (m <= BLOCK_E) { uint32_t n2 = 128, b = 3; while (n2 < m) { n2 <<= 1; ++b; } tr = b; }
            else tr = 10;
            tier[t] = tr;
            if (m == 0) { o.rd_cnt[t] = 0; o.u_cnt[t] = 0; o.a_cnt[t] = 0; }
        }
#pragma unroll
        for (int v = 0; v < RD_TIERS; ++v) acc[v] += (uint32_t)__popcll(__ballot(tr == (uint32_t)v));
    }
    if (lane == 0)
#pragma unroll
        for (int v = 0; v < RD_TIERS; ++v) h[w][v] = acc[v];
    __syncthreads();
    if (threadIdx.x < RD_TIERS) {
        uint32_t c = 0;
        for (int q = 0; q < WAVES; ++q) c += h[q][threadIdx.x];
        if (c) atomicAdd(&hist[threadIdx.x], c);
    }
}


// bitonic sort within lane groups of S (lane-aligned: the xor partners stay inside), ascending; partners through DPP /
// permlane swaps (xor_lanes: the whole wave active, as at every call below)
template <int S, class T>
__device__ __forceinline__ T group_sort(T x, uint32_t lane)
{
#pragma unroll
    for (uint32_t k = 2; k <= (uint32_t)S; k <<= 1) {
#pragma unroll
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            const T y = xor_lanes(x, (int)jj);
            const bool up = k == (uint32_t)S || (lane & k) == 0, lower = (lane & jj) == 0;
            const T mn = x < y ? x : y, mx = x < y ? y : x;
            x = (lower == up) ? mn : mx;
        }
    }
    return x;
}

// One chunk of S queries [qc, min(qc + S, q1)) of a txn whose (first entry, entries) records the group's lanes hold
// in qv: an inclusive count scan, a shuffle search for the query holding entry `sub` of the txn (after the m entries
// of earlier chunks), and that entry's load (issued here, waited for by the first use).
template <int S>
__device__ __forceinline__ void seg_chunk(const Out &o, ulonglong2 qv, uint32_t sub, int gb, uint64_t &m, uint64_t &x)
{
    const uint32_t c = (uint32_t)qv.y;
    const uint64_t qo = qv.x;
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < S; d <<= 1) {
        const uint32_t u = __shfl_up(incl, d, 64);
        if (sub >= (uint32_t)d) incl += u;
    }
    const uint32_t total = __shfl(incl, gb + S - 1, 64);
    uint32_t j = 0;   // lanes whose queries end at or before entry sub
#pragma unroll
    for (int step = S / 2; step >= 1; step >>= 1) {
        const uint32_t end = (uint32_t)m + __shfl(incl, gb + (int)j + step - 1, 64);
        if (end <= sub) j += step;
    }
    j = min(j, (uint32_t)S - 1);
    const uint64_t qoj = shfl_idx(qo, gb + (int)j);
    const uint32_t startj = (uint32_t)m + __shfl(incl - c, gb + (int)j, 64);
    if (sub >= m && sub < m + total) x = o.ent[qoj + (sub - startj)];
    m += total;
}

// Groups of S lanes (S = 16, 32 or 64), K txns each in turn: load, sort (range id, TxnId position), dedupe, TxnId
// union and index, range groups; results to the scratch regions of the txn.
// The K txns' loads are issued together — list entries, then their offsets, then their first S query records, then
// their entries — so a group waits for four dependent memory latencies per K txns, not per txn (the tier is
// latency-bound: each of those loads costs ~2.5K cycles under the build's load, the sorts ~1K).
// NARROW (range ids and TxnId positions below 2^26): both sorts on 32-bit keys, half the cross-lane traffic of the
// 64-bit network. The first sorts (range id << 6 | lane) and each lane then takes its key's entry; when some range id is
// held by entries of different TxnIds (commands with identical ranges: rare) the (range id, lane) order may separate
// duplicates or misorder TxnIds, so that wave sorts the 64-bit entries instead.
#ifdef ACC_PHASE_PROF
// tuning build only (tools/build_prof.sh): per-wave phase cycles of k_rd_build_seg, one row of 8 per wave, each phase
// closed by a full s_waitcnt so a phase owns its loads' latency
__device__ unsigned long long *g_rd_prof;
#define RD_PH(i) do { __builtin_amdgcn_s_waitcnt(0); ph[i] = clock64(); } while (0)
#else
#define RD_PH(i) ((void)0)
#endif
#ifndef ACC_RD_SEGK
#define ACC_RD_SEGK 4
#endif
constexpr int RD_SEGK = ACC_RD_SEGK;   // txns per lane group

template <int S, bool NARROW, int K>
__global__ __launch_bounds__(BLOCK) void k_rd_build_seg(uint32_t cnt, Out o)
{
#ifdef ACC_PHASE_PROF
    uint64_t ph[6];
#endif
    RD_PH(0);
    __shared__ uint32_t slot[WAVES][64];
    constexpr int G = 64 / S;
    const uint32_t wave = threadIdx.x >> 6, lane = lane_id();
    const uint32_t grp = lane / S, sub = lane & (S - 1);
    const uint32_t li0 = ((blockIdx.x * WAVES + wave) * G + grp) * K;
    const uint64_t gmask = S == 64 ? ~0ull : (((1ull << (S & 63)) - 1) << (grp * S));
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int gb = (int)(grp * S);
    const uint32_t g0 = grp * S;
    uint32_t t[K], q0[K], q1[K];
    uint64_t ra[K], m[K], x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = li0 + k < cnt ? o.list[li0 + k] : 0u;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        // both the key and the range bounds (txn_queries' choice made after the loads, not between them)
        q0[k] = q1[k] = 0; ra[k] = 0;
        if (li0 + k < cnt) {
            const uint32_t k0 = o.key_off[t[k]], k1 = o.key_off[t[k] + 1];
            const uint32_t r0 = o.rng_off[t[k]], r1 = o.rng_off[t[k] + 1];
            ra[k] = o.raw_off[t[k]];
            if (k1 > k0) { q0[k] = k0; q1[k] = k1; } else { q0[k] = o.P + r0; q1[k] = o.P + r1; }
        }
    }
    RD_PH(1);
    ulonglong2 qv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t q = q0[k] + sub;
        qv[k] = make_ulonglong2(0, 0);
        if (q < q1[k]) qv[k] = o.q_out[q];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        m[k] = 0; x[k] = ~0ull;
        seg_chunk<S>(o, qv[k], sub, gb, m[k], x[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        for (uint32_t qc = q0[k] + S; qc < q1[k]; qc += S) {   // group-uniform: txns of more than S queries
            const uint32_t q = qc + sub;
            ulonglong2 v = make_ulonglong2(0, 0);
            if (q < q1[k]) v = o.q_out[q];
            seg_chunk<S>(o, v, sub, gb, m[k], x[k]);
        }
    }
    RD_PH(2);
#ifdef ACC_PHASE_PROF
    uint64_t sort_cy = 0, write_cy = 0;
    bool wlive = false;
#endif
#pragma unroll
    for (int k = 0; k < K; ++k) {
#ifdef ACC_PHASE_PROF
        RD_PH(3);
#endif
        const bool live = li0 + k < cnt;
        uint64_t xk = x[k];
        const uint64_t mk = m[k];
        if (NARROW) {
            uint32_t k1 = (live && sub < mk) ? ((uint32_t)(xk >> 32) << 6) | sub : 0xFFFFFFFFu;
            k1 = group_sort<S>(k1, lane);
            const uint64_t xs = shfl_idx(xk, (int)(grp * S + (k1 & 63u)));
            xk = k1 == 0xFFFFFFFFu ? ~0ull : xs;
            const uint64_t pv = shfl_up(xk, 1);
            const bool mixed = live && sub > 0 && sub < mk && (uint32_t)(pv >> 32) == (uint32_t)(xk >> 32) && (uint32_t)pv != (uint32_t)xk;
            if (__ballot(mixed)) xk = group_sort<S>(xk, lane);   // wave-uniform; sorted groups stay as they are
        } else {
            xk = group_sort<S>(xk, lane);
        }
        const uint64_t prev = shfl_up(xk, 1);
        const bool valid = live && sub < mk && (sub == 0 || xk != prev);       // dedupe identical (range, txn)
        const uint64_t vb = __ballot(valid) & gmask;
        const uint32_t M = (uint32_t)__popcll(vb);
        const uint32_t pos = (uint32_t)__popcll(vb & lt);
        const uint32_t rid = (uint32_t)(xk >> 32), tp = (uint32_t)xk;
        // (TxnId position, entry) sorted: the TxnId union and each entry's index
        uint32_t ytp, ypos;
        if (NARROW) {
            const uint32_t y = group_sort<S>(valid ? (tp << 6) | pos : 0xFFFFFFFFu, lane);
            ytp = y >> 6; ypos = y & 63u;
        } else {
            const uint64_t y = group_sort<S>(valid ? (((uint64_t)tp << 8) | pos) : ~0ull, lane);
            ytp = (uint32_t)(y >> 8); ypos = (uint32_t)y & 0xFFu;
        }
        const uint32_t yprev = __shfl_up(ytp, 1, 64);
        const bool ynew = live && sub < M && (sub == 0 || ytp != yprev);
        const uint64_t nb = __ballot(ynew) & gmask;
        const uint32_t U = (uint32_t)__popcll(nb);
        const bool yin = live && sub < M;
        const uint32_t uidx = (uint32_t)__popcll(nb & lt) + (ynew ? 1u : 0u) - 1u;   // index of this entry's TxnId
        const bool rnew = valid && (sub == 0 || (uint32_t)(prev >> 32) != rid);
        const uint64_t rb = __ballot(rnew) & gmask;
        const uint32_t Rd = (uint32_t)__popcll(rb);
#ifdef ACC_PHASE_PROF
        RD_PH(4);
        sort_cy += ph[4] - ph[3];
        wlive = wlive || __ballot(live && mk != 0) != 0;
#endif
        __builtin_amdgcn_wave_barrier();   // the previous txn's reads of slot are done
        if (yin) slot[wave][g0 + ypos] = uidx;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        if (live && mk != 0) {
            uint32_t *sa = o.s_arena + 2 * ra[k], *sr = o.s_rid + ra[k], *sd = o.s_dep + ra[k];
            if (ynew) sd[uidx] = dep_of(o, ytp);
            const uint32_t g = (uint32_t)__popcll(rb & lt);
            if (valid) {
                sa[Rd + pos] = slot[wave][g0 + pos];
                if (rnew) {
                    sr[g] = rid;
                    if (g > 0) sa[g - 1] = Rd + pos;
                }
            }
            if (sub == 0) {
                sa[Rd - 1] = Rd + M;
                o.rd_cnt[t[k]] = Rd; o.u_cnt[t[k]] = U; o.a_cnt[t[k]] = (uint64_t)Rd + M;
            }
        }
#ifdef ACC_PHASE_PROF
        RD_PH(5);
        write_cy += ph[5] - ph[4];
#endif
    }
#ifdef ACC_PHASE_PROF
    if (lane == 0 && wlive) {
        unsigned long long *row = g_rd_prof + 8 * ((size_t)blockIdx.x * WAVES + wave);
        row[0] = ph[1] - ph[0]; row[1] = ph[2] - ph[1]; row[2] = sort_cy; row[3] = write_cy;
        row[7] = 1;
    }
#endif
}

// One workgroup per txn over buffers A, B of n2 >= m elements (LDS sized to the tier, or global scratch)
// qs / qo: LDS of BLOCK + 1 / BLOCK entries (query starts in the txn's raw list, query offsets in ent)
__device__ void build_block(const Out &o, uint32_t t, uint64_t *A, uint64_t *B, uint32_t *red, uint32_t *qs, uint64_t *qo)
{
    const uint32_t tid = threadIdx.x;
    uint32_t q0, q1;
    txn_queries(o, t, q0, q1);
    uint32_t m = 0;
    const uint32_t nq = q1 - q0;
    if (nq <= (uint32_t)BLOCK) {
        // every query's count and offset in one load round, then the raw entries four loads per thread at a time
        uint32_t c = 0;
        uint64_t off = 0;
        if (tid < nq) { const ulonglong2 qv = o.q_out[q0 + tid]; c = (uint32_t)qv.y; off = qv.x; }
        const uint32_t st = block_exclusive(c, OpAdd<uint32_t>(), red, m);
        if (tid < nq) { qs[tid] = st; qo[tid] = off; }
        __syncthreads();
        for (uint32_t k0 = tid; k0 < m; k0 += 4 * BLOCK) {
            uint64_t x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t k = k0 + (uint32_t)u * BLOCK;
                x[u] = 0;
                if (k < m) {
                    const uint32_t lo = seg_of(qs, nq, k);   // last query starting at or before k
                    x[u] = o.ent[qo[lo] + (k - qs[lo])];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) if (k0 + (uint32_t)u * BLOCK < m) A[k0 + (uint32_t)u * BLOCK] = x[u];
        }
    } else {
        for (uint32_t q = q0; q < q1; ++q) {
            const ulonglong2 qv = o.q_out[q];
            const uint32_t c = (uint32_t)qv.y;
            const uint64_t off = qv.x;
            for (uint32_t k = tid; k < c; k += BLOCK) A[m + k] = o.ent[off + k];
            m += c;
        }
    }
    uint32_t n2 = 64;
    while (n2 < m) n2 <<= 1;
    for (uint32_t i = m + tid; i < n2; i += BLOCK) A[i] = ~0ull;
    __syncthreads();
    block_bitonic(A, n2);
    // dedupe + compact into B; each thread owns a contiguous slice
    const uint32_t per = (n2 + BLOCK - 1) / BLOCK;
    const uint32_t lo = tid * per, hi = min(lo + per, n2);
    uint32_t c = 0;
    for (uint32_t i = lo; i < hi; ++i) c += (i < m && (i == 0 || A[i] != A[i - 1])) ? 1u : 0u;
    uint32_t M;
    uint32_t p = block_exclusive(c, OpAdd<uint32_t>(), red, M);
    for (uint32_t i = lo; i < hi; ++i)
        if (i < m && (i == 0 || A[i] != A[i - 1])) B[p++] = A[i];
    __syncthreads();
    uint32_t n2m = 64;
    while (n2m < M) n2m <<= 1;
    for (uint32_t i = tid; i < n2m; i += BLOCK) A[i] = i < M ? (((uint64_t)(uint32_t)B[i] << 32) | i) : ~0ull;
    __syncthreads();
    block_bitonic(A, n2m);
    // distinct TxnId positions -> index; B[e] becomes (range id << 32 | index)
    const uint64_t ra = o.raw_off[t];
    uint32_t *sa = o.s_arena + 2 * ra, *sr = o.s_rid + ra, *sd = o.s_dep + ra;
    const uint32_t per2 = (n2m + BLOCK - 1) / BLOCK;
    const uint32_t lo2 = tid * per2, hi2 = min(lo2 + per2, n2m);
    c = 0;
    for (uint32_t i = lo2; i < hi2; ++i) c += (i < M && (i == 0 || (A[i] >> 32) != (A[i - 1] >> 32))) ? 1u : 0u;
    uint32_t U;
    uint32_t u = block_exclusive(c, OpAdd<uint32_t>(), red, U);
    for (uint32_t i = lo2; i < hi2; ++i) {
        if (i >= M) break;
        const bool nw = i == 0 || (A[i] >> 32) != (A[i - 1] >> 32);
        if (nw) { sd[u] = dep_of(o, (uint32_t)(A[i] >> 32)); ++u; }
        const uint32_t e = (uint32_t)A[i];
        B[e] = (B[e] & 0xFFFFFFFF00000000ull) | (u - 1);
    }
    __syncthreads();
    // range groups over B[0, M)
    const uint32_t per3 = (M + BLOCK - 1) / BLOCK;
    const uint32_t lo3 = min(tid * per3, M), hi3 = min(lo3 + per3, M);
    c = 0;
    for (uint32_t e = lo3; e < hi3; ++e) c += (e == 0 || (B[e] >> 32) != (B[e - 1] >> 32)) ? 1u : 0u;
    uint32_t Rd;
    uint32_t g = block_exclusive(c, OpAdd<uint32_t>(), red, Rd);
    for (uint32_t e = lo3; e < hi3; ++e) {
        const uint32_t rid = (uint32_t)(B[e] >> 32);
        const bool nw = e == 0 || (B[e - 1] >> 32) != rid;
        if (nw) { sr[g] = rid; ++g; }
        sa[Rd + e] = (uint32_t)B[e];
        const bool last = e + 1 == M || (uint32_t)(B[e + 1] >> 32) != rid;
        if (last) sa[g - 1] = Rd + e + 1;
    }
    if (tid == 0) { o.rd_cnt[t] = Rd; o.u_cnt[t] = U; o.a_cnt[t] = (uint64_t)Rd + M; }
}

__global__ __launch_bounds__(BLOCK) void k_rd_build_block(Out o, uint32_t n2)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    // all LDS dynamic (no static __shared__ ahead of it: the base stays 16-B aligned, Guideline 17):
    // [A: n2 u64][B: n2 u64][qo: BLOCK u64][red: 16 u32][qs: BLOCK + 1 u32]
    uint64_t *qo = lds + 2 * n2;
    uint32_t *red = reinterpret_cast<uint32_t *>(qo + BLOCK);
    build_block(o, o.list[blockIdx.x], lds, lds + n2, red, red + 16, qo);
}

__global__ __launch_bounds__(BLOCK) void k_rd_build_global(Out o)
{
    __shared__ uint32_t red[WAVES];
    __shared__ uint32_t qs[BLOCK + 1];
    __shared__ uint64_t qo[BLOCK];
    const uint32_t t = o.list[blockIdx.x];
    uint64_t *A = o.gscratch + o.glb_off[blockIdx.x];
    const uint64_t m = o.raw_off[t + 1] - o.raw_off[t];
    uint64_t n2 = 64;
    while (n2 < m) n2 <<= 1;
    build_block(o, t, A, A + n2, red, qs, qo);
}

__global__ __launch_bounds__(BLOCK) void k_rd_glb_sizes(uint32_t ng, Out o, uint64_t *__restrict__ sz)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ng) return;
    const uint32_t t = o.list[i];
    const uint64_t m = o.raw_off[t + 1] - o.raw_off[t];
    uint64_t n2 = 64;
    while (n2 < m) n2 <<= 1;
    sz[i] = 2 * n2;
}

// scratch -> Java-layout CSR. A workgroup owns BLOCK consecutive txns, whose output runs are one contiguous range of
// each output array, copied in chunks of CP_CHUNK elements: each txn whose run starts inside the chunk marks its start
// in an LDS owner map (LDS max: of the txns starting at one position the last, the only non-empty one, wins), a block
// max-scan spreads the owners over the chunk (CP_PT consecutive positions per thread, written back to the map), and the
// block copies the chunk element-interleaved from the txns' scratch: every store instruction writes whole lines and no
// element searches for its txn.
constexpr int CP_PT = 8;
constexpr int CP_CHUNK = CP_PT * BLOCK;

__device__ __forceinline__ void compact_array(uint32_t nt, const uint64_t *off, const uint64_t *src_base,
                                              const uint32_t *__restrict__ src, uint32_t *__restrict__ dst,
                                              uint32_t *own, uint32_t *red)
{
    const uint32_t tid = threadIdx.x;
    const uint64_t j1 = off[nt];
    uint32_t carry = 0;
    for (uint64_t c0 = off[0]; c0 < j1; c0 += CP_CHUNK) {
        chunk_owners<CP_PT>(nt, off, c0, own, red, carry);
        // copies interleaved across the block (element u * BLOCK + tid): each store instruction writes whole lines
        uint32_t x[CP_PT];
#pragma unroll
        for (int u = 0; u < CP_PT; ++u) {
            const uint32_t p = (uint32_t)u * BLOCK + tid;
            const uint64_t j = c0 + p;
            const uint32_t k = own[p];
            x[u] = j < j1 ? src[src_base[k] + (j - off[k])] : 0u;
        }
#pragma unroll
        for (int u = 0; u < CP_PT; ++u) {
            const uint64_t j = c0 + (uint64_t)u * BLOCK + tid;
            if (j < j1) dst[j] = x[u];
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_rd_compact(uint32_t n, Out o)
{
    __shared__ uint64_t ao[BLOCK + 1], ro[BLOCK + 1], uo[BLOCK + 1], sa[BLOCK], sr[BLOCK];
    __shared__ uint32_t own[CP_CHUNK], red[WAVES];
    const uint32_t t0 = blockIdx.x * BLOCK, nt = min((uint32_t)BLOCK, n - t0), tid = threadIdx.x;
    if (tid < nt) {
        const uint32_t t = t0 + tid;
        ao[tid] = o.arena_off[t]; ro[tid] = o.rd_off[t]; uo[tid] = o.u_off[t];
        const uint64_t ra = o.raw_off[t];
        sa[tid] = 2 * ra; sr[tid] = ra;
    }
    if (tid == 0) { ao[nt] = o.arena_off[t0 + nt]; ro[nt] = o.rd_off[t0 + nt]; uo[nt] = o.u_off[t0 + nt]; }   // the block's ends
    __syncthreads();
    compact_array(nt, ao, sa, o.s_arena, reinterpret_cast<uint32_t *>(o.arena), own, red);
    compact_array(nt, ro, sr, o.s_rid, o.range_id, own, red);
    compact_array(nt, uo, sr, o.s_dep, o.dep_txn, own, red);
}

}  // namespace rd

using namespace rd;

#ifdef ACC_PHASE_PROF
// tuning build: rows for one k_rd_build_seg launch of `blocks` workgroups; rd_prof_print after it (serialises the tier)
static unsigned long long *rd_prof_arm(acc_ctx *ctx, uint32_t blocks)
{
    return prof_arm(ctx, "rd_prof", HIP_SYMBOL(g_rd_prof), 8 * (size_t)blocks * WAVES, ctx->stream);
}
static void rd_prof_print(acc_ctx *ctx, const char *tier, unsigned long long *buf, uint32_t blocks)
{
    const size_t rows = (size_t)blocks * WAVES;
    const std::vector<unsigned long long> h = prof_read(buf, 8 * rows, ctx->stream);
    double sum[4] = {};
    size_t w = 0;
    for (size_t r = 0; r < rows; ++r) {
        if (!h[8 * r + 7]) continue;
        ++w;
        for (int i = 0; i < 4; ++i) sum[i] += (double)h[8 * r + i];
    }
    const double d = w ? (double)w : 1.0;
    fprintf(stderr, "[rd_phase] %s waves=%zu avg cycles: head %.0f gather %.0f sort %.0f write %.0f\n", tier, w, sum[0] / d,
            sum[1] / d, sum[2] / d, sum[3] / d);
}
#endif

// One lane-group tier: the cnt txns at o.list, S lanes and RD_SEGK txns per group, on `stream` (null: the main stream).
// The tuning build runs every tier on the main stream, between the arming of its phase rows and their print.
template <int S>
static void build_seg_tier(acc_ctx *ctx, const char *tag, const char *tier, hipStream_t stream, bool narrow, uint32_t cnt, const Out &o)
{
    if (!cnt) return;
    constexpr uint32_t per_block = RD_SEGK * (64 / S) * WAVES;   // txns per workgroup
    const uint32_t blocks = (cnt + per_block - 1) / per_block;
    ctx->launch_stream = stream;
#ifdef ACC_PHASE_PROF
    ctx->launch_stream = nullptr;
    unsigned long long *pf = rd_prof_arm(ctx, blocks);
#endif
    launch(ctx, tag, narrow ? k_rd_build_seg<S, true, RD_SEGK> : k_rd_build_seg<S, false, RD_SEGK>, dim3(blocks), dim3(BLOCK), 0,
           cnt, o);
#ifdef ACC_PHASE_PROF
    rd_prof_print(ctx, tier, pf, blocks);
#endif
}

// the global tier: one workgroup per txn on a scratch region sized on the device (one read-back)
static void build_global_tier(acc_ctx *ctx, uint32_t nglb, Out &o)
{
    uint64_t *gsz = ctx->get<uint64_t>("rd_glb_sz", nglb);
    uint64_t *goff = ctx->get<uint64_t>("rd_glb_off", (size_t)nglb + 1);
    launch(ctx, "rd_glb_sizes", k_rd_glb_sizes, dim3(grid_for(nglb, BLOCK)), dim3(BLOCK), 0, nglb, o, gsz);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, gsz, goff, nglb, true, goff + nglb);
    ReadBack rb(ctx);
    const auto words = rb.u64(goff + nglb);
    rb.wait();
    o.glb_off = goff;
    o.gscratch = ctx->get<uint64_t>("rd_glb_scratch", words);
    launch(ctx, "rd_build_global", k_rd_build_global, dim3(nglb), dim3(BLOCK), 0, o);
}

// ---- 4. per-txn RangeDeps: raw sizes and tiers, build into scratch, offsets, compaction
void rd_build_txns(acc_ctx *ctx, RdBuild &b)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = b.n;
    Out &o = b.o;
    o.n = n; o.P = (uint32_t)b.P; o.key_off = b.key_off; o.rng_off = b.rng_off; o.q_out = b.v.q_out;
    o.ent = b.v.ent;
    o.txn_of_tpos = b.dict.batch_sorted ? nullptr : b.txn_of_tpos;
    o.rd_cnt = ctx->get<uint32_t>("rd_rd_cnt", n);
    o.u_cnt = ctx->get<uint32_t>("rd_u_cnt", n);
    o.a_cnt = ctx->get<uint64_t>("rd_a_cnt", n);
    uint64_t *m_raw = ctx->get<uint64_t>("rd_m_raw", n);
    uint32_t *tier = ctx->get<uint32_t>("rd_tier", n);
    uint64_t *raw_off = ctx->get<uint64_t>("rd_raw_off", (size_t)n + 1);
    uint32_t *thist = ctx->get<uint32_t>("rd_thist", 16);
    ACC_HIP(hipMemsetAsync(thist, 0, 16 * sizeof(uint32_t), st));
    launch(ctx, "rd_tsize", k_rd_tsize, dim3(grid_for(n, (size_t)BLOCK * RD_TS)), dim3(BLOCK), 0, n, o, m_raw, tier, thist);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, m_raw, raw_off, n, true, raw_off + n);
    o.raw_off = raw_off;
    // txns grouped by tier: one 8-bit radix pass (stable)
    uint64_t *tkey = ctx->get<uint64_t>("rd_tkey", n);
    launch(ctx, "rd_widen", k_widen_u32, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, (size_t)n, (const uint32_t *)tier, tkey);
    Sorted ts = radix_sort(ctx, "rs_rd_tier", tkey, nullptr, n, 4);
    uint32_t *hh = b.tier_txns, toff[17];
    {
        ReadBack rb(ctx);
        const auto hist = rb.words((const uint32_t *)thist, 16);
        rb.wait();
        toff[0] = 0;
        for (int i = 0; i < 16; ++i) { hh[i] = hist[i]; toff[i + 1] = toff[i] + hh[i]; }
    }
    o.s_arena = ctx->get<uint32_t>("rd_s_arena", 2 * b.E);
    o.s_rid = ctx->get<uint32_t>("rd_s_rid", b.E);
    o.s_dep = ctx->get<uint32_t>("rd_s_dep", b.E);
    const uint32_t *tl_sorted = ts.vals;
    // 32-bit sort keys in the lane-group tiers: range ids (< NE) and TxnId positions (< npos) within 26 bits
    const uint32_t npos = b.npos ? b.npos : n;
    const bool narrow = b.NE < (1u << 26) && npos < (1u << 26) && !(ctx->flags & ACC_OPT_RD_WIDE_SORT);   // (testing: 64-bit sorts throughout)
    ctx->stat("rangedeps.narrow_sorts", narrow ? 1 : 0);
    // tiers own disjoint txns (disjoint scratch): LDS workgroup tiers on side stream 1, 16- and 32-lane groups on side
    // stream 0, waves on the main stream, all concurrently
    ctx->fork(2);
    o.list = tl_sorted + toff[1];
    build_seg_tier<16>(ctx, "rd_build_s16", "s16", ctx->aux[0], narrow, hh[1], o);
    o.list = tl_sorted + toff[11];
    build_seg_tier<32>(ctx, "rd_build_s32", "s32", ctx->aux[0], narrow, hh[11], o);
    ctx->launch_stream = ctx->aux[1];
    for (int t = 9; t >= 3; --t) {
        if (!hh[t]) continue;
        const uint32_t n2 = 128u << (t - 3);
        const size_t lds = 2 * (size_t)n2 * sizeof(uint64_t) + BLOCK * 8 + 64 + (BLOCK + 1) * 4;
        if (lds > 64 * 1024)
            ACC_HIP(hipFuncSetAttribute((const void *)k_rd_build_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        o.list = tl_sorted + toff[t];
        launch(ctx, "rd_build_block", k_rd_build_block, dim3(hh[t]), dim3(BLOCK), lds, o, n2);
        b.block_txns += hh[t];
    }
    ctx->launch_stream = nullptr;
    o.list = tl_sorted + toff[2];
    build_seg_tier<64>(ctx, "rd_build_s64", "s64", nullptr, narrow, hh[2], o);
    ctx->join(2);
    if (hh[10]) {
        o.list = tl_sorted + toff[10];
        build_global_tier(ctx, hh[10], o);
    }
    uint64_t *rd_cnt64 = ctx->get<uint64_t>("rd_rd_cnt64", n), *u_cnt64 = ctx->get<uint64_t>("rd_u_cnt64", n);
    launch(ctx, "rd_widen", k_widen_u32, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, (size_t)n, (const uint32_t *)o.rd_cnt, rd_cnt64);
    launch(ctx, "rd_widen", k_widen_u32, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, (size_t)n, (const uint32_t *)o.u_cnt, u_cnt64);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, o.a_cnt, b.arena_off, n, true, b.arena_off + n);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, rd_cnt64, b.rd_off, n, true, b.rd_off + n);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, u_cnt64, b.u_off, n, true, b.u_off + n);
    ReadBack rb(ctx);
    const auto tot_arena = rb.u64(b.arena_off + n), tot_rd = rb.u64(b.rd_off + n), tot_u = rb.u64(b.u_off + n);
    const auto n_dict = rb.u32(b.dincl + b.NE);
    rb.wait();
    b.tot_arena = tot_arena; b.tot_rd = tot_rd; b.tot_u = tot_u;
    b.n_dict = b.NE ? (uint32_t)n_dict : 0;
    o.arena_off = b.arena_off; o.rd_off = b.rd_off; o.u_off = b.u_off;
    o.arena = ctx->get<int32_t>("rd_arena", b.tot_arena);
    o.range_id = ctx->get<uint32_t>("rd_range_id", b.tot_rd);
    o.dep_txn = ctx->get<uint32_t>("rd_dep_txn", b.tot_u);
    launch(ctx, "rd_compact", k_rd_compact, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, o);
}

}  // namespace acc
