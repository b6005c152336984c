// keydeps_mixed.hip — KeyDeps of a mixed key/range batch (acc_keydeps_mixed, the KeyDeps half of PartialDeps).
//
// A range-domain txn T is no CommandsForKey member (SafeCommandStore.updateCommandsForKey registers key txns only,
// local/SafeCommandStore.java:217-240); as a query it visits every CFK whose key lies inside its store-sliced ranges
// (impl/InMemoryCommandStore.java:274-289: commandsForKey.subMap(start, startInclusive, end, endInclusive)) and runs
// the same mapReduceActive there. The key txns' results come from the key part of the batch (build_cfk, keydeps_of);
// each range txn's covered CFK keys become "virtual" queries (T, segment) answered by the exact-replay scan
// (make_query / run_query), then one sort of (txn, TxnId rank) gives every range txn's TxnId union and indices.
#include "keydeps.hpp"

namespace acc {

constexpr uint64_t MX_ERR_DOMAIN = 1, MX_ERR_EMPTY = 2, MX_ERR_UNSORTED = 4, MX_ERR_OFF = 8;
constexpr uint32_t MX_PIECE = 32;   // covered segments per work piece

// Bucket directory of the sorted CFK keys: bucket(x) = (x - seg_key[0]) >> shift over 2^tbits buckets, the shift
// making the key span fit; bstart[b] = first segment whose bucket is >= b (b in [0, 2^tbits]). A bound search then
// bisects one bucket (a few keys) instead of all segments: 2-3 dependent loads instead of ~25.
__device__ __forceinline__ uint32_t mx_shift(const uint64_t *seg_key, uint32_t nseg, uint32_t tbits)
{
    const uint64_t span = seg_key[nseg - 1] - seg_key[0];
    const uint32_t sb = span ? 64u - (uint32_t)__clzll((long long)span) : 0u;
    return sb > tbits ? sb - tbits : 0u;
}

// bend[b] = 1 + the last segment of bucket b (written by that segment; 0 for empty buckets, zeroed before): an
// exclusive max-scan of bend is bstart (keys are sorted, so the segments of buckets <= b are a prefix)
__global__ __launch_bounds__(BLOCK) void k_mx_buckets(uint32_t nseg, uint32_t tbits, const uint64_t *__restrict__ seg_key,
                                                      uint32_t *__restrict__ bend)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nseg) return;
    const uint32_t sh = mx_shift(seg_key, nseg, tbits);
    const uint64_t k0 = seg_key[0], b = (seg_key[i] - k0) >> sh;
    if (i + 1 == nseg || ((seg_key[i + 1] - k0) >> sh) != b) bend[b] = i + 1;
}

// first segment m in [0, nseg) with seg_key[m] > x (upper) / >= x (!upper)
__device__ __forceinline__ uint32_t mx_bound(const uint64_t *seg_key, const uint32_t *bstart, uint32_t nseg, uint32_t sh,
                                             uint32_t tbits, uint64_t x, bool upper)
{
    const uint64_t k0 = seg_key[0];
    if (x < k0) return 0;
    uint64_t b = (x - k0) >> sh;
    if (b >= (1ull << tbits)) return nseg;
    return partition_point(bstart[b], bstart[b + 1], [&](uint32_t m) { return upper ? seg_key[m] <= x : seg_key[m] < x; });
}

// validation (TxnId.domain(), Range start < end, Ranges.ofSortedAndDeoverlapped) and, per range, its run of covered
// segments [ra, ra + rcnt) over the sorted CFK keys, its owner and its number of work pieces
__global__ __launch_bounds__(BLOCK) void k_mx_ranges(uint32_t n, const uint64_t *__restrict__ tl,
                                                     const uint32_t *__restrict__ key_off, const uint32_t *__restrict__ rng_off,
                                                     const uint64_t *__restrict__ rs, const uint64_t *__restrict__ re,
                                                     uint32_t end_inclusive, const uint64_t *__restrict__ seg_key, uint32_t nseg,
                                                     const uint32_t *__restrict__ bstart, uint32_t tbits,
                                                     uint32_t *__restrict__ ra, uint32_t *__restrict__ rowner,
                                                     uint64_t *__restrict__ rcnt, uint64_t *__restrict__ rpieces,
                                                     uint64_t *__restrict__ errs)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n) return;
    const bool isr = (tl[t] & 1u) != 0;
    const uint32_t r0 = rng_off[t], r1 = rng_off[t + 1];
    uint64_t e = 0;
    if (r1 < r0) e |= MX_ERR_OFF;
    else {
        if (isr && key_off[t + 1] != key_off[t]) e |= MX_ERR_DOMAIN;
        if (!isr && r1 != r0) e |= MX_ERR_DOMAIN;
        for (uint32_t j = r0; j < r1; ++j) {
            const uint64_t s = rs[j], x = re[j];
            if (s >= x) e |= MX_ERR_EMPTY;
            if (j > r0 && re[j - 1] > s) e |= MX_ERR_UNSORTED;
            // EndInclusive (s, x]: keys > s .. <= x; StartInclusive [s, x): keys >= s .. < x
            uint32_t a = 0, b = 0;
            if (nseg) {
                const uint32_t sh = mx_shift(seg_key, nseg, tbits);
                a = mx_bound(seg_key, bstart, nseg, sh, tbits, s, end_inclusive != 0);
                b = mx_bound(seg_key, bstart, nseg, sh, tbits, x, end_inclusive != 0);
            }
            const uint32_t c = (e || b < a) ? 0u : b - a;
            ra[j] = a;
            rowner[j] = t;
            rcnt[j] = c;
            rpieces[j] = (c + MX_PIECE - 1) / MX_PIECE;
        }
    }
    if (e) atomicOr((unsigned long long *)errs, (unsigned long long)e);
}


// work pieces: piece p = (range, first covered segment), at most MX_PIECE segments each. Its record (one thread per
// range writes its pieces', so the count / emit passes read one record instead of a chain of dependent loads):
// prec[2p] = (owner txn, first segment, covered-key index of that segment within the txn's keys, queries),
// prec[2p + 1] = (T.executeAt rank S, T's TxnId rank, T.kind().witnesses() mask | p1 << 8, 0)
__global__ __launch_bounds__(BLOCK) void k_mx_pieces(uint32_t R, const uint64_t *__restrict__ poff, const uint32_t *__restrict__ ra,
                                                     const uint32_t *__restrict__ rowner, const uint64_t *__restrict__ rcnt,
                                                     const uint64_t *__restrict__ r_off, const uint32_t *__restrict__ rng_off,
                                                     const uint32_t *__restrict__ rank, uint32_t n, const uint64_t *__restrict__ tl,
                                                     uint4 *__restrict__ prec)
{
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= R) return;
    const uint64_t p0 = poff[j], p1 = poff[j + 1];
    if (p0 == p1) return;
    const uint32_t t = rowner[j], a = ra[j], c = (uint32_t)rcnt[j];
    const uint32_t kb = (uint32_t)(r_off[j] - r_off[rng_off[t]]);
    const uint32_t S = rank[n + t], tr = rank[t];
    const uint32_t wk = witnesses((uint32_t)(tl[t] >> 1) & 7u) | (S != tr ? 1u << 8 : 0u);
    for (uint64_t p = p0; p < p1; ++p) {
        const uint32_t k0 = (uint32_t)(p - p0) * MX_PIECE;
        prec[2 * p] = make_uint4(t, a + k0, kb + k0, min(c - k0, MX_PIECE));
        prec[2 * p + 1] = make_uint4(S, tr, wk, 0);
    }
}

// 32 lanes per piece, one covered segment (one query) per lane
__device__ __forceinline__ uint32_t mx_scan32(uint32_t x, uint32_t sub)   // inclusive, within the 32-lane half
{
#pragma unroll
    for (uint32_t d = 1; d < 32; d <<= 1) {
        const uint32_t u = __shfl_up(x, d, 64);
        if (sub >= d) x += u;
    }
    return x;
}

// count pass: entries and non-empty keys per piece. Each lane keeps its count in qc, or, for a single entry (nearly
// every non-empty (range txn, key) query: one conflicting key txn), the entry itself with MX_ONE set, so the emit pass
// replays the scan only for the rare lanes with two or more entries
constexpr uint32_t MX_ONE = 0x80000000u;
__device__ __forceinline__ uint32_t mx_qcount(uint32_t q) { return (q & MX_ONE) ? 1u : q; }

// A segment holding one CFK entry (nearly every covered key of a sparse key space) is answered in place: with
// s1 = s0 + 1, make_query_ts / run_query reduce to one test of that entry. Its committed[] is itself or empty, so any
// maxCommittedBefore M is its own executeAt, which the prefix-max prune (executeAt < M) never removes; nothing of the
// segment lies below scanStart = s0; the scan [s0, insertPos) is the entry exactly when its TxnId is below T.executeAt.
// Queries over longer segments go to deferred lists that k_mx_pdefer answers densely, adding into the piece totals:
// MX_DSLOTS lists (block b appends to list b % MX_DSLOTS with wave-aggregated atomics on that list's counter, so the
// appends spread over many addresses), list s holding at most dcap entries (its blocks' lanes); dlist null: every
// query in place.
constexpr uint32_t MX_DSLOTS = 1024;
__global__ __launch_bounds__(BLOCK) void k_mx_pcount(uint64_t NP, const uint4 *__restrict__ prec, CfkView v,
                                                     uint64_t *__restrict__ pe_cnt, uint32_t *__restrict__ pk_cnt,
                                                     uint32_t *__restrict__ qc, uint32_t pack, uint32_t *__restrict__ dlist,
                                                     uint32_t *__restrict__ dcnt, uint32_t dcap)
{
    const uint64_t p = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 5;
    const uint32_t sub = threadIdx.x & 31u, g0 = lane_id() & 32u;
    uint32_t c = 0;
    bool dfr = false;
    if (p < NP) {
        const uint4 pr = prec[2 * p], pq = prec[2 * p + 1];
        uint32_t f = 0;
        if (sub < pr.w) {
            const uint32_t seg = pr.y + sub;
            const uint32_t s0 = v.seg_start[seg], s1 = v.seg_start[seg + 1];
            if (dlist && s1 - s0 == 1) {
                const uint32_t S = pq.x, trank = pq.y, wk = pq.z & 0xFFu;
                const uint32_t r = v.s_rank[s0], info = v.s_info[s0], st = info & 7u;
                c = (r < S && ((wk >> (info >> 3)) & 1u) && st != 0 && st != 7 && !((pq.z >> 8) && r == trank)) ? 1u : 0u;
                f = r;
            } else if (dlist) dfr = true;
            else c = run_query<false, true>(v, make_query_ts(v, pr.x, seg), &f);
        }
        qc[p * 32 + sub] = (pack && c == 1) ? (MX_ONE | f) : c;
    }
    const uint64_t db = __ballot(dfr);
    if (db) {
        const uint32_t slot = blockIdx.x % MX_DSLOTS;
        uint32_t base = 0;
        const uint32_t lead = (uint32_t)__ffsll((unsigned long long)db) - 1;
        if (lane_id() == lead) base = atomicAdd(&dcnt[slot], (uint32_t)__popcll(db));
        base = __shfl(base, (int)lead, 64);
        if (dfr) dlist[(size_t)slot * dcap + base + (uint32_t)__popcll(db & ((1ull << lane_id()) - 1))] = (uint32_t)(p * 32 + sub);
    }
    const uint32_t ce = mx_scan32(c, sub), ck = mx_scan32(c != 0 ? 1u : 0u, sub);
    const uint32_t te = __shfl(ce, (int)(g0 + 31), 64), tk = __shfl(ck, (int)(g0 + 31), 64);
    if (p < NP && sub == 0) { pe_cnt[p] = te; pk_cnt[p] = tk; }
}

// the deferred queries (segments of two or more entries): the exact-replay scan, one lane each; blockIdx.y = list,
// a grid-stride loop over its device-side count
__global__ __launch_bounds__(BLOCK) void k_mx_pdefer(const uint4 *__restrict__ prec, CfkView v, const uint32_t *__restrict__ dlist,
                                                     const uint32_t *__restrict__ dcnt, uint32_t dcap, uint64_t *__restrict__ pe_cnt,
                                                     uint32_t *__restrict__ pk_cnt, uint32_t *__restrict__ qc, uint32_t pack)
{
    const uint32_t nd = dcnt[blockIdx.y];
    const uint32_t *lst = dlist + (size_t)blockIdx.y * dcap;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < nd; i += gridDim.x * BLOCK) {
        const uint32_t q = lst[i], p = q >> 5, sub = q & 31u;
        const uint4 pr = prec[2 * (uint64_t)p];
        uint32_t f = 0;
        const uint32_t c = run_query<false, true>(v, make_query_ts(v, pr.x, pr.y + sub), &f);
        qc[q] = (pack && c == 1) ? (MX_ONE | f) : c;
        if (c) {
            atomicAdd((unsigned long long *)&pe_cnt[p], (unsigned long long)c);
            atomicAdd(&pk_cnt[p], 1u);
        }
    }
}

struct MxE {   // emitted entries and key records of the range txns
    uint32_t *deps, *owner;          // [Ex]: TxnId rank, owning txn
    uint32_t *kx_idx, *kx_end;       // [Kx]: covered-key index, end of its entries (absolute entry index)
    uint64_t *kx_code;               // [Kx]: key code
};

__global__ __launch_bounds__(BLOCK) void k_mx_pemit(uint64_t NP, const uint4 *__restrict__ prec, const uint64_t *__restrict__ seg_key,
                                                    CfkView v, const uint64_t *__restrict__ pe_off,
                                                    const uint32_t *__restrict__ pk_off, MxE x, const uint32_t *__restrict__ qc)
{
    const uint64_t p = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 5;
    const uint32_t sub = threadIdx.x & 31u;
    uint32_t c = 0, q = 0;
    uint4 pr = make_uint4(0, 0, 0, 0);
    bool act = false;
    if (p < NP) {
        pr = prec[2 * p];
        q = qc[p * 32 + sub];
        act = sub < pr.w;
        c = act ? mx_qcount(q) : 0u;
    }
    const uint32_t ce = mx_scan32(c, sub), ck = mx_scan32(c != 0 ? 1u : 0u, sub);
    if (!act || c == 0) return;
    const uint64_t e = pe_off[p] + (ce - c);
    const uint32_t seg = pr.y + sub;
    if (q & MX_ONE) x.deps[e] = q & ~MX_ONE;
    else run_query<true>(v, make_query_ts(v, pr.x, seg), x.deps + e);
    const uint32_t kr = pk_off[p] + ck - 1;
    x.kx_idx[kr] = pr.z + sub;
    x.kx_code[kr] = seg_key[seg];
    x.kx_end[kr] = (uint32_t)(e + c);
}

__global__ __launch_bounds__(BLOCK) void k_mx_toff(uint32_t n, const uint32_t *__restrict__ rng_off, const uint64_t *__restrict__ poff,
                                                   const uint64_t *__restrict__ pe_off, const uint32_t *__restrict__ pk_off,
                                                   uint64_t *__restrict__ etoff, uint32_t *__restrict__ ktoff)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t > n) return;
    const uint64_t p = poff[rng_off[t]];
    etoff[t] = pe_off[p];
    ktoff[t] = pk_off[p];
}

// the owning txn of every emitted entry (fallback union only)
__global__ __launch_bounds__(BLOCK) void k_mx_owner(uint32_t n, const uint64_t *__restrict__ etoff, uint32_t *__restrict__ owner)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n) return;
    for (uint64_t e = etoff[t]; e < etoff[t + 1]; ++e) owner[e] = t;
}

// sort keys (txn, TxnId rank) of the emitted entries (fallback union)
__global__ __launch_bounds__(BLOCK) void k_mx_sortkeys(uint64_t E, const uint32_t *__restrict__ deps, const uint32_t *__restrict__ owner,
                                                       int rbits, uint64_t *__restrict__ key)
{
    const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e < E) key[e] = ((uint64_t)owner[e] << rbits) | deps[e];
}

__global__ __launch_bounds__(BLOCK) void k_mx_uflag(uint64_t E, const uint64_t *__restrict__ sk, uint32_t *__restrict__ f)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < E) f[i] = i == 0 || sk[i] != sk[i - 1];
}

struct MxKv {   // the key-txn KeyDeps (keydeps_of's view)
    const uint64_t *arena_off, *kd_off, *u_off;
    const int32_t *arena;
    const uint32_t *key_idx, *dep_txn;
};
struct MxOut {
    uint64_t *arena_off, *kd_off, *u_off;
    int32_t *arena;
    uint32_t *key_idx, *dep_txn;
    uint64_t *kd_key;
};
// per-txn TxnId union of the emitted entries: idx_of_e[e] = index of entry e's TxnId in its txn's union,
// dep_scr[e0 + i] = batch index of the i-th union TxnId, ucnt[t] = union size
struct MxU {
    const uint32_t *deps;
    const uint64_t *etoff;
    const uint32_t *txn_of_rank;
    uint32_t *idx_of_e, *dep_scr, *ucnt;
};

// per txn: entry count routing into tier lists (txns without entries: none): E <= 16, <= 32, <= 64 (lane groups),
// <= MX_MID_E (wave, LDS), <= MX_BLK_E (block); beyond: the sorted fallback (flag gst[1]).
// gst: [0] block count, [1] fallback flag, [2] mid count, [3..5] 16 / 32 / 64-lane counts
constexpr uint32_t MX_MID_E = 512, MX_BLK_E = 4096;
struct MxLists {
    uint32_t *l[5];   // 16, 32, 64, mid, block
};
// MX_RT chunks of BLOCK txns per workgroup: one list-counter add per list and workgroup (the five counters share one
// line: per-256-txn adds serialised there); list order is free (each txn writes its own outputs)
constexpr int MX_RT = 16;
__global__ __launch_bounds__(BLOCK) void k_mx_route(uint32_t n, const uint64_t *__restrict__ etoff, MxLists L,
                                                    uint64_t *__restrict__ gst)
{
    __shared__ uint32_t wcnt[5][MX_RT * WAVES], base[5];
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int cs[MX_RT];
    bool ovf = false;
#pragma unroll
    for (int r = 0; r < MX_RT; ++r) {
        const uint32_t t = (blockIdx.x * MX_RT + (uint32_t)r) * BLOCK + threadIdx.x;
        int c = -1;
        if (t < n) {
            const uint64_t E = etoff[t + 1] - etoff[t];
            if (E == 0) c = -1;
            else if (E <= 16) c = 0;
            else if (E <= 32) c = 1;
            else if (E <= 64) c = 2;
            else if (E <= MX_MID_E) c = 3;
            else if (E <= MX_BLK_E) c = 4;
            else ovf = true;
        }
        cs[r] = c;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint32_t cnt = (uint32_t)__popcll(__ballot(c == k));
            if (lane == 0) wcnt[k][r * WAVES + w] = cnt;
        }
    }
    if (ovf) atomicOr((unsigned long long *)&gst[1], 1ull);
    __syncthreads();
    if (threadIdx.x < 5) {
        uint32_t tot = 0;
        for (int q = 0; q < MX_RT * WAVES; ++q) { const uint32_t x = wcnt[threadIdx.x][q]; wcnt[threadIdx.x][q] = tot; tot += x; }
        const int slot = threadIdx.x == 4 ? 0 : threadIdx.x == 3 ? 2 : 3 + (int)threadIdx.x;
        base[threadIdx.x] = tot ? (uint32_t)atomicAdd((unsigned long long *)&gst[slot], (unsigned long long)tot) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < MX_RT; ++r) {
        const int c = cs[r];
        const uint32_t t = (blockIdx.x * MX_RT + (uint32_t)r) * BLOCK + threadIdx.x;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint64_t bal = __ballot(c == k);
            if (c == k) L.l[k][base[k] + wcnt[k][r * WAVES + w] + (uint32_t)__popcll(bal & lt)] = t;
        }
    }
}

// groups of S lanes (S = 16, 32, 64), one listed txn each (E <= S): register bitonic of (rank << 32 | local entry)
template <int S>
__global__ __launch_bounds__(BLOCK) void k_mx_union_seg(const uint32_t *__restrict__ list, const uint64_t *__restrict__ cnt, MxU u)
{
    constexpr uint32_t G = 64 / S;
    const uint32_t lane = lane_id(), grp = lane / S, sub = lane & (S - 1);
    const uint32_t li = (blockIdx.x * WAVES + (threadIdx.x >> 6)) * G + grp;
    const bool live = li < (uint32_t)*cnt;
    const uint32_t t = live ? list[li] : 0;
    const uint64_t e0 = live ? u.etoff[t] : 0;
    const uint32_t E = live ? (uint32_t)(u.etoff[t + 1] - e0) : 0;
    const bool in = sub < E;
    uint64_t x = in ? (((uint64_t)u.deps[e0 + sub] << 32) | sub) : ~0ull;
#pragma unroll
    for (uint32_t k = 2; k <= (uint32_t)S; k <<= 1) {
#pragma unroll
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            const uint64_t y = xor_lanes(x, (int)jj);
            const bool up = k == (uint32_t)S || (lane & k) == 0, lower = (lane & jj) == 0;   // ascending per group
            const uint64_t mn = x < y ? x : y, mx = x < y ? y : x;
            x = (lower == up) ? mn : mx;
        }
    }
    const uint64_t prev = shfl_up(x, 1);
    const bool nw = in && (sub == 0 || (prev >> 32) != (x >> 32));
    const uint64_t gmask = S == 64 ? ~0ull : (((1ull << S) - 1) << (grp * S));
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const uint64_t bal = __ballot(nw) & gmask;
    const uint32_t idx = (uint32_t)__popcll(bal & lt) + (nw ? 1u : 0u) - 1u;
    if (in) {
        u.idx_of_e[e0 + (uint32_t)x] = idx;
        if (nw) u.dep_scr[e0 + idx] = u.txn_of_rank[(uint32_t)(x >> 32)];
    }
    if (live && sub == 0) u.ucnt[t] = (uint32_t)__popcll(bal);
}

// R values per lane sorted across the wave (element r * 64 + lane), ascending: partners 64 or more apart are registers
// of the same lane, the others lanes (shuffles)
template <int R>
__device__ __forceinline__ void wave_reg_sort(uint64_t (&v)[R])
{
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t k = 2; k <= 64u * R; k <<= 1) {
#pragma unroll
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            if (jj >= 64) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int r2 = r ^ (int)(jj >> 6);
                    if (r2 > r) {
                        const bool up = ((((uint32_t)r << 6) | lane) & k) == 0;
                        const uint64_t a = v[r], b = v[r2];
                        if ((a > b) == up) { v[r] = b; v[r2] = a; }
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint64_t y = xor_lanes(v[r], (int)jj);
                    const bool up = ((((uint32_t)r << 6) | lane) & k) == 0, lower = (lane & jj) == 0;
                    const uint64_t mn = v[r] < y ? v[r] : y, mx = v[r] < y ? y : v[r];
                    v[r] = (lower == up) ? mn : mx;
                }
            }
        }
    }
}

// a txn's union over E <= 64 R entries in registers: sort (rank << 32 | entry), distinct ranks -> indices
template <int R>
__device__ __forceinline__ void mx_union_regs(const MxU &u, uint32_t t, uint64_t e0, uint32_t E)
{
    const uint32_t lane = lane_id();
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    uint64_t v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = ((uint32_t)r << 6) | lane;
        v[r] = i < E ? (((uint64_t)u.deps[e0 + i] << 32) | i) : ~0ull;
    }
    wave_reg_sort<R>(v);
    uint32_t base = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint64_t x = v[r];
        uint64_t prev = shfl_up(x, 1);
        if (r > 0) {
            const uint64_t pl = shfl_idx(v[r - 1], 63);
            if (lane == 0) prev = pl;
        }
        const uint32_t i = ((uint32_t)r << 6) | lane;
        const bool in = i < E;
        const bool nw = in && (i == 0 || (prev >> 32) != (x >> 32));
        const uint64_t bal = __ballot(nw);
        const uint32_t idx = base + (uint32_t)__popcll(bal & lt) + (nw ? 1u : 0u) - 1u;
        if (in) {
            u.idx_of_e[e0 + (uint32_t)x] = idx;
            if (nw) u.dep_scr[e0 + idx] = u.txn_of_rank[(uint32_t)(x >> 32)];
        }
        base += (uint32_t)__popcll(bal);
    }
    if (lane == 0) u.ucnt[t] = base;
}

// wave per listed txn, 64 < E <= MX_MID_E: registers up to 256 entries, one wave's LDS bitonic beyond
__global__ __launch_bounds__(BLOCK) void k_mx_union_mid(const uint32_t *__restrict__ list, const uint64_t *__restrict__ gst, MxU u)
{
    __shared__ uint64_t sbuf[WAVES][MX_MID_E];
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6, i = blockIdx.x * WAVES + w;
    if (i >= (uint32_t)gst[2]) return;
    const uint32_t t = list[i];
    uint64_t *buf = sbuf[w];
    const uint64_t e0 = u.etoff[t];
    const uint32_t E = (uint32_t)(u.etoff[t + 1] - e0);
    if (E <= 128) { mx_union_regs<2>(u, t, e0, E); return; }   // wave-uniform
    if (E <= 256) { mx_union_regs<4>(u, t, e0, E); return; }
    uint32_t n2 = 128;
    while (n2 < E) n2 <<= 1;
    for (uint32_t q = lane; q < n2; q += 64) buf[q] = q < E ? (((uint64_t)u.deps[e0 + q] << 32) | q) : ~0ull;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    wave_bitonic_lds(buf, n2);
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    uint32_t distinct = 0;
    for (uint32_t q0 = 0; q0 < E; q0 += 64) {
        const uint32_t q = q0 + lane;
        const bool in = q < E;
        const uint64_t x = in ? buf[q] : 0;
        const bool nw = in && (q == 0 || (buf[q - 1] >> 32) != (x >> 32));
        const uint64_t bal = __ballot(nw);
        const uint32_t idx = distinct + (uint32_t)__popcll(bal & lt) + (nw ? 1u : 0u) - 1u;
        if (in) {
            u.idx_of_e[e0 + (uint32_t)x] = idx;
            if (nw) u.dep_scr[e0 + idx] = u.txn_of_rank[(uint32_t)(x >> 32)];
        }
        distinct += (uint32_t)__popcll(bal);
    }
    if (lane == 0) u.ucnt[t] = distinct;
}

// block per listed txn, 64 < E <= MX_BLK_E: LDS bitonic
__global__ __launch_bounds__(BLOCK) void k_mx_union_block(const uint32_t *__restrict__ list, const uint64_t *__restrict__ gst, MxU u)
{
    __shared__ uint64_t buf[MX_BLK_E];
    __shared__ uint32_t lds[WAVES];
    const uint32_t b = blockIdx.x;
    if (b >= (uint32_t)gst[0]) return;
    const uint32_t t = list[b], tid = threadIdx.x;
    const uint64_t e0 = u.etoff[t];
    const uint32_t E = (uint32_t)(u.etoff[t + 1] - e0);
    uint32_t n2 = 128;
    while (n2 < E) n2 <<= 1;
    for (uint32_t i = tid; i < n2; i += BLOCK) buf[i] = i < E ? (((uint64_t)u.deps[e0 + i] << 32) | i) : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= n2; k <<= 1)
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            for (uint32_t pi = tid; pi < (n2 >> 1); pi += BLOCK) {
                const uint32_t i = ((pi & ~(jj - 1)) << 1) | (pi & (jj - 1)), l = i | jj;
                const uint64_t xa = buf[i], ya = buf[l];
                if ((xa > ya) == ((i & k) == 0)) { buf[i] = ya; buf[l] = xa; }
            }
            __syncthreads();
        }
    // distinct index: chunked scan of the "new value" flags (contiguous chunks per thread)
    const uint32_t per = (E + BLOCK - 1) / BLOCK, lo = min(E, tid * per), hi = min(E, lo + per);
    uint32_t c = 0;
    for (uint32_t i = lo; i < hi; ++i) c += i == 0 || (buf[i] >> 32) != (buf[i - 1] >> 32);
    uint32_t total;
    uint32_t run = block_exclusive(c, OpAdd<uint32_t>(), lds, total);
    for (uint32_t i = lo; i < hi; ++i) {
        const uint64_t x = buf[i];
        const bool nw = i == 0 || (x >> 32) != (buf[i - 1] >> 32);
        run += nw;
        u.idx_of_e[e0 + (uint32_t)x] = run - 1;
        if (nw) u.dep_scr[e0 + run - 1] = u.txn_of_rank[(uint32_t)(x >> 32)];
    }
    if (tid == 0) u.ucnt[t] = total;
}

// global fallback (some txn beyond MX_BLK_E): from the (txn, rank) sort
__global__ __launch_bounds__(BLOCK) void k_mx_union_sorted(uint64_t E, const uint64_t *__restrict__ sk, const uint32_t *__restrict__ sperm,
                                                           const uint32_t *__restrict__ uflag, const uint32_t *__restrict__ ucum,
                                                           const uint32_t *__restrict__ owner, int rbits, MxU u)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= E) return;
    const uint32_t e = sperm[i];
    const uint64_t e0 = u.etoff[owner[e]];
    const uint32_t idx = ucum[i] + uflag[i] - 1 - ucum[e0];
    u.idx_of_e[e] = idx;
    if (uflag[i]) u.dep_scr[e0 + idx] = u.txn_of_rank[(uint32_t)(sk[i] & ((1ull << rbits) - 1))];
}
__global__ __launch_bounds__(BLOCK) void k_mx_ucnt_sorted(uint32_t n, const uint64_t *__restrict__ etoff, const uint32_t *__restrict__ ucum,
                                                          uint32_t *__restrict__ ucnt)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < n) ucnt[t] = ucum[etoff[t + 1]] - ucum[etoff[t]];
}

__global__ __launch_bounds__(BLOCK) void k_mx_sizes(uint32_t n, MxKv kv, const uint64_t *__restrict__ etoff,
                                                    const uint32_t *__restrict__ ktoff, const uint32_t *__restrict__ ucnt,
                                                    uint64_t *__restrict__ a_cnt, uint64_t *__restrict__ kd_cnt,
                                                    uint64_t *__restrict__ u_cnt)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t == n) { a_cnt[n] = 0; kd_cnt[n] = 0; u_cnt[n] = 0; }   // the exclusive scans over n + 1 end in the totals
    if (t >= n) return;
    const uint64_t ex = etoff[t + 1] - etoff[t];
    const uint64_t kd = ktoff[t + 1] - ktoff[t];
    a_cnt[t] = (kv.arena_off[t + 1] - kv.arena_off[t]) + kd + ex;
    kd_cnt[t] = (kv.kd_off[t + 1] - kv.kd_off[t]) + kd;
    u_cnt[t] = (kv.u_off[t + 1] - kv.u_off[t]) + (ex ? ucnt[t] : 0u);
}

// the combined layout. A workgroup owns BLOCK consecutive txns, whose output runs are one contiguous range of each
// output array: each output element takes its txn from a chunk owner map (chunk_owners) and reads from that txn's
// source (key txns: keydeps_of's result, with key codes; range txns: their key records, per-entry union indices and
// union TxnIds), so every write is a whole-line access.
__global__ __launch_bounds__(BLOCK) void k_mx_write(uint32_t n, MxKv kv, const uint64_t *__restrict__ etoff,
                                                    const uint32_t *__restrict__ ktoff, MxE x,
                                                    const uint32_t *__restrict__ idx_of_e, const uint32_t *__restrict__ dep_scr,
                                                    const uint32_t *__restrict__ key_off, const uint64_t *__restrict__ key_code,
                                                    MxOut o)
{
    __shared__ uint64_t ao[BLOCK + 1], ko[BLOCK + 1], uo[BLOCK + 1];   // output offsets
    __shared__ uint64_t sa[BLOCK], sk[BLOCK], su[BLOCK];                // source bases: arena / keys / TxnIds
    __shared__ uint32_t kdn[BLOCK], kofs[BLOCK];                        // range txn: key records; key txn: key_off
    __shared__ uint32_t own[8 * BLOCK], red[WAVES];                     // chunk owner map (chunk_owners)
    const uint32_t t0 = blockIdx.x * BLOCK, nt = min((uint32_t)BLOCK, n - t0), tid = threadIdx.x;
    if (tid < nt) {
        const uint32_t t = t0 + tid;
        ao[tid] = o.arena_off[t]; ko[tid] = o.kd_off[t]; uo[tid] = o.u_off[t];
        const uint64_t e0 = etoff[t], ex = etoff[t + 1] - e0;
        if (ex) {
            const uint32_t k0 = ktoff[t];
            kdn[tid] = ktoff[t + 1] - k0;
            sa[tid] = e0; sk[tid] = k0; su[tid] = e0;
        } else {
            kdn[tid] = 0xFFFFFFFFu;   // a key txn
            sa[tid] = kv.arena_off[t]; sk[tid] = kv.kd_off[t]; su[tid] = kv.u_off[t];
            kofs[tid] = key_off[t];
        }
    }
    if (tid == 0) { ao[nt] = o.arena_off[t0 + nt]; ko[nt] = o.kd_off[t0 + nt]; uo[nt] = o.u_off[t0 + nt]; }
    __syncthreads();
    // per array, chunks of U * BLOCK outputs: the owner map of the chunk (chunk_owners), then U outputs per thread,
    // interleaved across the block (whole-line stores), each reading its txn from the map
    constexpr int U = 8;
    uint32_t carry = 0;
    for (uint64_t c0 = ao[0]; c0 < ao[nt]; c0 += (uint64_t)U * BLOCK) {
        chunk_owners<U>(nt, ao, c0, own, red, carry);
        int32_t v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t p = (uint32_t)u * BLOCK + tid;
            const uint64_t j = c0 + p;
            v[u] = 0;
            if (j < ao[nt]) {
                const uint32_t a = own[p];
                const uint64_t i = j - ao[a];
                const uint32_t kd = kdn[a];
                if (kd == 0xFFFFFFFFu) v[u] = kv.arena[sa[a] + i];
                else if (i < kd) v[u] = (int32_t)(kd + (x.kx_end[sk[a] + i] - (uint32_t)sa[a]));
                else v[u] = (int32_t)idx_of_e[sa[a] + i - kd];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t j = c0 + (uint64_t)u * BLOCK + tid;
            if (j < ao[nt]) o.arena[j] = v[u];
        }
    }
    carry = 0;
    for (uint64_t c0 = ko[0]; c0 < ko[nt]; c0 += (uint64_t)U * BLOCK) {
        chunk_owners<U>(nt, ko, c0, own, red, carry);
        uint32_t ki[U];
        uint64_t kc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t p = (uint32_t)u * BLOCK + tid;
            const uint64_t j = c0 + p;
            ki[u] = 0; kc[u] = 0;
            if (j < ko[nt]) {
                const uint32_t a = own[p];
                const uint64_t i = j - ko[a];
                if (kdn[a] == 0xFFFFFFFFu) {
                    ki[u] = kv.key_idx[sk[a] + i];
                    kc[u] = key_code[kofs[a] + ki[u]];
                } else {
                    ki[u] = x.kx_idx[sk[a] + i];
                    kc[u] = x.kx_code[sk[a] + i];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t j = c0 + (uint64_t)u * BLOCK + tid;
            if (j < ko[nt]) { o.key_idx[j] = ki[u]; o.kd_key[j] = kc[u]; }
        }
    }
    carry = 0;
    for (uint64_t c0 = uo[0]; c0 < uo[nt]; c0 += (uint64_t)U * BLOCK) {
        chunk_owners<U>(nt, uo, c0, own, red, carry);
        uint32_t d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t p = (uint32_t)u * BLOCK + tid;
            const uint64_t j = c0 + p;
            d[u] = 0;
            if (j < uo[nt]) {
                const uint32_t a = own[p];
                const uint64_t i = j - uo[a];
                d[u] = kdn[a] == 0xFFFFFFFFu ? kv.dep_txn[su[a] + i] : dep_scr[su[a] + i];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t j = c0 + (uint64_t)u * BLOCK + tid;
            if (j < uo[nt]) o.dep_txn[j] = d[u];
        }
    }
}

void keydeps_mixed(acc_ctx *ctx, const acc_range_batch_in *in, acc_keydeps_view *view, SharedDict *shared)
{
    if (!in || !view) fail(ACC_E_ARG, "null argument");
    if (in->mem != ACC_MEM_HOST && in->mem != ACC_MEM_DEVICE) fail(ACC_E_ARG, "mem must be ACC_MEM_HOST or ACC_MEM_DEVICE");
    if (in->end_inclusive > 1) fail(ACC_E_ARG, "end_inclusive must be 0 (StartInclusive) or 1 (EndInclusive)");
    const uint32_t n = in->n_txn;
    const size_t R = (size_t)in->n_ranges;
    if (R >= 0xFFFFFFFFull) fail(ACC_E_ARG, "n_ranges must be < 2^32");
    hipStream_t st = ctx->stream;
    ctx->kd_valid = false;

    // ---- key txns (and the CFK snapshot): the key part of the batch, exactly as acc_keydeps_batch runs it, with the
    // segment keys and pair positions the range queries need
    acc_batch_in kin{ n, in->mem, in->n_pairs, in->txn_id, in->execute_at, in->status, in->key_off, in->key_code };
    acc_keydeps_view kv{};
    CfkOpts opts;
    opts.seg_keys = true;
    opts.sparse = R > 0;
    CfkBuild cb = build_cfk(ctx, &kin, opts);
    keydeps_of(ctx, cb, &kv);
    const int rbits = cb.dict.rbits;
    ctx->kd_valid = false;
    if (shared) {
        shared->valid = cb.cfk; shared->dict = cb.dict; shared->owner = cb.owner;
        if (shared->ready && shared->valid) shared->ready(*shared);
    }
    if (n == 0) {
        kv.kd_key = ctx->get<uint64_t>("mx_kd_key", 1);
        *view = kv;
        ctx->kd_view = kv;
        ctx->kd_valid = true;
        return;
    }
    const uint32_t *key_off = stage_in(ctx, "in_key_off", in->key_off, (size_t)n + 1, in->mem);
    const uint64_t *key_code = stage_in(ctx, "in_key_code", in->key_code, (size_t)in->n_pairs, in->mem);
    const uint64_t *tl = stage_in(ctx, "in_tl", in->txn_id.lsb, n, in->mem);
    const uint32_t *rng_off = stage_in(ctx, "in_rng_off", in->rng_off, (size_t)n + 1, in->mem);
    const uint64_t *rs = stage_in(ctx, "in_rng_start", in->rng_start, R, in->mem);
    const uint64_t *re = stage_in(ctx, "in_rng_end", in->rng_end, R, in->mem);

    // ---- covered segments per range, work pieces
    const uint32_t nseg = cb.cfk ? cfk_nseg(ctx, cb) : 0u;
    const uint64_t *seg_key = cb.cfk ? cb.seg_key : ctx->get<uint64_t>("mx_seg_key", 1);   // written by k_v2_apply
    // bucket directory: about one key per bucket
    const uint32_t tbits = nseg ? (uint32_t)std::min(26, std::max(0, bits_for(nseg) - 1)) : 0u;
    const size_t nbk = (size_t)1 << tbits;
    uint32_t *bstart = ctx->get<uint32_t>("mx_bstart", nbk + 1);
    if (nseg) {
        uint32_t *bend = ctx->get<uint32_t>("mx_bend", nbk);
        ACC_HIP(hipMemsetAsync(bend, 0, nbk * sizeof(uint32_t), st));
        launch(ctx, "mx_buckets", k_mx_buckets, dim3(grid_for(nseg, BLOCK)), dim3(BLOCK), 0, nseg, tbits,
               (const uint64_t *)seg_key, bend);
        scan<uint32_t, OpMax<uint32_t>>(ctx, bend, bstart, nbk, true, bstart + nbk);
    }
    uint32_t *ra = ctx->get<uint32_t>("mx_ra", R + 1);
    uint32_t *rowner = ctx->get<uint32_t>("mx_rowner", R + 1);
    uint64_t *rcnt = ctx->get<uint64_t>("mx_rcnt", R + 1);
    uint64_t *rpieces = ctx->get<uint64_t>("mx_rpieces", R + 1);
    uint64_t *r_off = ctx->get<uint64_t>("mx_r_off", R + 2);
    uint64_t *poff = ctx->get<uint64_t>("mx_poff", R + 2);
    uint64_t *errs = ctx->get<uint64_t>("mx_errs", 1);
    ACC_HIP(hipMemsetAsync(errs, 0, 8, st));
    launch(ctx, "mx_ranges", k_mx_ranges, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, tl, key_off, rng_off, rs, re,
           in->end_inclusive, (const uint64_t *)seg_key, nseg, (const uint32_t *)bstart, tbits, ra, rowner, rcnt, rpieces, errs);
    if (R) {
        const uint64_t *si[2] = { rcnt, rpieces };
        uint64_t *so[2] = { r_off, poff }, *stot[2] = { r_off + R, poff + R };
        const size_t sn[2] = { R, R };
        scan_multi<uint64_t, OpAdd<uint64_t>>(ctx, 2, si, so, sn, true, stot);
    } else {
        ACC_HIP(hipMemsetAsync(r_off, 0, 8, st));
        ACC_HIP(hipMemsetAsync(poff, 0, 8, st));
    }
    ACC_HIP(hipMemcpyAsync(ctx->pinned, errs, 8, hipMemcpyDeviceToHost, st));
    ACC_HIP(hipMemcpyAsync(ctx->pinned + 1, r_off + R, 8, hipMemcpyDeviceToHost, st));
    ACC_HIP(hipMemcpyAsync(ctx->pinned + 2, poff + R, 8, hipMemcpyDeviceToHost, st));
    ctx->sync();
    const uint64_t merr = ctx->pinned[0];
    if (merr & MX_ERR_DOMAIN) fail(ACC_E_ARG, "a range-domain txn lists keys or a key-domain txn lists ranges (TxnId.domain())");
    if (merr & MX_ERR_EMPTY) fail(ACC_E_ARG, "range start must be below its end (Range: start >= end)");
    if (merr & MX_ERR_UNSORTED) fail(ACC_E_ARG, "ranges of a txn must be sorted and deoverlapped (Ranges.ofSortedAndDeoverlapped)");
    if (merr & MX_ERR_OFF) fail(ACC_E_ARG, "rng_off must be non-decreasing");
    const uint64_t V = ctx->pinned[1], NP = ctx->pinned[2];
    if (V >= 0xFFFFFFFFull) fail(ACC_E_CAP, "more than 2^32-1 (range txn, covered key) queries in one batch");
    ctx->stat("keydeps.range_key_queries", V);

    // ---- count and emit per piece with the exact-replay scan
    uint64_t *pe_cnt = ctx->get<uint64_t>("mx_pe_cnt", NP + 1);
    uint64_t *pe_off = ctx->get<uint64_t>("mx_pe_off", NP + 2);
    uint32_t *pk_cnt = ctx->get<uint32_t>("mx_pk_cnt", NP + 1);
    uint32_t *pk_off = ctx->get<uint32_t>("mx_pk_off", NP + 2);
    uint64_t *etoff = ctx->get<uint64_t>("mx_etoff", (size_t)n + 1);
    uint32_t *ktoff = ctx->get<uint32_t>("mx_ktoff", (size_t)n + 1);
    uint64_t Ex = 0, Kx = 0;
    CfkView v{};
    uint32_t *qc = ctx->get<uint32_t>("mx_qc", NP * 32);
    uint4 *prec = ctx->get<uint4>("mx_prec", 2 * NP + 2);
    if (NP) {
        const uint32_t pack = rbits <= 31;
        const bool defer = NP * 32 < 0xFFFFFFFFull;
        if (!cb.v1) {
            // with deferral and packed single results the exact-replay scan only ever runs on segments of two or more
            // entries (pcount / pdefer; pemit replays only lanes of two or more entries)
            cb.v1view = build_v1_cfk(ctx, cb, defer && pack);
            cb.v1 = true;
        }
        v = cb.v1view;
        launch(ctx, "mx_pieces", k_mx_pieces, dim3(grid_for(R, BLOCK)), dim3(BLOCK), 0, (uint32_t)R, (const uint64_t *)poff,
               (const uint32_t *)ra, (const uint32_t *)rowner, (const uint64_t *)rcnt, (const uint64_t *)r_off, rng_off,
               (const uint32_t *)cb.dict.rank, n, cb.tl, prec);
        const unsigned gcount = grid_for(NP * 32, BLOCK);
        const uint32_t dcap = ((gcount + MX_DSLOTS - 1) / MX_DSLOTS) * BLOCK;   // lanes of the blocks of one list
        uint32_t *dlist = defer ? ctx->get<uint32_t>("mx_dlist", (size_t)MX_DSLOTS * dcap) : nullptr;
        uint32_t *dcnt = ctx->get<uint32_t>("mx_dcnt", MX_DSLOTS);
        if (defer) ACC_HIP(hipMemsetAsync(dcnt, 0, MX_DSLOTS * sizeof(uint32_t), st));
        launch(ctx, "mx_pcount", k_mx_pcount, dim3(gcount), dim3(BLOCK), 0, NP, (const uint4 *)prec, v, pe_cnt, pk_cnt, qc, pack,
               dlist, dcnt, dcap);
        if (defer)
            launch(ctx, "mx_pdefer", k_mx_pdefer, dim3(8, MX_DSLOTS), dim3(BLOCK), 0, (const uint4 *)prec, v, (const uint32_t *)dlist,
                   (const uint32_t *)dcnt, dcap, pe_cnt, pk_cnt, qc, pack);
        scan<uint64_t, OpAdd<uint64_t>>(ctx, pe_cnt, pe_off, NP, true, pe_off + NP);
        scan<uint32_t, OpAdd<uint32_t>>(ctx, pk_cnt, pk_off, NP, true, pk_off + NP);
        ACC_HIP(hipMemcpyAsync(ctx->pinned, pe_off + NP, 8, hipMemcpyDeviceToHost, st));
        ACC_HIP(hipMemcpyAsync(ctx->pinned + 1, pk_off + NP, 4, hipMemcpyDeviceToHost, st));
        ctx->sync();
        Ex = ctx->pinned[0];
        Kx = ctx->pinned[1] & 0xFFFFFFFFull;
        if (Ex >= 0xFFFFFFFFull) fail(ACC_E_CAP, "more than 2^32-1 range-txn KeyDeps entries in one batch");
    } else {
        ACC_HIP(hipMemsetAsync(pe_off, 0, 8, st));
        ACC_HIP(hipMemsetAsync(pk_off, 0, 4, st));
    }
    launch(ctx, "mx_toff", k_mx_toff, dim3(grid_for((size_t)n + 1, BLOCK)), dim3(BLOCK), 0, n, rng_off, (const uint64_t *)poff,
           (const uint64_t *)pe_off, (const uint32_t *)pk_off, etoff, ktoff);
    MxE mx;
    mx.deps = ctx->get<uint32_t>("mx_deps", Ex + 1);
    mx.owner = ctx->get<uint32_t>("mx_owner", Ex + 1);
    mx.kx_idx = ctx->get<uint32_t>("mx_kx_idx", Kx + 1);
    mx.kx_end = ctx->get<uint32_t>("mx_kx_end", Kx + 1);
    mx.kx_code = ctx->get<uint64_t>("mx_kx_code", Kx + 1);
    uint32_t *ucnt = ctx->get<uint32_t>("mx_ucnt", (size_t)n + 1);
    uint32_t *idx_of_e = ctx->get<uint32_t>("mx_idx_of_e", Ex + 1);
    uint32_t *dep_scr = ctx->get<uint32_t>("mx_dep_scr", Ex + 1);
    MxU mu{ mx.deps, etoff, cb.dict.txn_of_rank, idx_of_e, dep_scr, ucnt };
    if (Ex) {
        launch(ctx, "mx_pemit", k_mx_pemit, dim3(grid_for(NP * 32, BLOCK)), dim3(BLOCK), 0, NP, (const uint4 *)prec,
               (const uint64_t *)seg_key, v, (const uint64_t *)pe_off, (const uint32_t *)pk_off, mx, (const uint32_t *)qc);
        // per-txn TxnId unions: wave / block tiers, or one (txn, rank) sort when some txn is beyond the block tier
        MxLists L;
        static const char *lnames[5] = { "mx_l16", "mx_l32", "mx_l64", "mx_mid_list", "mx_blk_list" };
        for (int k = 0; k < 5; ++k) L.l[k] = ctx->get<uint32_t>(lnames[k], n);
        uint32_t *const mid_list = L.l[3], *const blk_list = L.l[4];
        uint64_t *gst = ctx->get<uint64_t>("mx_gst", 6);
        ACC_HIP(hipMemsetAsync(gst, 0, 48, st));
        launch(ctx, "mx_route", k_mx_route, dim3(grid_for(n, (size_t)BLOCK * MX_RT)), dim3(BLOCK), 0, n, (const uint64_t *)etoff, L,
               gst);
        ACC_HIP(hipMemcpyAsync(ctx->pinned, gst, 48, hipMemcpyDeviceToHost, st));
        ctx->sync();
        const uint64_t nblk = ctx->pinned[0], nmid = ctx->pinned[2];
        const uint64_t nsmall[3] = { ctx->pinned[3], ctx->pinned[4], ctx->pinned[5] };
        ctx->stat("keydeps.range_block_txns", nblk);
        ctx->stat("keydeps.range_mid_txns", nmid);
        if (!ctx->pinned[1]) {
            if (nsmall[0])
                launch(ctx, "mx_union_s16", k_mx_union_seg<16>, dim3((unsigned)((nsmall[0] + 4 * WAVES - 1) / (4 * WAVES))),
                       dim3(BLOCK), 0, (const uint32_t *)L.l[0], (const uint64_t *)(gst + 3), mu);
            if (nsmall[1])
                launch(ctx, "mx_union_s32", k_mx_union_seg<32>, dim3((unsigned)((nsmall[1] + 2 * WAVES - 1) / (2 * WAVES))),
                       dim3(BLOCK), 0, (const uint32_t *)L.l[1], (const uint64_t *)(gst + 4), mu);
            if (nsmall[2])
                launch(ctx, "mx_union_s64", k_mx_union_seg<64>, dim3((unsigned)((nsmall[2] + WAVES - 1) / WAVES)),
                       dim3(BLOCK), 0, (const uint32_t *)L.l[2], (const uint64_t *)(gst + 5), mu);
            if (nmid)
                launch(ctx, "mx_union_mid", k_mx_union_mid, dim3((unsigned)((nmid + WAVES - 1) / WAVES)), dim3(BLOCK), 0,
                       (const uint32_t *)mid_list, (const uint64_t *)gst, mu);
            if (nblk)
                launch(ctx, "mx_union_block", k_mx_union_block, dim3((unsigned)nblk), dim3(BLOCK), 0,
                       (const uint32_t *)blk_list, (const uint64_t *)gst, mu);
        } else {
            const int tbits = bits_for(n);
            if (tbits + rbits > 64) fail(ACC_E_CAP, "batch too large for the (txn, TxnId rank) composite key");
            uint64_t *skey = ctx->get<uint64_t>("mx_skey", Ex);
            uint32_t *uflag = ctx->get<uint32_t>("mx_uflag", Ex + 1);
            uint32_t *ucum = ctx->get<uint32_t>("mx_ucum", Ex + 1);
            launch(ctx, "mx_owner", k_mx_owner, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, (const uint64_t *)etoff, mx.owner);
            launch(ctx, "mx_sortkeys", k_mx_sortkeys, dim3(grid_for(Ex, BLOCK)), dim3(BLOCK), 0, Ex, (const uint32_t *)mx.deps,
                   (const uint32_t *)mx.owner, rbits, skey);
            Sorted so = radix_sort(ctx, "mx_rs", skey, nullptr, Ex, tbits + rbits);
            launch(ctx, "mx_uflag", k_mx_uflag, dim3(grid_for(Ex, BLOCK)), dim3(BLOCK), 0, Ex, (const uint64_t *)so.keys, uflag);
            scan<uint32_t, OpAdd<uint32_t>>(ctx, uflag, ucum, Ex, true, ucum + Ex);
            launch(ctx, "mx_union_sorted", k_mx_union_sorted, dim3(grid_for(Ex, BLOCK)), dim3(BLOCK), 0, Ex,
                   (const uint64_t *)so.keys, (const uint32_t *)so.vals, (const uint32_t *)uflag, (const uint32_t *)ucum,
                   (const uint32_t *)mx.owner, rbits, mu);
            launch(ctx, "mx_ucnt_sorted", k_mx_ucnt_sorted, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, (const uint64_t *)etoff,
                   (const uint32_t *)ucum, ucnt);
        }
    }

    // ---- combined offsets and the combined layout
    MxKv mkv{ kv.arena_off, kv.kd_off, kv.u_off, kv.arena, kv.key_idx, kv.dep_txn };
    uint64_t *a_cnt = ctx->get<uint64_t>("mx_a_cnt", (size_t)n + 1);
    uint64_t *kd_cnt = ctx->get<uint64_t>("mx_kd_cnt", (size_t)n + 1);
    uint64_t *u_cnt = ctx->get<uint64_t>("mx_u_cnt", (size_t)n + 1);
    launch(ctx, "mx_sizes", k_mx_sizes, dim3(grid_for((size_t)n + 1, BLOCK)), dim3(BLOCK), 0, n, mkv, (const uint64_t *)etoff,
           (const uint32_t *)ktoff, (const uint32_t *)ucnt, a_cnt, kd_cnt, u_cnt);
    MxOut o;
    o.arena_off = ctx->get<uint64_t>("mx_arena_off", (size_t)n + 1);
    o.kd_off = ctx->get<uint64_t>("mx_kd_off", (size_t)n + 1);
    o.u_off = ctx->get<uint64_t>("mx_u_off", (size_t)n + 1);
    uint64_t *mtot = ctx->get<uint64_t>("mx_totals", 3);
    {   // the three combined offset arrays in one launch (over n + 1: the last element is each total), totals staged
        const uint64_t *si[3] = { a_cnt, kd_cnt, u_cnt };
        uint64_t *so[3] = { o.arena_off, o.kd_off, o.u_off }, *stot[3] = { mtot, mtot + 1, mtot + 2 };
        const size_t sn[3] = { (size_t)n + 1, (size_t)n + 1, (size_t)n + 1 };
        scan_multi<uint64_t, OpAdd<uint64_t>>(ctx, 3, si, so, sn, true, stot);
    }
    ACC_HIP(hipMemcpyAsync(ctx->pinned, mtot, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ctx->sync();
    const uint64_t TA = ctx->pinned[0], TK = ctx->pinned[1], TU = ctx->pinned[2];
    o.arena = ctx->get<int32_t>("mx_arena", TA + 1);
    o.key_idx = ctx->get<uint32_t>("mx_key_idx", TK + 1);
    o.kd_key = ctx->get<uint64_t>("mx_kd_key", TK + 1);
    o.dep_txn = ctx->get<uint32_t>("mx_dep_txn", TU + 1);
    launch(ctx, "mx_write", k_mx_write, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, mkv, (const uint64_t *)etoff,
           (const uint32_t *)ktoff, mx, (const uint32_t *)idx_of_e, (const uint32_t *)dep_scr, key_off, key_code, o);
    ctx->sync();
    *view = acc_keydeps_view{ n, TA, TK, TU, kv.total_edges + Ex, o.arena_off, o.arena, o.kd_off, o.key_idx, o.u_off,
                              o.dep_txn, o.kd_key };
    ctx->kd_view = *view;
    ctx->kd_valid = true;
}

}  // namespace acc
