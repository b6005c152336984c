// dictionary.hip — dense order ranks of composite keys (up to three u64 words compared unsigned, most significant
// first). Used wherever the reference compares objects the device cannot hold as one machine word:
//   * TxnId / Timestamp (Timestamp.compareTo, primitives/Timestamp.java:208-217) as (msb, lsb & IDENTITY_LSB,
//     node ^ 2^31), so equal rank <=> Timestamp.equals (:244-249);
//   * Range keys of RangeDeps (Range::compare, primitives/Range.java:310-317) as (start, end);
//   * u64 key codes whose varying bits leave no room for a group field in a composite sort key.
// Each word is bit-compacted to its varying bits (order preserving); the words are sorted by one LSD radix sort over
// the concatenation when it fits 64 bits, else word by word (least significant first, stable), then runs of equal
// keys get one rank. first[r] = the smallest input index of rank r (stable sort: the first occurrence).
//
// The second half is the front end the KeyDeps and RangeDeps paths share (dict.hpp): the prep pass (validation, the
// varying bits of every word, sortedness) and the order-rank dictionary of a batch's 2N timestamps, by the sorted-batch
// shortcut or the general sort (prep_dictionary, redo_general_dictionary, check_errors).
#include "dict.hpp"
#include "search.hpp"

namespace acc {

namespace {

constexpr int DMAXW = 3;

struct DWords {
    const uint64_t *w[DMAXW];
    uint64_t xor_mask[DMAXW];   // applied before compaction (sign flips of signed words), 0 = none
    uint64_t and_mask[DMAXW];   // identity masks (IDENTITY_LSB), ~0 = none
};

__device__ __forceinline__ uint64_t dword(const DWords &d, int k, size_t i)
{
    return (d.w[k][i] & d.and_mask[k]) ^ d.xor_mask[k];
}

// g[k] |= word_k(i) ^ word_k(0) over every i: the varying bits of each word
__global__ __launch_bounds__(BLOCK) void k_dict_masks(size_t n, DWords d, int nw, uint64_t *__restrict__ g)
{
    uint64_t m[DMAXW] = { 0, 0, 0 };
    uint64_t ref[DMAXW];
    for (int k = 0; k < nw; ++k) ref[k] = dword(d, k, 0);
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK)
        for (int k = 0; k < nw; ++k) m[k] |= dword(d, k, i) ^ ref[k];
    __shared__ uint64_t part[WAVES][DMAXW];
    for (int k = 0; k < DMAXW; ++k) {
        uint64_t x = m[k];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) x |= shfl_xor(x, s);
        if (lane_id() == 0) part[threadIdx.x >> 6][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)nw) {
        uint64_t x = 0;
        for (int q = 0; q < WAVES; ++q) x |= part[q][threadIdx.x];
        if (x) atomicOr((unsigned long long *)&g[threadIdx.x], (unsigned long long)x);
    }
}

struct DPlan {
    Runs r[DMAXW];
    int shift[DMAXW];   // position of word k in the single composite (when it fits 64 bits)
};

// composite of every compacted word (sel < 0), or word `sel` alone, optionally gathered through perm
__global__ __launch_bounds__(BLOCK) void k_dict_compact(size_t n, DWords d, int nw, DPlan p, int sel, const uint32_t *__restrict__ perm,
                                                        uint64_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t src = perm ? perm[i] : i;
    if (sel >= 0) { out[i] = pext_runs(dword(d, sel, src), p.r[sel]); return; }
    uint64_t c = 0;
    for (int k = 0; k < nw; ++k)
        if (p.r[k].bits) c |= pext_runs(dword(d, k, src), p.r[k]) << p.shift[k];
    out[i] = c;
}

// flag[i] = sorted key i differs from sorted key i-1
__global__ __launch_bounds__(BLOCK) void k_dict_flags(size_t n, const uint64_t *__restrict__ sorted_single, const uint32_t *__restrict__ perm,
                                                      DWords d, int nw, uint32_t *__restrict__ flag)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t f = 1;
    if (i > 0) {
        if (sorted_single) f = sorted_single[i] != sorted_single[i - 1];
        else {
            const uint32_t a = perm[i], b = perm[i - 1];
            f = 0;
            for (int k = 0; k < nw; ++k) f |= dword(d, k, a) != dword(d, k, b);
        }
    }
    flag[i] = f;
}

__global__ __launch_bounds__(BLOCK) void k_dict_scatter(size_t n, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ flag,
                                                        const uint32_t *__restrict__ incl, uint32_t *__restrict__ rank,
                                                        uint32_t *__restrict__ first, uint64_t *__restrict__ count)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = perm[i], r = incl[i] - 1;
    rank[src] = r;
    if (first && flag[i]) first[r] = src;
    if (i == n - 1) *count = incl[i];
}

}  // namespace

DenseRank dense_rank(acc_ctx *ctx, const char *tag, size_t n, int nw, const uint64_t *const *words, const uint64_t *and_mask,
                     const uint64_t *xor_mask, bool want_first)
{
    if (nw < 1 || nw > DMAXW) fail(ACC_E_STATE, "internal: dense_rank supports 1..3 words");
    if (n >= 0xFFFFFFFFull) fail(ACC_E_CAP, "dictionary too large (>= 2^32 keys)");
    hipStream_t st = ctx->stream;
    char nm[64];
    auto name = [&](const char *s) { snprintf(nm, sizeof nm, "%s.%s", tag, s); return nm; };
    DenseRank out;
    out.rank = ctx->get<uint32_t>(name("rank"), n);
    out.first = want_first ? ctx->get<uint32_t>(name("first"), n) : nullptr;
    out.count_dev = ctx->get<uint64_t>(name("count"), 1);
    if (n == 0) {
        ACC_HIP(hipMemsetAsync(out.count_dev, 0, 8, st));
        out.count = 0;
        return out;
    }
    DWords d{};
    for (int k = 0; k < DMAXW; ++k) {
        d.w[k] = k < nw ? words[k] : nullptr;
        d.and_mask[k] = (k < nw && and_mask) ? and_mask[k] : ~0ull;
        d.xor_mask[k] = (k < nw && xor_mask) ? xor_mask[k] : 0ull;
    }
    uint64_t *g = ctx->get<uint64_t>(name("masks"), DMAXW);
    ACC_HIP(hipMemsetAsync(g, 0, DMAXW * 8, st));
    launch(ctx, "dict_masks", k_dict_masks, dim3(std::min<unsigned>(grid_for(n, BLOCK), 1024u)), dim3(BLOCK), 0, n, d, nw, g);
    ACC_HIP(hipMemcpyAsync(ctx->pinned + 32, g, DMAXW * 8, hipMemcpyDeviceToHost, st));
    ctx->sync();
    DPlan p{};
    int total = 0;
    for (int k = nw - 1; k >= 0; --k) {
        p.r[k] = make_runs(ctx->pinned[32 + k]);
        p.shift[k] = total;
        total += p.r[k].bits;
    }
    const unsigned gn = grid_for(n, BLOCK);
    uint32_t *flag = ctx->get<uint32_t>(name("flag"), n);
    uint32_t *incl = ctx->get<uint32_t>(name("incl"), n);
    const uint32_t *perm;
    if (total <= 64) {
        uint64_t *ck = ctx->get<uint64_t>(name("ckey"), n);
        launch(ctx, "dict_compact", k_dict_compact, dim3(gn), dim3(BLOCK), 0, n, d, nw, p, -1, (const uint32_t *)nullptr, ck);
        Sorted s = radix_sort(ctx, name("rs"), ck, nullptr, n, total);
        perm = s.vals;
        launch(ctx, "dict_flags", k_dict_flags, dim3(gn), dim3(BLOCK), 0, n, (const uint64_t *)s.keys, (const uint32_t *)nullptr,
               d, nw, flag);
    } else {
        // stable LSD over the words, least significant first; each pass gathers its word through the running order
        uint64_t *wk = ctx->get<uint64_t>(name("wkey"), n);
        uint32_t *pb = ctx->get<uint32_t>(name("perm"), n);
        const uint32_t *cur = nullptr;
        for (int k = nw - 1; k >= 0; --k) {
            if (!p.r[k].bits) continue;
            launch(ctx, "dict_compact", k_dict_compact, dim3(gn), dim3(BLOCK), 0, n, d, nw, p, k, cur, wk);
            Sorted s = radix_sort(ctx, name("rs"), wk, cur, n, p.r[k].bits);
            ACC_HIP(hipMemcpyAsync(pb, s.vals, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
            cur = pb;
        }
        perm = cur;
        launch(ctx, "dict_flags", k_dict_flags, dim3(gn), dim3(BLOCK), 0, n, (const uint64_t *)nullptr, perm, d, nw, flag);
    }
    scan<uint32_t, OpAdd<uint32_t>>(ctx, flag, incl, n, false);
    launch(ctx, "dict_scatter", k_dict_scatter, dim3(gn), dim3(BLOCK), 0, n, perm, (const uint32_t *)flag, (const uint32_t *)incl,
           out.rank, out.first, out.count_dev);
    out.count = ~0ull;   // on device until the caller's next sync (count_dev)
    out.perm = perm;
    return out;
}

// ---------------------------------------------------------------- prep: validation and the timestamp dictionary

struct TsPlan {
    Runs r0, r1, r2;
    int b0, b1, b2;
};

// g[0..2] ts word masks, g[3] key mask, g[4] error bits, g[5] batch-not-in-TxnId-order flag.
// Block-level OR (wave shuffles, then LDS across waves) and ONE atomic per block and word: same-address
// atomics from every wave serialise at the L2 (1.4 ms for 8M pairs in the first build).
template <int NW>
__device__ __forceinline__ void block_or_n(uint64_t (&v)[NW], uint64_t *dst)
{
    __shared__ uint64_t part[WAVES][NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        uint64_t x = v[w];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x |= shfl_idx(x, (int)(lane_id() ^ d));
        if (lane_id() == 0) part[threadIdx.x >> 6][w] = x;
    }
    __syncthreads();
    if (threadIdx.x < NW) {
        uint64_t x = 0;
#pragma unroll
        for (int q = 0; q < WAVES; ++q) x |= part[q][threadIdx.x];
        if (x) atomicOr((unsigned long long *)&dst[threadIdx.x], (unsigned long long)x);
    }
}

// Per txn: executeAt != TxnId flags, varying-bit masks, status / kind checks, TxnId order; per pair (a chunk's txns'
// pairs are one contiguous range, walked coalesced with each pair's txn found in the chunk's key offsets in LDS):
// owner[], key order within a txn (Keys.ofSortedUnique), the key-code varying-bit mask. Pair indices are bounded by P
// (a malformed key_off is reported, never followed out of bounds). One chunk of BLOCK txns per block (full occupancy:
// a few resident blocks per CU left every chunk's HBM round trips exposed, 0.11 ms for config 2); each block folds its
// words into one of PREP_SLOTS slot rows of g (same-address atomics serialise at the L2) and the host ORs the rows
// (words 0-6) or adds them up (7: the bumped txns; 8: the keys of the bumped committed txns, ts.hpp).

__global__ __launch_bounds__(BLOCK) void k_prep_txn(uint32_t n, size_t P, const uint64_t *__restrict__ tm, const uint64_t *__restrict__ tl,
                                                    const int32_t *__restrict__ tn, const uint64_t *__restrict__ em,
                                                    const uint64_t *__restrict__ el, const int32_t *__restrict__ en,
                                                    const uint8_t *__restrict__ status, const uint32_t *__restrict__ key_off,
                                                    const uint64_t *__restrict__ key_code, uint32_t *__restrict__ owner,
                                                    uint32_t *__restrict__ bflag, uint64_t *__restrict__ g)
{
    __shared__ uint32_t ko[BLOCK + 1];
    const uint32_t tid = threadIdx.x;
    uint64_t m0 = 0, m1 = 0, m2 = 0, km = 0, errs = 0, unsorted = 0, ornk = 0;
    uint32_t differs = 0;
    unsigned long long bckeys = 0;
    const uint64_t r0 = tm[0], r1 = ts_w1(tl[0]), r2 = ts_w2(tn[0]);
    const uint64_t kref = P ? key_code[0] : 0;
    if (blockIdx.x == 0 && tid == 0 && key_off[n] != P) errs |= ERR_KEY_TOTAL;
    for (uint32_t t0 = blockIdx.x * BLOCK; t0 < n; t0 += gridDim.x * BLOCK) {
        const uint32_t t = t0 + tid;
        const uint32_t tcnt = min((uint32_t)BLOCK, n - t0);
        __syncthreads();   // the previous chunk's ko[] readers are done
        if (tid < tcnt) ko[tid] = key_off[t];
        if (tid == 0) ko[tcnt] = key_off[t0 + tcnt];
        bool bc = false;
        if (t < n) {
            // executeAt != txnId (Timestamp.equals): these are the only executeAts the sorted-batch
            // dictionary has to sort
            const bool d = tm[t] != em[t] || ts_w1(tl[t]) != ts_w1(el[t]) || tn[t] != en[t];
            differs += d;
            bflag[t] = (uint32_t)d;
            m0 |= (tm[t] ^ r0) | (em[t] ^ r0);
            m1 |= (ts_w1(tl[t]) ^ r1) | (ts_w1(el[t]) ^ r1);
            m2 |= (ts_w2(tn[t]) ^ r2) | (ts_w2(en[t]) ^ r2);
            if (status[t] > 7) errs |= ERR_BAD_STATUS;
            uint32_t kind = (uint32_t)(tl[t] >> 1) & 7u;
            if (kind >= 6) errs |= ERR_BAD_KIND;
            else if (kind == 5) errs |= ERR_LOCAL_ONLY;
            bc = bumped_committed(status[t], kind, d);
            if (t + 1 < n && ts_cmp(tm[t], tl[t], tn[t], tm[t + 1], tl[t + 1], tn[t + 1]) >= 0) unsorted = 1;
        }
        __syncthreads();
        const bool bad = tid < tcnt && ko[tid + 1] < ko[tid];
        if (bad) errs |= ERR_KEY_OFF;
        else if (tid < tcnt) {
            ornk |= ko[tid + 1] - ko[tid];   // bounds the keys per txn (pair packing)
            if (bc) bckeys += ko[tid + 1] - ko[tid];
        }
        if (!__syncthreads_or(bad ? 1 : 0) && P) {
            const uint32_t a = (uint32_t)min((size_t)ko[0], P), b = (uint32_t)min((size_t)ko[tcnt], P);
            for (uint32_t j = a + tid; j < b; j += BLOCK) {
                const uint32_t lo = seg_of(ko, tcnt, j);   // last txn i with ko[i] <= j (empty txns share their offset with the next)
                owner[j] = t0 + lo;
                const uint64_t kc = key_code[j];
                km |= kc ^ kref;
                if (j > ko[lo] && key_code[j - 1] >= kc) errs |= ERR_KEYS_UNSORTED;
            }
        }
    }
    uint64_t *gs = g + PREP_ROW * (blockIdx.x % PREP_SLOTS);
    uint64_t v[7] = { m0, m1, m2, km, errs, unsorted, ornk };
    block_or_n<7>(v, gs);
    __shared__ uint32_t s_nd;
    __shared__ unsigned long long s_bck;
    if (tid == 0) { s_nd = 0; s_bck = 0; }
    __syncthreads();
    if (differs) atomicAdd(&s_nd, differs);
    if (bckeys) atomicAdd(&s_bck, bckeys);
    __syncthreads();
    if (tid == 0 && s_nd) atomicAdd((unsigned long long *)&gs[7], (unsigned long long)s_nd);
    if (tid == 0 && s_bck) atomicAdd((unsigned long long *)&gs[8], s_bck);
}

// ---- sorted-batch dictionary: TxnIds are already in order; only the differing executeAts (B) are sorted.
// rank(txnId_t) = t + |{b in B : b < txnId_t}|, rank(b_k) = k + |{txnIds < b_k}|; exact dense ranks when no
// executeAt equals another timestamp (checked here; otherwise the general sort recomputes them).
__global__ __launch_bounds__(BLOCK) void k_b_compact(uint32_t n, const uint32_t *__restrict__ bflag, const uint32_t *__restrict__ bidx,
                                                     const uint64_t *__restrict__ em, const uint64_t *__restrict__ el,
                                                     const int32_t *__restrict__ en, const uint64_t *__restrict__ tm,
                                                     const uint64_t *__restrict__ tl, const int32_t *__restrict__ tn,
                                                     TsPlan plan, uint64_t *__restrict__ bkey, uint32_t *__restrict__ bsrc,
                                                     uint64_t *__restrict__ tkey)
{
    uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n) return;
    uint64_t c0 = pext_runs(tm[t], plan.r0), c1 = pext_runs(ts_w1(tl[t]), plan.r1), c2 = pext_runs(ts_w2(tn[t]), plan.r2);
    tkey[t] = (plan.b0 ? (c0 << (plan.b1 + plan.b2)) : 0) | (plan.b1 ? (c1 << plan.b2) : 0) | c2;
    if (bflag[t]) {
        c0 = pext_runs(em[t], plan.r0); c1 = pext_runs(ts_w1(el[t]), plan.r1); c2 = pext_runs(ts_w2(en[t]), plan.r2);
        uint32_t b = bidx[t];
        bkey[b] = (plan.b0 ? (c0 << (plan.b1 + plan.b2)) : 0) | (plan.b1 ? (c1 << plan.b2) : 0) | c2;
        bsrc[b] = t;
    }
}

__global__ __launch_bounds__(BLOCK) void k_rank_txn_sorted(uint32_t n, uint32_t nb, const uint64_t *__restrict__ tkey,
                                                           const uint64_t *__restrict__ sb, const uint32_t *__restrict__ bflag,
                                                           uint32_t *__restrict__ rank, uint32_t *__restrict__ txn_of_rank,
                                                           uint64_t *__restrict__ g)
{
    uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    uint64_t tie = 0;
    if (t < n) {
        uint32_t lb = lower_bound(sb, 0, nb, tkey[t]);
        if (lb < nb && sb[lb] == tkey[t]) tie = 1;
        uint32_t r = t + lb;
        rank[t] = r;
        txn_of_rank[r] = t;
        if (!bflag[t]) rank[n + t] = r;
    }
    uint64_t v[1] = { tie };
    block_or_n<1>(v, g + 6);
}

__global__ __launch_bounds__(BLOCK) void k_rank_b_sorted(uint32_t n, uint32_t nb, const uint64_t *__restrict__ tkey,
                                                         const uint64_t *__restrict__ sb, const uint32_t *__restrict__ sperm,
                                                         const uint32_t *__restrict__ bsrc, uint32_t *__restrict__ rank,
                                                         uint64_t *__restrict__ g)
{
    uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    uint64_t tie = 0;
    if (k < nb) {
        if (k > 0 && sb[k] == sb[k - 1]) tie = 1;
        uint32_t t = bsrc[sperm[k]];
        rank[n + t] = k + lower_bound(tkey, 0, n, sb[k]);
    }
    uint64_t v[1] = { tie };
    block_or_n<1>(v, g + 6);
}

// ---------------------------------------------------------------- dictionary (order ranks)

// i < N: TxnId of txn i; i >= N: executeAt of txn i-N. word_sel < 0: whole compacted key (fits 64 bits);
// else the compaction of that single word.
__global__ __launch_bounds__(BLOCK) void k_ts_compact(uint32_t n, const uint64_t *__restrict__ tm, const uint64_t *__restrict__ tl,
                                                      const int32_t *__restrict__ tn, const uint64_t *__restrict__ em,
                                                      const uint64_t *__restrict__ el, const int32_t *__restrict__ en,
                                                      TsPlan plan, int word_sel, const uint32_t *__restrict__ perm,
                                                      uint64_t *__restrict__ out)
{
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= 2 * (size_t)n) return;
    size_t src = perm ? perm[i] : i;
    uint32_t t = (uint32_t)(src < n ? src : src - n);
    bool is_exec = src >= n;
    uint64_t w0 = is_exec ? em[t] : tm[t];
    uint64_t w1 = ts_w1(is_exec ? el[t] : tl[t]);
    uint64_t w2 = ts_w2(is_exec ? en[t] : tn[t]);
    uint64_t c0 = pext_runs(w0, plan.r0), c1 = pext_runs(w1, plan.r1), c2 = pext_runs(w2, plan.r2);
    uint64_t k;
    if (word_sel < 0) k = (plan.b0 ? (c0 << (plan.b1 + plan.b2)) : 0) | (plan.b1 ? (c1 << plan.b2) : 0) | c2;
    else k = word_sel == 0 ? c0 : word_sel == 1 ? c1 : c2;
    out[i] = k;
}

// flag[i] = sorted key i differs from key i-1 (all compacted words compared).
__global__ __launch_bounds__(BLOCK) void k_rank_flags(size_t m, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ c0,
                                                      const uint64_t *__restrict__ c1, const uint64_t *__restrict__ c2,
                                                      const uint64_t *__restrict__ sorted_single, uint32_t *__restrict__ flag)
{
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    uint32_t f = 1;
    if (i > 0) {
        if (sorted_single) f = sorted_single[i] != sorted_single[i - 1];
        else {
            uint32_t a = perm[i], b = perm[i - 1];
            f = (c0[a] != c0[b]) || (c1[a] != c1[b]) || (c2[a] != c2[b]);
        }
    }
    flag[i] = f;
}

// rank[src] = inclusive(flag) - 1 (equal Timestamps share a rank); txn_of_rank for TxnId entries.
__global__ __launch_bounds__(BLOCK) void k_rank_scatter(size_t m, uint32_t n, const uint32_t *__restrict__ perm,
                                                        const uint32_t *__restrict__ incl, uint32_t *__restrict__ rank,
                                                        uint32_t *__restrict__ txn_of_rank)
{
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    uint32_t src = perm[i];
    uint32_t r = incl[i] - 1;
    rank[src] = r;
    if (src < n) txn_of_rank[r] = src;
}

// Count TxnId entries per rank to detect duplicate TxnIds (CommandsForKey txns are sorted unique).
__global__ __launch_bounds__(BLOCK) void k_dup_txn(uint32_t n, const uint32_t *__restrict__ rank, uint32_t *__restrict__ seen,
                                                   uint64_t *__restrict__ g)
{
    uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    uint64_t err = 0;
    if (t < n) {
        if (atomicAdd(&seen[rank[t]], 1u) != 0) err = ERR_DUP_TXNID;
    }
    uint64_t v[1] = { err };
    block_or_n<1>(v, g + 4);
}

// g[6] != 0: some executeAt compares equal to another txn's TxnId or executeAt. Only then can two
// committed entries of one key tie on executeAt, where the FAST bisection's pick (CommandsForKey.java:619)
// is order-dependent; such batches take the exact replay path (v1).
__global__ __launch_bounds__(BLOCK) void k_exec_ties(uint32_t n, const uint32_t *__restrict__ rank, uint32_t *__restrict__ seen,
                                                     uint64_t *__restrict__ g)
{
    uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    uint64_t tie = 0;
    if (t < n && rank[n + t] != rank[t]) {
        if (atomicAdd(&seen[rank[n + t]], 1u) != 0) tie = 1;
    }
    uint64_t v[1] = { tie };
    block_or_n<1>(v, g + 6);
}

// ---------------------------------------------------------------- host orchestration

void check_errors(uint64_t errs)
{
    if (errs & ERR_KEY_TOTAL) fail(ACC_E_ARG, "key_off[n_txn] must equal n_pairs");
    if (errs & ERR_BAD_STATUS) fail(ACC_E_ARG, "invalid InternalStatus ordinal (> INVALID_OR_TRUNCATED)");
    if (errs & ERR_BAD_KIND) fail(ACC_E_ARG, "Kind.ofOrdinal: invalid kind ordinal in TxnId flags");
    if (errs & ERR_KEY_OFF) fail(ACC_E_ARG, "key_off must be non-decreasing");
    if (errs & ERR_KEYS_UNSORTED) fail(ACC_E_ARG, "keys of a txn must be sorted and unique (Keys.ofSortedUnique)");
    if (errs & ERR_DUP_TXNID) fail(ACC_E_ARG, "TxnIds of a batch must be distinct (CommandsForKey txns are sorted unique)");
    if (errs & ERR_LOCAL_ONLY) fail(ACC_E_STATE, "Kind.witnesses(): unhandled kind LocalOnly (AssertionError)");
}

// The general dictionary: a compacted LSD radix sort of all 2N timestamps (multi-word beyond 64 varying bits), dense
// ranks by a flag scan, duplicate-TxnId and executeAt-tie checks (g[4], g[6]).
static void general_ranks(acc_ctx *ctx, uint32_t n, const uint64_t *tm, const uint64_t *tl, const int32_t *tn,
                          const uint64_t *em, const uint64_t *el, const int32_t *en, const TsPlan &plan, uint64_t *g,
                          uint32_t *rank, uint32_t *txn_of_rank)
{
    hipStream_t st = ctx->stream;
    const size_t m = 2 * (size_t)n;
    uint32_t *flag = ctx->get<uint32_t>("rank_flag", m);
    uint32_t *incl = ctx->get<uint32_t>("rank_incl", m);
    const unsigned gm = grid_for(m, BLOCK);
    Sorted ts_sorted;
    if (plan.b0 + plan.b1 + plan.b2 <= 64) {
        uint64_t *ck = ctx->get<uint64_t>("ts_ckey", m);
        launch(ctx, "ts_compact", k_ts_compact, dim3(gm), dim3(BLOCK), 0, n, tm, tl, tn, em, el, en, plan, -1,
               (const uint32_t *)nullptr, ck);
        ts_sorted = radix_sort(ctx, "rs_ts", ck, nullptr, m, plan.b0 + plan.b1 + plan.b2);
        launch(ctx, "rank_flags", k_rank_flags, dim3(gm), dim3(BLOCK), 0, m, (const uint32_t *)ts_sorted.vals,
               (const uint64_t *)nullptr, (const uint64_t *)nullptr, (const uint64_t *)nullptr,
               (const uint64_t *)ts_sorted.keys, flag);
    } else {
        // multi-word LSD: node word, then lsb word, then msb word (each only over its varying bits)
        uint64_t *c[3] = { ctx->get<uint64_t>("ts_c0", m), ctx->get<uint64_t>("ts_c1", m), ctx->get<uint64_t>("ts_c2", m) };
        for (int w = 0; w < 3; ++w)
            launch(ctx, "ts_compact", k_ts_compact, dim3(gm), dim3(BLOCK), 0, n, tm, tl, tn, em, el, en, plan, w,
                   (const uint32_t *)nullptr, c[w]);
        uint64_t *tmpk = ctx->get<uint64_t>("ts_tmpk", m);
        uint32_t *permb = ctx->get<uint32_t>("ts_perm", m);
        const uint32_t *perm = nullptr;
        const int wbits[3] = { plan.b0, plan.b1, plan.b2 };
        for (int w = 2; w >= 0; --w) {
            const uint64_t *keys = c[w];
            if (perm) {
                launch(ctx, "ts_compact", k_ts_compact, dim3(gm), dim3(BLOCK), 0, n, tm, tl, tn, em, el, en, plan, w,
                       perm, tmpk);
                keys = tmpk;
            }
            Sorted s = radix_sort(ctx, "rs_ts", keys, perm, m, wbits[w]);
            ACC_HIP(hipMemcpyAsync(permb, s.vals, m * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
            perm = permb;
        }
        ts_sorted = { nullptr, permb };
        launch(ctx, "rank_flags", k_rank_flags, dim3(gm), dim3(BLOCK), 0, m, (const uint32_t *)permb,
               (const uint64_t *)c[0], (const uint64_t *)c[1], (const uint64_t *)c[2], (const uint64_t *)nullptr, flag);
    }
    scan<uint32_t, OpAdd<uint32_t>>(ctx, flag, incl, m, false);
    launch(ctx, "rank_scatter", k_rank_scatter, dim3(gm), dim3(BLOCK), 0, m, n, (const uint32_t *)ts_sorted.vals,
           (const uint32_t *)incl, rank, txn_of_rank);
    uint32_t *seen = ctx->get<uint32_t>("dup_seen", m);
    ACC_HIP(hipMemsetAsync(seen, 0, m * sizeof(uint32_t), st));
    launch(ctx, "dup_txn", k_dup_txn, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, (const uint32_t *)rank, seen, g);
    launch(ctx, "exec_ties", k_exec_ties, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, (const uint32_t *)rank, seen, g);
}

static TsPlan ts_plan(const uint64_t *hg)
{
    TsPlan plan;
    plan.r0 = make_runs(hg[0]); plan.r1 = make_runs(hg[1]); plan.r2 = make_runs(hg[2]);
    plan.b0 = plan.r0.bits; plan.b1 = plan.r1.bits; plan.b2 = plan.r2.bits;
    return plan;
}

// A batch whose sorted-batch dictionary met an executeAt tie (g[6], found after the caller's next sync when the check
// was deferred): the general dictionary instead, in place (same rank buffers). g[6] is then the exact-tie flag.
void redo_general_dictionary(acc_ctx *ctx, uint32_t n, const uint64_t *tm, const uint64_t *tl, const int32_t *tn,
                             const uint64_t *em, const uint64_t *el, const int32_t *en, uint64_t *g, Dictionary &d)
{
    ACC_HIP(hipMemsetAsync(g + 6, 0, sizeof(uint64_t), ctx->stream));
    general_ranks(ctx, n, tm, tl, tn, em, el, en, ts_plan(d.hg), g, d.rank, d.txn_of_rank);
    d.fast = false;
    d.ties_pending = false;
    ctx->stat("keydeps.fast_dictionary", 0);
}

// Validation (k_prep_txn: statuses, kinds, key order, TxnId order) and the order-rank dictionary of the 2N
// timestamps (rank[t] = TxnId of t, rank[n + t] = executeAt of t; equal <=> Timestamp.equals). Shared by the
// KeyDeps and RangeDeps paths. Throws the first validation error. defer_ties: the sorted-batch dictionary's tie check
// (g[6]) is left to the caller's next sync (out.ties_pending), which then calls redo_general_dictionary on a tie.
//
// prep_batch: the prep pass and its host sync. The rank arrays are allocated here, so the kernels a caller enqueues
// before build_dictionary can already take their addresses.
void prep_batch(acc_ctx *ctx, uint32_t n, size_t P, const uint64_t *tm, const uint64_t *tl, const int32_t *tn,
                const uint64_t *em, const uint64_t *el, const int32_t *en, const uint8_t *status, const uint32_t *key_off,
                const uint64_t *key_code, uint32_t *owner, uint64_t *g, Dictionary &out)
{
    hipStream_t st = ctx->stream;
    static_assert(PREP_ROW * PREP_SLOTS <= acc_ctx::PINNED_WORDS - acc_ctx::PINNED_SLOTS, "slot rows fit the pinned area");
    static_assert(PREP_G_WORDS == 8 + PREP_ROW * PREP_SLOTS, "g and the prep slots share one buffer");
    static_assert(PREP_ROW >= 9, "seven OR words and two sums per slot row");
    uint64_t *gslots = g + 8;   // g has PREP_G_WORDS words
    ACC_HIP(hipMemsetAsync(g, 0, PREP_G_WORDS * sizeof(uint64_t), st));
    uint32_t *bflag = ctx->get<uint32_t>("bflag", n);
    launch(ctx, "prep_txn", k_prep_txn, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, P, tm, tl, tn, em, el, en, status,
           key_off, key_code, owner, bflag, gslots);
    uint64_t hg[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, nbc = 0;
    {
        // (key_off[n] == P is checked by the kernel: ERR_KEY_TOTAL)
        uint64_t *hs = ctx->pinned + acc_ctx::PINNED_SLOTS;
        ACC_HIP(hipMemcpyAsync(hs, gslots, PREP_ROW * PREP_SLOTS * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        ctx->sync();
        for (uint32_t r = 0; r < PREP_SLOTS; ++r) {
            for (int w = 0; w < 7; ++w) hg[w] |= hs[PREP_ROW * r + w];
            hg[7] += hs[PREP_ROW * r + 7];
            nbc += hs[PREP_ROW * r + 8];
        }
    }
    check_errors(hg[4]);
    const TsPlan plan = ts_plan(hg);
    const size_t m = 2 * (size_t)n;
    out.rank = ctx->get<uint32_t>("rank", m);
    out.txn_of_rank = ctx->get<uint32_t>("txn_of_rank", m);
    out.rbits = bits_for(m - 1);
    out.batch_sorted = hg[5] == 0;
    out.fast_ok = out.batch_sorted && plan.b0 + plan.b1 + plan.b2 <= 64 && hg[7] < n;
    out.fast = false;
    out.ties_pending = false;
    out.nbc = nbc;
    out.nb = 0;
    out.sb_vals = out.bsrc = nullptr;
    memcpy(out.hg, hg, sizeof hg);
}

// build_dictionary: order ranks over the 2N timestamps of a batch prep_batch has passed. Enqueued on ctx->cur(); the
// sorted-batch dictionary with defer_ties has no host sync, so it can run on the side lane (the other cases use the
// context stream: the general sort and the undeferred tie check sync it).
void build_dictionary(acc_ctx *ctx, uint32_t n, const uint64_t *tm, const uint64_t *tl, const int32_t *tn,
                      const uint64_t *em, const uint64_t *el, const int32_t *en, uint64_t *g, Dictionary &out, bool defer_ties)
{
    const TsPlan plan = ts_plan(out.hg);
    uint32_t *rank = out.rank, *txn_of_rank = out.txn_of_rank;
    const uint64_t nb = out.hg[7];
    bool fast_dict = out.fast_ok;
    if (ctx->launch_stream && !(fast_dict && defer_ties)) fail(ACC_E_STATE, "internal: this dictionary syncs the context stream");
    out.ties_pending = false;
    if (fast_dict) {
        const uint32_t *bflag = ctx->get<uint32_t>("bflag", n);
        uint32_t *bidx = ctx->get<uint32_t>("bidx", (size_t)n + 1);
        scan<uint32_t, OpAdd<uint32_t>>(ctx, bflag, bidx, n, true, bidx + n);
        uint64_t *bkey = ctx->get<uint64_t>("bkey", nb);
        uint32_t *bsrc = ctx->get<uint32_t>("bsrc", nb);
        uint64_t *tkey = ctx->get<uint64_t>("tkey", n);
        launch(ctx, "b_compact", k_b_compact, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, (const uint32_t *)bflag,
               (const uint32_t *)bidx, em, el, en, tm, tl, tn, plan, bkey, bsrc, tkey);
        Sorted sb = radix_sort(ctx, "rs_b", bkey, nullptr, nb, plan.b0 + plan.b1 + plan.b2);
        launch(ctx, "rank_txn_sorted", k_rank_txn_sorted, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, (uint32_t)nb,
               (const uint64_t *)tkey, (const uint64_t *)sb.keys, (const uint32_t *)bflag, rank, txn_of_rank, g);
        launch(ctx, "rank_b_sorted", k_rank_b_sorted, dim3(grid_for(nb, BLOCK)), dim3(BLOCK), 0, n, (uint32_t)nb,
               (const uint64_t *)tkey, (const uint64_t *)sb.keys, (const uint32_t *)sb.vals, (const uint32_t *)bsrc, rank, g);
        out.nb = (uint32_t)nb;
        out.sb_vals = sb.vals;
        out.bsrc = bsrc;
        if (defer_ties) {
            out.ties_pending = true;
        } else {
            hipStream_t st = ctx->stream;
            ACC_HIP(hipMemcpyAsync(ctx->pinned, g + 6, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
            ctx->sync();
            if (ctx->pinned[0]) {   // an executeAt equals another timestamp: dense ranks need the general dictionary
                ACC_HIP(hipMemsetAsync(g + 6, 0, sizeof(uint64_t), st));
                fast_dict = false;
            }
        }
    }
    if (!fast_dict) general_ranks(ctx, n, tm, tl, tn, em, el, en, plan, g, rank, txn_of_rank);
    ctx->stat("keydeps.fast_dictionary", fast_dict ? 1 : 0);
    out.fast = fast_dict;
}

void prep_dictionary(acc_ctx *ctx, uint32_t n, size_t P, const uint64_t *tm, const uint64_t *tl, const int32_t *tn,
                     const uint64_t *em, const uint64_t *el, const int32_t *en, const uint8_t *status,
                     const uint32_t *key_off, const uint64_t *key_code, uint32_t *owner, uint64_t *g, Dictionary &out,
                     bool defer_ties)
{
    prep_batch(ctx, n, P, tm, tl, tn, em, el, en, status, key_off, key_code, owner, g, out);
    build_dictionary(ctx, n, tm, tl, tn, em, el, en, g, out, defer_ties);
}

}  // namespace acc
