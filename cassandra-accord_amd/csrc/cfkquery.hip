// cfkquery.hip — acc_cfk_keydeps: PreAccept.calculatePartialDeps' key half for a batch of NEW transactions against the
// resident CommandsForKey store (messages/PreAccept.java:107-138, 245-265 -> impl/InMemoryCommandStore.java:257-292 ->
// CommandsForKey.mapReduceActive, local/CommandsForKey.java:614-650). The reference computes deps for the incoming txn
// against the live CommandsForKey and recomputes nothing for stored txns; so does this: the store's key-major segments
// (acc_cfk::km, cfk.hip) are scanned in place, no (key, TxnId) pair of the store is sorted and no segment is rebuilt.
// Work = the queries' (query, key) pairs + the segment prefixes (entries with TxnId < executeAt) they read.
//
//   1. validate   per query: kind, domain, offsets, keys sorted unique (before anything indexes by them)
//   2. locate     per pair: the key's segment (binary search of km.key), end = first entry with TxnId >= S = executeAt
//                 (binary search of the segment's TxnId columns), its 256-entry chunks
//   3. max        one wave per chunk (its pair read from a chunk -> pair map): M = the largest executeAt < S among
//                 COMMITTED / STABLE / APPLIED Writes of the prefix (closed form of the FAST bisection + the walk down
//                 to a Write) and the count of committed entries whose executeAt compares equal to S; pairs of several
//                 chunks fold their chunks' partials (one wave per pair). Two or more ties: ACC_E_STATE (the bisection
//                 could land on either).
//   4. count      entries the map function emits: a pair of one chunk (a short prefix, the common case) by the wave
//                 that just found its M, the chunks of longer pairs one wave each; one device scan gives every offset
//   5. emit       the same walk; each emitted entry as its index in the store's txn-major view (lower bound of its
//                 TxnId in the view's sorted TxnId columns), pair by pair in TxnId order
//   6. build      KeyDeps.Builder per query (utils/RelationMultiMap.java:201-260): queries with at most cfq_wave_cap
//                 hits sort / unique / look up in one wave's LDS; larger ones go through one radix sort of
//                 (query, txn index), a unique flag scan and a binary search per hit. Both leave the sorted unique
//                 txn indices in the hit slots, which one scan compacts into dep_txn.
//
//
// acc_cfk_keydeps_mixed: the same for queries of both domains (impl/InMemoryCommandStore.java:274-289, the Range case of
// mapReduceForKey: mapReduceActive on every CFK of commandsForKey.subMap(start, startInclusive, end, endInclusive) per
// range). A range query's row is the row of a key query over the CFK keys its ranges cover, and km.key is sorted, so
// the keys a range covers are one run of km.key and their entries one span of the entry columns. A front end turns
// the call into the (query, key) pairs of step 2 and everything from the offsets on runs as above:
//   r1. rvalidate  per query: kind, both offset arrays, keys only on key-domain and ranges only on range-domain queries,
//                  keys sorted unique, ranges start < end, sorted, not overlapping
//   r2. rbounds    per range: the run of km.key it covers (two binary searches with the store's bound type); per query
//                  its pairs (own keys or covered keys); one scan: the expanded pair offsets (the total goes to the host)
//   r3. rexpand    per expanded pair: its query, its range (a search of the per-range offsets: no thread walks a wide
//                  range) and its store key; a key-domain pair is located as in step 2, a covered pair knows its segment
//   lane tier      a covered pair whose whole segment holds at most lane_seg entries is answered by one lane: consecutive
//                  lanes take consecutive covered keys, so a wave reads one contiguous span of the entry columns
//                  instead of one wave per pair using a few of its 256 entry slots. The lane walks its segment to the
//                  first TxnId >= S gathering M and the tie count, then counts (cq_lane_max) and, after the offsets,
//                  writes (cq_lane_emit) the emitted entries. Such a pair keeps one chunk slot; the chunk kernels see
//                  it with an empty prefix and the lane kernels fill the slot after them, so neither the chunk kernels
//                  nor the offset machinery know about the tier.
//
// acc_cfk_map_reduce_full (the last section): BeginRecovery's CommandsForKey.mapReduceFull scans over the same resident
// segments, behind the same front end and in front of the same builder (build_keydeps).
//
// Results live in cq_* buffers only: acc_cfk_apply_deps trades the context's cd_* / cb_* buffers with the store.
#include "keydeps.hpp"
#include "cfkquery.hpp"
#include "recovery_pred.hpp"

namespace acc {

namespace cq {

constexpr uint32_t CH = 256;          // segment entries per work chunk: one wave, four per lane
constexpr uint32_t CAP_MAX = 1024;    // hits of a query the one-wave build tier holds in LDS (u64 each, per wave)
constexpr uint32_t LANE_SEG_DEFAULT = 16;   // acc_cfk_mixed_queries::lane_seg == 0 (the measured table)

enum : uint64_t { E_KIND_ARG = 1, E_KIND_STATE = 2, E_RANGE = 4, E_OFF = 8, E_KEYS = 16, E_TIE = 32,
                  E_RKEYS = 64, E_KRANGES = 128, E_ROFF = 256, E_RBOUND = 512, E_RORDER = 1024, E_KIND_BY = 2048 };

// which kinds a front end's validation refuses: PreAccept asks Kind.witnesses() of every query, a recovery scan asks
// Kind.witnessedBy() of its testTxnId only when the caller gave no Kinds mask (k_rc_query, recovery.hip)
enum : uint32_t { KINDS_WITNESSES = 0, KINDS_WITNESSED_BY = 1, KINDS_UNCHECKED = 2 };

struct Queries {
    const uint64_t *qm, *ql, *xm, *xl;   // TxnId, executeAt (= TxnId columns when the caller gave none)
    const int32_t *qn, *xn;
    const uint32_t *off;                 // [nq + 1]
    const uint64_t *key;                 // [Qp]
    uint32_t nq, Qp;
};

struct Pairs {
    const uint32_t *q, *a, *w;           // per pair: query, first entry of the segment, prefix length
    const uint64_t *chunk_off;           // [Qp + 1]
    const uint32_t *item;                // [chunks] the pair of every chunk
    uint32_t Qp;
};

// the lane tier's pairs: to the chunk kernels such a pair has an empty prefix (w = 0) and one chunk slot
struct Lanes {
    const uint8_t *is;                   // [Qp] the pair is answered by the lane tier
    uint32_t *w;                         // [Qp] its segment's length, then (k_cq_lane_max) its prefix's
};

// acc_cfk_keydeps_mixed: the caller's keys and ranges, and per range the run of km.key it covers
struct Ranges {
    const uint32_t *key_off, *rng_off;   // [nq + 1]
    const uint64_t *key_code;            // [n_pairs]
    const uint64_t *start, *end;         // [nr]
    uint32_t nr, end_inclusive;
    const uint32_t *lo;                  // [nr] first covered store key
    const uint64_t *cum;                 // [nr + 1] covered keys of the ranges before it
};

// a chunk's (and, in a pair's first chunk slot, the pair's) M and tie count: f = has M << 31 | min(ties, 3)
struct Part {
    uint64_t *m, *l;
    int32_t *n;
    uint32_t *f;
};

struct Best {
    uint64_t m, l;
    int32_t n;
    uint32_t has;
};

__device__ __forceinline__ bool committed(uint32_t st) { return st >= ACC_ST_COMMITTED && st <= ACC_ST_APPLIED; }

__device__ __forceinline__ void best_take(Best &b, uint64_t m, uint64_t l, int32_t n, uint32_t has)
{
    if (has && (!b.has || ts_cmp(m, l, n, b.m, b.l, b.n) > 0)) { b.m = m; b.l = l; b.n = n; b.has = 1; }
}

__device__ __forceinline__ Best wave_best(Best b)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t om = shfl_xor(b.m, d), ol = shfl_xor(b.l, d);
        const int32_t on = (int32_t)shfl_xor((uint32_t)b.n, d);
        const uint32_t oh = shfl_xor(b.has, d);
        best_take(b, om, ol, on, oh);
    }
    return b;
}

__global__ __launch_bounds__(BLOCK) void k_cq_validate(Queries Q, uint64_t *__restrict__ errs)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= Q.nq) return;
    uint64_t e = 0;
    const uint64_t l = Q.ql[q];
    const uint32_t kind = (uint32_t)(l >> 1) & 7u;
    if (kind > ACC_KIND_LOCAL_ONLY) e |= E_KIND_ARG;          // Kind.ofOrdinal
    else if (witnesses(kind) == 0) e |= E_KIND_STATE;         // Kind.witnesses(): LocalOnly throws
    if (l & 1u) e |= E_RANGE;
    const uint32_t k0 = Q.off[q], k1 = Q.off[q + 1];
    if (k1 < k0 || k1 > Q.Qp || (q == 0 && k0 != 0) || (q == Q.nq - 1 && k1 != Q.Qp)) e |= E_OFF;
    else
        for (uint32_t j = k0 + 1; j < k1; ++j)
            if (Q.key[j - 1] >= Q.key[j]) { e |= E_KEYS; break; }
    if (e) atomicOr((unsigned long long *)errs, (unsigned long long)e);
}

// the prefix of segment [s0, s1) below S (its length), and whether the entry at its end counts towards the tie rule
__device__ __forceinline__ uint32_t prefix_of(const CfkResident &s, uint32_t s0, uint32_t s1, uint64_t Sm, uint64_t Sl, int32_t Sn,
                                              uint32_t &t0)
{
    const uint32_t x = lower_bound_ts(s.em, s.el, s.en, s0, s1, Ts{ Sm, Sl, Sn });
    // entries past it have TxnId > S, and executeAt >= TxnId
    t0 = x < s1 && committed(s.st[x]) && ts_cmp(s.xm[x], s.xl[x], s.xn[x], Sm, Sl, Sn) == 0 ? 1u : 0u;
    return x - s0;
}

// per pair: the prefix [a, a + w) of its key's segment the scan visits, whether the entry at its end is a committed
// entry executing at S (it counts towards the tie rule), and its chunks
__global__ __launch_bounds__(BLOCK) void k_cq_locate(Queries Q, CfkResident s, uint32_t *__restrict__ pair_q,
                                                     uint32_t *__restrict__ pair_a, uint32_t *__restrict__ pair_w,
                                                     uint8_t *__restrict__ pair_t0, uint64_t *__restrict__ chunks)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= Q.Qp) return;
    const uint32_t q = upper_bound(Q.off, 0, Q.nq + 1, i) - 1;
    uint32_t a = 0, w = 0, t0 = 0;
    const uint64_t k = Q.key[i];
    const uint32_t lo = find_sorted(s.key, s.nk, k);
    if (lo != NOT_FOUND) {
        a = s.ent_off[lo];
        w = prefix_of(s, a, s.ent_off[lo + 1], Q.xm[q], Q.xl[q], Q.xn[q], t0);
    }
    pair_q[i] = q;
    pair_a[i] = a;
    pair_w[i] = w;
    pair_t0[i] = (uint8_t)t0;
    chunks[i] = (w + CH - 1) / CH;
}

// per pair: the pair of each of its chunks, so a chunk's wave reads its pair instead of searching the offsets
__global__ __launch_bounds__(BLOCK) void k_cq_items(uint32_t Qp, const uint64_t *__restrict__ chunk_off, uint32_t *__restrict__ item)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= Qp) return;
    for (uint64_t c = chunk_off[i], c1 = chunk_off[i + 1]; c < c1; ++c) item[c] = i;
}

// the per-entry switch of CommandsForKey.mapReduceActive (:628-647) and the map function's p1 test (PreAccept.java:253-259)
struct ChunkCtx {
    uint32_t item, q, base, end, wk, has_m;
    uint64_t qm, ql, Mm, Ml;
    int32_t qn, Mn;
};

__device__ __forceinline__ bool emitted(const CfkResident &s, const ChunkCtx &c, uint32_t e)
{
    const uint64_t el = s.el[e];
    if (!((c.wk >> ((uint32_t)(el >> 1) & 7u)) & 1u)) return false;
    const uint32_t st = s.st[e];
    if (st == ACC_ST_TRANSITIVELY_KNOWN || st == ACC_ST_INVALID_OR_TRUNCATED) return false;
    if (committed(st) && c.has_m && ts_cmp(s.xm[e], s.xl[e], s.xn[e], c.Mm, c.Ml, c.Mn) < 0) return false;
    if (ts_w1(el) == ts_w1(c.ql) && s.em[e] == c.qm && s.en[e] == c.qn) return false;
    return true;
}

__device__ __forceinline__ uint32_t chunk_count(const CfkResident &s, const ChunkCtx &c)
{
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t u = 0; u < CH / 64; ++u) {
        const uint32_t e = c.base + u * 64 + lane_id();
        cnt += (uint32_t)__popcll(__ballot(e < c.end && emitted(s, c, e)));
    }
    return cnt;
}

// one wave per chunk: the chunk's part of maxCommittedBefore and of the tie count. A pair of one chunk (a short prefix:
// the common case) has its M right here, so its wave counts the emitted entries as well (the entries are still in cache).
__global__ __launch_bounds__(BLOCK) void k_cq_max(uint64_t first, uint64_t nchunks, Queries Q, CfkResident s, Pairs P,
                                                  const uint8_t *__restrict__ pair_t0, Part part, uint64_t *__restrict__ chunk_cnt,
                                                  uint64_t *__restrict__ errs)
{
    const uint64_t cw = first + (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (cw >= nchunks) return;
    const uint32_t item = P.item[cw];
    const uint32_t q = P.q[item];
    const uint64_t c0 = P.chunk_off[item];
    const uint32_t base = P.a[item] + (uint32_t)(cw - c0) * CH, end = P.a[item] + P.w[item];
    const uint64_t Sm = Q.xm[q], Sl = Q.xl[q];
    const int32_t Sn = Q.xn[q];
    Best b{ 0, 0, 0, 0 };
    uint32_t ties = cw == c0 ? pair_t0[item] : 0u;
#pragma unroll
    for (uint32_t u = 0; u < CH / 64; ++u) {
        const uint32_t e = base + u * 64 + lane_id();
        bool tie = false;
        if (e < end && committed(s.st[e])) {
            const uint64_t xm = s.xm[e], xl = s.xl[e];
            const int32_t xn = s.xn[e];
            const int c = ts_cmp(xm, xl, xn, Sm, Sl, Sn);
            tie = c == 0;
            if (c < 0 && ((uint32_t)(s.el[e] >> 1) & 7u) == ACC_KIND_WRITE) best_take(b, xm, xl, xn, 1u);
        }
        ties += (uint32_t)__popcll(__ballot(tie));
    }
    b = wave_best(b);
    if (lane_id() == 0) {
        part.m[cw] = b.m; part.l[cw] = b.l; part.n[cw] = b.n;
        part.f[cw] = (b.has << 31) | min(ties, 3u);
        if (ties >= 2) atomicOr((unsigned long long *)errs, (unsigned long long)E_TIE);
    }
    if (P.chunk_off[item + 1] - c0 == 1) {
        ChunkCtx c;
        c.item = item; c.q = q; c.base = base; c.end = end;
        c.qm = Q.qm[q]; c.ql = Q.ql[q]; c.qn = Q.qn[q];
        c.wk = witnesses((uint32_t)(c.ql >> 1) & 7u);
        c.has_m = b.has; c.Mm = b.m; c.Ml = b.l; c.Mn = b.n;
        const uint32_t cnt = chunk_count(s, c);
        if (lane_id() == 0) chunk_cnt[cw] = cnt;
    }
}

// one wave per pair of several chunks: the chunks' parts folded into the pair's first chunk slot
__global__ __launch_bounds__(BLOCK) void k_cq_fold(uint64_t first, Pairs P, Part part, uint64_t *__restrict__ errs)
{
    const uint64_t i = first + (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= P.Qp) return;
    const uint64_t c0 = P.chunk_off[i], c1 = P.chunk_off[i + 1];
    if (c1 - c0 <= 1) return;
    Best b{ 0, 0, 0, 0 };
    uint32_t ties = 0;
    for (uint64_t c = c0 + lane_id(); c < c1; c += 64) {
        const uint32_t f = part.f[c];
        best_take(b, part.m[c], part.l[c], part.n[c], f >> 31);
        ties = min(ties + (f & 3u), 3u);
    }
    b = wave_best(b);
    ties = wave_inclusive(ties, OpAdd<uint32_t>());   // <= 3 * 64
    ties = shfl_idx(ties, 63);
    if (lane_id() == 0) {
        part.m[c0] = b.m; part.l[c0] = b.l; part.n[c0] = b.n;
        part.f[c0] = (b.has << 31) | min(ties, 3u);
        if (ties >= 2) atomicOr((unsigned long long *)errs, (unsigned long long)E_TIE);
    }
}

// what one wave needs of its chunk's pair and query, M read from the pair's first chunk slot
__device__ __forceinline__ ChunkCtx chunk_ctx(uint64_t cw, const Queries &Q, const Pairs &P, const Part &part)
{
    ChunkCtx c;
    c.item = P.item[cw];
    c.q = P.q[c.item];
    const uint64_t c0 = P.chunk_off[c.item];
    c.base = P.a[c.item] + (uint32_t)(cw - c0) * CH;
    c.end = P.a[c.item] + P.w[c.item];
    c.qm = Q.qm[c.q]; c.ql = Q.ql[c.q]; c.qn = Q.qn[c.q];
    c.wk = witnesses((uint32_t)(c.ql >> 1) & 7u);
    c.has_m = part.f[c0] >> 31;
    c.Mm = part.m[c0]; c.Ml = part.l[c0]; c.Mn = part.n[c0];
    return c;
}

// one wave per chunk of a pair of several chunks (k_cq_max counted the others)
__global__ __launch_bounds__(BLOCK) void k_cq_count(uint64_t first, uint64_t nchunks, Queries Q, CfkResident s, Pairs P, Part part,
                                                    uint64_t *__restrict__ chunk_cnt)
{
    const uint64_t cw = first + (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (cw >= nchunks) return;
    const uint32_t item = P.item[cw];
    if (P.chunk_off[item + 1] - P.chunk_off[item] == 1) return;
    const ChunkCtx c = chunk_ctx(cw, Q, P, part);
    const uint32_t cnt = chunk_count(s, c);
    if (lane_id() == 0) chunk_cnt[cw] = cnt;
}

// per pair (and the end sentinel): its first hit slot; per pair: does its key get a KeyDeps entry
__global__ __launch_bounds__(BLOCK) void k_cq_epos(uint32_t Qp, const uint64_t *__restrict__ chunk_off,
                                                   const uint64_t *__restrict__ chunk_eoff, uint64_t *__restrict__ epos,
                                                   uint64_t *__restrict__ kept)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > Qp) return;
    const uint64_t e0 = chunk_eoff[chunk_off[i]];
    epos[i] = e0;
    if (i < Qp) kept[i] = chunk_eoff[chunk_off[i + 1]] > e0 ? 1u : 0u;
}

// per query (and the end sentinel): arena and key offsets; per query: its hits when they exceed the one-wave tier's cap
__global__ __launch_bounds__(BLOCK) void k_cq_qoff(uint32_t nq, const uint32_t *__restrict__ qoff, const uint64_t *__restrict__ kpos,
                                                   const uint64_t *__restrict__ epos, uint32_t cap, uint64_t *__restrict__ arena_off,
                                                   uint64_t *__restrict__ kd_off, uint64_t *__restrict__ gcnt)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q > nq) return;
    const uint32_t b = qoff[q];
    arena_off[q] = kpos[b] + epos[b];
    kd_off[q] = kpos[b];
    if (q < nq) {
        const uint64_t h = epos[qoff[q + 1]] - epos[b];
        gcnt[q] = h > cap ? h : 0u;
    }
}

// entry e as its index in the store's txn-major view: the lower bound of its TxnId in the view's sorted TxnId columns
__device__ __forceinline__ uint32_t view_index(const CfkResident &s, uint32_t e)
{
    const uint64_t xm = s.em[e], xl = s.el[e];
    const int32_t xn = s.en[e];
    return lower_bound_ts(s.tm, s.tl, s.tn, 0, s.n_txn, Ts{ xm, xl, xn });
}

// the count pass's walk, compacting in position order: every emitted entry as its index in the store's txn-major view
__global__ __launch_bounds__(BLOCK) void k_cq_emit(uint64_t first, uint64_t nchunks, Queries Q, CfkResident s, Pairs P, Part part,
                                                   const uint64_t *__restrict__ chunk_eoff, const uint64_t *__restrict__ epos,
                                                   const uint64_t *__restrict__ gcnt, const uint64_t *__restrict__ goff, int tb,
                                                   uint32_t *__restrict__ hit, uint64_t *__restrict__ gkey)
{
    const uint64_t cw = first + (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (cw >= nchunks) return;
    const ChunkCtx c = chunk_ctx(cw, Q, P, part);
    const uint64_t lt = (1ull << lane_id()) - 1;
    uint64_t out = chunk_eoff[cw];
    const bool big = gcnt[c.q] != 0;
    const uint64_t gbase = big ? goff[c.q] - epos[Q.off[c.q]] : 0;   // hit slot -> slot among the sorting tier's hits
#pragma unroll
    for (uint32_t u = 0; u < CH / 64; ++u) {
        const uint32_t e = c.base + u * 64 + lane_id();
        const bool m = e < c.end && emitted(s, c, e);
        const uint64_t bal = __ballot(m);
        if (m) {
            const uint32_t lo = view_index(s, e);
            const uint64_t p = out + (uint64_t)__popcll(bal & lt);
            hit[p] = lo;
            if (big) gkey[gbase + p] = ((uint64_t)c.q << tb) | lo;
        }
        out += (uint64_t)__popcll(bal);
    }
}

// AbstractBuilder: a key with entries gets its end offset (keys.length + entries through it), its index and its code
__global__ __launch_bounds__(BLOCK) void k_cq_header(Queries Q, const uint32_t *__restrict__ pair_q, const uint64_t *__restrict__ kpos,
                                                     const uint64_t *__restrict__ epos, const uint64_t *__restrict__ arena_off,
                                                     int32_t *__restrict__ arena, uint32_t *__restrict__ key_idx,
                                                     uint64_t *__restrict__ kd_key)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= Q.Qp) return;
    if (epos[i + 1] == epos[i]) return;
    const uint32_t q = pair_q[i], b = Q.off[q], e = Q.off[q + 1];
    const uint64_t kd = kpos[e] - kpos[b];
    arena[arena_off[q] + (kpos[i] - kpos[b])] = (int32_t)(kd + (epos[i + 1] - epos[b]));
    key_idx[kpos[i]] = i - b;
    kd_key[kpos[i]] = Q.key[i];
}

// build tier 1, one wave per query with 1..cap hits: sort in LDS, unique in place, every hit's position by binary search.
// Leaves the sorted unique txn indices in the query's first hit slots (uflag 1), the rest flagged 0.
__global__ __launch_bounds__(BLOCK) void k_cq_build_wave(uint64_t first, uint32_t nq, const uint32_t *__restrict__ qoff, const uint64_t *__restrict__ epos,
                                                         const uint64_t *__restrict__ arena_off, const uint64_t *__restrict__ kd_off,
                                                         uint32_t cap, const uint32_t *__restrict__ hit, int32_t *__restrict__ arena,
                                                         uint32_t *__restrict__ uflag, uint32_t *__restrict__ uval)
{
    __shared__ uint64_t lds[WAVES][CAP_MAX];
    const uint64_t qi = first + (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const uint32_t q = (uint32_t)qi;
    const uint64_t h0 = epos[qoff[q]];
    const uint64_t h64 = epos[qoff[q + 1]] - h0;
    if (h64 == 0 || h64 > cap) return;
    const uint32_t H = (uint32_t)h64, lane = lane_id();
    uint64_t *buf = lds[threadIdx.x >> 6];
    uint32_t n2 = 128;
    while (n2 < H) n2 <<= 1;
    for (uint32_t i = lane; i < n2; i += 64) buf[i] = i < H ? (uint64_t)hit[h0 + i] : ~0ull;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    wave_bitonic_lds(buf, n2);
    // unique, in place: round r compacts sorted positions [64 r, 64 r + 64) to positions <= their own
    uint32_t U = 0;
    uint64_t last = ~0ull;
    const uint64_t lt = (1ull << lane) - 1;
    for (uint32_t base = 0; base < H; base += 64) {
        const uint32_t i = base + lane;
        const uint64_t a = i < H ? buf[i] : ~0ull;
        uint64_t prev = shfl_up(a, 1);
        if (lane == 0) prev = last;
        const bool f = i < H && a != prev;
        const uint64_t bal = __ballot(f);
        __builtin_amdgcn_wave_barrier();
        if (f) buf[U + (uint32_t)__popcll(bal & lt)] = a;
        U += (uint32_t)__popcll(bal);
        last = shfl_idx(a, 63);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    const uint64_t body = arena_off[q] + (kd_off[q + 1] - kd_off[q]);
    for (uint32_t i = lane; i < H; i += 64) {
        const uint64_t v = hit[h0 + i];
        arena[body + i] = (int32_t)lower_bound(buf, 0, U, v);
        uflag[h0 + i] = i < U ? 1u : 0u;
        uval[h0 + i] = i < U ? (uint32_t)buf[i] : 0u;
    }
}

// build tier 2 over the sorted (query, txn index) keys: first occurrences, left in the hit slots of their query
__global__ __launch_bounds__(BLOCK) void k_cq_guniq(uint64_t G, const uint64_t *__restrict__ sk, int tb, const uint32_t *__restrict__ qoff,
                                                    const uint64_t *__restrict__ epos, const uint64_t *__restrict__ goff,
                                                    uint32_t *__restrict__ gflag, uint32_t *__restrict__ uflag, uint32_t *__restrict__ uval)
{
    const uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= G) return;
    const uint64_t k = sk[g];
    const uint32_t f = (g == 0 || sk[g - 1] != k) ? 1u : 0u;
    gflag[g] = f;
    const uint32_t q = (uint32_t)(k >> tb);
    const uint64_t p = epos[qoff[q]] + (g - goff[q]);
    uflag[p] = f;
    uval[p] = (uint32_t)(k & ((1ull << tb) - 1));
}

// every sorting-tier hit's index into its query's sorted unique txn indices
__global__ __launch_bounds__(BLOCK) void k_cq_gbody(uint64_t G, const uint64_t *__restrict__ gkey, const uint64_t *__restrict__ sk,
                                                    const uint32_t *__restrict__ ginc, int tb, const uint64_t *__restrict__ gcnt,
                                                    const uint64_t *__restrict__ goff, const uint64_t *__restrict__ arena_off,
                                                    const uint64_t *__restrict__ kd_off, int32_t *__restrict__ arena)
{
    const uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= G) return;
    const uint64_t k = gkey[g];
    const uint32_t q = (uint32_t)(k >> tb);
    const uint64_t g0 = goff[q];
    const uint64_t lo = lower_bound(sk, g0, g0 + gcnt[q], k);
    arena[arena_off[q] + (kd_off[q + 1] - kd_off[q]) + (g - g0)] = (int32_t)(ginc[lo] - ginc[g0]);
}

__global__ __launch_bounds__(BLOCK) void k_cq_deps(uint64_t E, const uint32_t *__restrict__ uflag, const uint32_t *__restrict__ uval,
                                                   const uint32_t *__restrict__ upos, uint32_t *__restrict__ dep_txn)
{
    const uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p < E && uflag[p]) dep_txn[upos[p]] = uval[p];
}

__global__ __launch_bounds__(BLOCK) void k_cq_uoff(uint32_t nq, const uint32_t *__restrict__ qoff, const uint64_t *__restrict__ epos,
                                                   const uint32_t *__restrict__ upos, uint64_t *__restrict__ u_off)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q <= nq) u_off[q] = upos[epos[qoff[q]]];
}

// ---------------------------------------------------------------- acc_cfk_keydeps_mixed: the front end and the lane tier

// Q.off / Q.key: the caller's key_off / key_code
__global__ __launch_bounds__(BLOCK) void k_cq_rvalidate(Queries Q, Ranges R, uint32_t kinds, uint64_t *__restrict__ errs)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= Q.nq) return;
    uint64_t e = 0;
    const uint64_t l = Q.ql[q];
    const uint32_t kind = (uint32_t)(l >> 1) & 7u;
    if (kinds == KINDS_WITNESSES) {
        if (kind > ACC_KIND_LOCAL_ONLY) e |= E_KIND_ARG;          // Kind.ofOrdinal
        else if (witnesses(kind) == 0) e |= E_KIND_STATE;         // Kind.witnesses(): LocalOnly throws
    } else if (kinds == KINDS_WITNESSED_BY && witnessed_by(kind) < 0) {
        e |= kind == ACC_KIND_LOCAL_ONLY ? E_KIND_BY : E_KIND_ARG;   // Kind.witnessedBy(): LocalOnly throws
    }
    const bool range = l & 1u;
    const uint32_t k0 = Q.off[q], k1 = Q.off[q + 1];
    if (k1 < k0 || k1 > Q.Qp || (q == 0 && k0 != 0) || (q == Q.nq - 1 && k1 != Q.Qp)) e |= E_OFF;
    else if (range) { if (k1 != k0) e |= E_RKEYS; }
    else
        for (uint32_t j = k0 + 1; j < k1; ++j)
            if (Q.key[j - 1] >= Q.key[j]) { e |= E_KEYS; break; }
    const uint32_t r0 = R.rng_off[q], r1 = R.rng_off[q + 1];
    if (r1 < r0 || r1 > R.nr || (q == 0 && r0 != 0) || (q == Q.nq - 1 && r1 != R.nr)) e |= E_ROFF;
    else if (!range) { if (r1 != r0) e |= E_KRANGES; }
    else
        for (uint32_t j = r0; j < r1; ++j) {
            if (R.start[j] >= R.end[j]) e |= E_RBOUND;
            if (j > r0 && R.end[j - 1] > R.start[j]) e |= E_RORDER;     // touching ranges are allowed
        }
    if (e) atomicOr((unsigned long long *)errs, (unsigned long long)e);
}

// per range: the run of store keys it covers, (start, end] or [start, end)
__global__ __launch_bounds__(BLOCK) void k_cq_rbounds(Ranges R, CfkResident s, uint32_t *__restrict__ rlo, uint64_t *__restrict__ rcnt)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= R.nr) return;
    const uint64_t a = R.start[r], b = R.end[r];
    uint32_t lo, hi;
    if (R.end_inclusive) {
        lo = upper_bound(s.key, 0, s.nk, a);
        hi = upper_bound(s.key, 0, s.nk, b);
    } else {
        lo = a ? upper_bound(s.key, 0, s.nk, a - 1) : 0u;
        hi = upper_bound(s.key, 0, s.nk, b - 1);                      // start < end: b >= 1
    }
    rlo[r] = lo;
    rcnt[r] = hi - lo;
}

// per query: its pairs, own keys or covered keys
__global__ __launch_bounds__(BLOCK) void k_cq_rcount(Queries Q, Ranges R, uint64_t *__restrict__ qcnt)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= Q.nq) return;
    qcnt[q] = (Q.ql[q] & 1u) ? R.cum[R.rng_off[q + 1]] - R.cum[R.rng_off[q]] : (uint64_t)(Q.off[q + 1] - Q.off[q]);
}

// the expanded pair offsets as the u32 the scan reads (the host has checked the total)
__global__ __launch_bounds__(BLOCK) void k_cq_roff(uint32_t n, const uint64_t *__restrict__ in, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = (uint32_t)in[i];
}

// an expanded pair (Q.off: the expanded offsets): its query, its key's code and its segment (s.nk: the key has no CFK).
// A key-domain pair searches its key; a covered pair finds its range by the per-range offsets (no thread walks a wide
// range) and knows its segment.
__device__ __forceinline__ uint32_t pair_segment(const Queries &Q, const Ranges &R, const CfkResident &s, uint32_t i, uint32_t &q,
                                                 uint64_t &k, bool &range)
{
    q = upper_bound(Q.off, 0, Q.nq + 1, i) - 1;
    const uint32_t j = i - Q.off[q];
    uint32_t seg = s.nk;
    range = Q.ql[q] & 1u;
    if (range) {
        const uint32_t r0 = R.rng_off[q], r1 = R.rng_off[q + 1];
        const uint64_t at = R.cum[r0] + j;
        const uint32_t r = upper_bound(R.cum, r0, r1, at) - 1;     // the last range starting at or below at
        seg = R.lo[r] + (uint32_t)(at - R.cum[r]);
        k = s.key[seg];
    } else {
        k = R.key_code[R.key_off[q] + j];
        const uint32_t lo = find_sorted(s.key, s.nk, k);
        if (lo != NOT_FOUND) seg = lo;
    }
    return seg;
}

// k_cq_locate over the expanded pairs: a key-domain pair is located as there, a covered pair knows its segment; a
// covered pair with a short segment goes to the lane tier, which finds the prefix itself (lane_w: the segment's length
// until then). Writes every pair's key code.
__global__ __launch_bounds__(BLOCK) void k_cq_rexpand(Queries Q, Ranges R, CfkResident s, uint32_t lane_seg, uint64_t *__restrict__ x_key,
                                                      uint32_t *__restrict__ pair_q, uint32_t *__restrict__ pair_a,
                                                      uint32_t *__restrict__ pair_w, uint8_t *__restrict__ pair_t0,
                                                      uint64_t *__restrict__ chunks, uint8_t *__restrict__ lane,
                                                      uint32_t *__restrict__ lane_w, uint64_t *__restrict__ nlane)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= Q.Qp) return;
    uint32_t q, a = 0, w = 0, t0 = 0, ln = 0;
    uint64_t k;
    bool range;
    const uint32_t seg = pair_segment(Q, R, s, i, q, k, range);
    if (seg < s.nk) {
        const uint32_t s0 = s.ent_off[seg], s1 = s.ent_off[seg + 1];
        a = s0;
        if (range && lane && s1 - s0 <= lane_seg) { ln = 1; lane_w[i] = s1 - s0; }
        else w = prefix_of(s, s0, s1, Q.xm[q], Q.xl[q], Q.xn[q], t0);
    }
    x_key[i] = k;
    pair_q[i] = q;
    pair_a[i] = a;
    pair_w[i] = w;
    pair_t0[i] = (uint8_t)t0;
    if (lane) lane[i] = (uint8_t)ln;
    chunks[i] = ln ? 1u : (w + CH - 1) / CH;
    const uint64_t bal = __ballot(ln != 0);
    if (ln && lane_id() == (uint32_t)__ffsll((long long)bal) - 1)
        atomicAdd((unsigned long long *)nlane, (unsigned long long)__popcll(bal));
}

// lane tier, one lane per pair: walks the segment to the first TxnId >= S (the prefix's end), gathering M and the tie
// count (the entry at the end included), then counts the emitted entries of the prefix; fills the pair's chunk slot
__global__ __launch_bounds__(BLOCK) void k_cq_lane_max(Queries Q, CfkResident s, Pairs P, Lanes ln, Part part,
                                                       uint64_t *__restrict__ chunk_cnt, uint64_t *__restrict__ errs)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.Qp || !ln.is[i]) return;
    const uint32_t q = P.q[i], a = P.a[i], s1 = a + ln.w[i];
    const uint64_t Sm = Q.xm[q], Sl = Q.xl[q];
    const int32_t Sn = Q.xn[q];
    Best b{ 0, 0, 0, 0 };
    uint32_t ties = 0, e = a;
    for (; e < s1; ++e) {
        if (ts_cmp(s.em[e], s.el[e], s.en[e], Sm, Sl, Sn) >= 0) break;
        if (committed(s.st[e])) {
            const uint64_t xm = s.xm[e], xl = s.xl[e];
            const int32_t xn = s.xn[e];
            const int c = ts_cmp(xm, xl, xn, Sm, Sl, Sn);
            if (c == 0) ++ties;
            else if (c < 0 && ((uint32_t)(s.el[e] >> 1) & 7u) == ACC_KIND_WRITE) best_take(b, xm, xl, xn, 1u);
        }
    }
    if (e < s1 && committed(s.st[e]) && ts_cmp(s.xm[e], s.xl[e], s.xn[e], Sm, Sl, Sn) == 0) ++ties;
    ChunkCtx c;
    c.item = i; c.q = q; c.base = a; c.end = e;
    c.qm = Q.qm[q]; c.ql = Q.ql[q]; c.qn = Q.qn[q];
    c.wk = witnesses((uint32_t)(c.ql >> 1) & 7u);
    c.has_m = b.has; c.Mm = b.m; c.Ml = b.l; c.Mn = b.n;
    uint32_t cnt = 0;
    for (uint32_t x = a; x < e; ++x) cnt += emitted(s, c, x) ? 1u : 0u;
    const uint64_t cw = P.chunk_off[i];
    part.m[cw] = b.m; part.l[cw] = b.l; part.n[cw] = b.n;
    part.f[cw] = (b.has << 31) | min(ties, 3u);
    chunk_cnt[cw] = cnt;
    ln.w[i] = e - a;
    if (ties >= 2) atomicOr((unsigned long long *)errs, (unsigned long long)E_TIE);
}

// lane tier: the same walk over the prefix, every emitted entry as its view index, in TxnId order
__global__ __launch_bounds__(BLOCK) void k_cq_lane_emit(Queries Q, CfkResident s, Pairs P, Lanes ln, Part part, const uint64_t *__restrict__ chunk_eoff,
                                                        const uint64_t *__restrict__ epos, const uint64_t *__restrict__ gcnt,
                                                        const uint64_t *__restrict__ goff, int tb, uint32_t *__restrict__ hit,
                                                        uint64_t *__restrict__ gkey)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.Qp || !ln.is[i]) return;
    const uint64_t cw = P.chunk_off[i];
    uint64_t out = chunk_eoff[cw];
    if (chunk_eoff[cw + 1] == out) return;
    ChunkCtx c = chunk_ctx(cw, Q, P, part);
    c.end = c.base + ln.w[i];
    const bool big = gcnt[c.q] != 0;
    const uint64_t gbase = big ? goff[c.q] - epos[Q.off[c.q]] : 0;
    for (uint32_t e = c.base; e < c.end; ++e) {
        if (!emitted(s, c, e)) continue;
        const uint32_t lo = view_index(s, e);
        hit[out] = lo;
        if (big) gkey[gbase + out] = ((uint64_t)c.q << tb) | lo;
        ++out;
    }
}

static void check_cq_errors(uint64_t e)
{
    if (e & E_KIND_ARG) fail(ACC_E_ARG, "Kind.ofOrdinal: invalid kind ordinal in a query TxnId");
    if (e & E_RANGE) fail(ACC_E_ARG, "range-domain queries against the resident store are not supported");
    if (e & E_OFF) fail(ACC_E_ARG, "query key_off must start at 0, be non-decreasing and end at n_pairs");
    if (e & E_KEYS) fail(ACC_E_ARG, "keys of a query must be sorted and unique (Keys.ofSortedUnique)");
    if (e & E_ROFF) fail(ACC_E_ARG, "query rng_off must start at 0, be non-decreasing and end at n_ranges");
    if (e & E_RKEYS) fail(ACC_E_ARG, "a range-domain query lists keys");
    if (e & E_KRANGES) fail(ACC_E_ARG, "a key-domain query lists ranges");
    if (e & E_RBOUND) fail(ACC_E_ARG, "a range needs start < end");
    if (e & E_RORDER) fail(ACC_E_ARG, "ranges of a query must be sorted and must not overlap (Ranges.ofSortedAndDeoverlapped)");
    if (e & E_KIND_STATE) fail(ACC_E_STATE, "Kind.witnesses(): unhandled kind LocalOnly (AssertionError)");
    if (e & E_KIND_BY) fail(ACC_E_STATE, "Kind.witnessedBy(): unhandled kind LocalOnly (AssertionError)");
    if (e & E_TIE)
        fail(ACC_E_STATE, "two or more committed entries of one key execute at a query's executeAt: the FAST bisection "
                          "of committed[] is not determined");
}

}  // namespace cq

using namespace cq;

// what an entry's front end (k_cq_locate / k_cq_rexpand) leaves per pair for the scan both entries share
struct Located {
    uint32_t *pair_q, *pair_a, *pair_w;
    uint8_t *pair_t0;
    uint64_t *chunks;
    uint8_t *lane;          // null: no lane tier (acc_cfk_keydeps, ACC_CFQ_LANE_NONE)
    uint32_t *lane_w;
    uint64_t *nlane;        // the lane tier's pairs, counted on the device; null: acc_cfk_keydeps
};

static Located located_bufs(acc_ctx *ctx, uint32_t Qp, bool lanes)
{
    return Located{ ctx->get<uint32_t>("cq_pair_q", Qp), ctx->get<uint32_t>("cq_pair_a", Qp), ctx->get<uint32_t>("cq_pair_w", Qp),
                    ctx->get<uint8_t>("cq_pair_t0", Qp), ctx->get<uint64_t>("cq_chunks", Qp),
                    lanes ? ctx->get<uint8_t>("cq_pair_lane", Qp) : nullptr, lanes ? ctx->get<uint32_t>("cq_lane_w", Qp) : nullptr,
                    nullptr };
}

static CfkResident resident_checked(acc_cfk *cfk, uint32_t mem)
{
    if (mem != ACC_MEM_HOST && mem != ACC_MEM_DEVICE) fail(ACC_E_ARG, "mem must be ACC_MEM_HOST or ACC_MEM_DEVICE");
    const CfkResident s = cfk_resident(cfk);
    if (!s.deps && s.n_txn)
        fail(ACC_E_STATE, "the store holds status-only state (acc_cfk_update): it has no key-major CommandsForKey to scan");
    return s;
}

// n_query == 0
static void empty_result(acc_ctx *ctx, acc_keydeps_view *view)
{
    hipStream_t st = ctx->stream;
    uint64_t *arena_off = ctx->get<uint64_t>("cq_arena_off", 1);
    uint64_t *kd_off = ctx->get<uint64_t>("cq_kd_off", 1);
    uint64_t *u_off = ctx->get<uint64_t>("cq_u_off", 1);
    ACC_HIP(hipMemsetAsync(arena_off, 0, 8, st));
    ACC_HIP(hipMemsetAsync(kd_off, 0, 8, st));
    ACC_HIP(hipMemsetAsync(u_off, 0, 8, st));
    ctx->sync();
    *view = acc_keydeps_view{ 0, 0, 0, 0, 0, arena_off, ctx->get<int32_t>("cq_arena", 1), kd_off,
                              ctx->get<uint32_t>("cq_key_idx", 1), u_off, ctx->get<uint32_t>("cq_dep_txn", 1),
                              ctx->get<uint64_t>("cq_kd_key", 1) };
    ctx->kd_view = *view;
    ctx->kd_valid = true;
}

static void stage_ids(acc_ctx *ctx, Queries &Q, const acc_ts_cols &txn_id, const acc_ts_cols &execute_at, uint32_t nq, uint32_t mem)
{
    Q.qm = stage_in(ctx, "cq_in_qm", txn_id.msb, nq, mem);
    Q.ql = stage_in(ctx, "cq_in_ql", txn_id.lsb, nq, mem);
    Q.qn = stage_in(ctx, "cq_in_qn", txn_id.node, nq, mem);
    if (execute_at.msb) {
        Q.xm = stage_in(ctx, "cq_in_xm", execute_at.msb, nq, mem);
        Q.xl = stage_in(ctx, "cq_in_xl", execute_at.lsb, nq, mem);
        Q.xn = stage_in(ctx, "cq_in_xn", execute_at.node, nq, mem);
    } else {
        Q.xm = Q.qm; Q.xl = Q.ql; Q.xn = Q.qn;
    }
}

static uint64_t scan_located(acc_ctx *ctx, const CfkResident &s, const Queries &Q, const Located &L, uint64_t *errs, acc_keydeps_view *view);

// the caller's participants of a call over both domains (acc_cfk_mixed_queries, acc_cfk_recovery_in)
struct Parts {
    const uint32_t *key_off;
    const uint64_t *key_code;
    const uint32_t *rng_off;
    const uint64_t *rng_start, *rng_end;
    uint32_t n_pairs, n_ranges, end_inclusive, mem;
};

// The front end both entries over both domains share (r1, r2 above): stages the participants, validates (kinds by the
// entry's rule; nothing after it indexes by an offset or trusts key or range order before it has passed), finds the
// store keys every range covers and the expanded pair offsets. Q (nq and the ids staged) leaves as the queries over the
// expanded pairs: off their offsets, Qp their number, key = xkey, which the entry's expand kernel fills (pair_segment).
// Returns the covered (range query, key) pairs.
static uint64_t expand_queries(acc_ctx *ctx, const CfkResident &s, Queries &Q, Ranges &R, const Parts &in, uint32_t kinds,
                               uint64_t *errs, uint64_t *&xkey)
{
    hipStream_t st = ctx->stream;
    const uint32_t nq = Q.nq, NR = in.n_ranges, mem = in.mem;
    Q.Qp = in.n_pairs;       // over the caller's keys until the expansion
    Q.off = stage_in(ctx, "cq_in_off", in.key_off, (size_t)nq + 1, mem);
    Q.key = stage_in(ctx, "cq_in_key", in.key_code, in.n_pairs, mem);
    R.key_off = Q.off;
    R.key_code = Q.key;
    R.rng_off = stage_in(ctx, "cq_in_roff", in.rng_off, (size_t)nq + 1, mem);
    R.start = stage_in(ctx, "cq_in_rs", in.rng_start, NR, mem);
    R.end = stage_in(ctx, "cq_in_re", in.rng_end, NR, mem);
    R.nr = NR;
    R.end_inclusive = in.end_inclusive;

    // ---- validate
    ACC_HIP(hipMemsetAsync(errs, 0, 8, st));
    launch(ctx, "cq_rvalidate", k_cq_rvalidate, dim3(grid_for(nq, BLOCK)), dim3(BLOCK), 0, Q, R, kinds, errs);
    ReadBack rb_valid(ctx);
    const auto h_errs = rb_valid.u64(errs);
    rb_valid.wait();
    check_cq_errors(h_errs);

    // ---- bounds: the store keys every range covers, the expanded pair offsets
    uint32_t *rlo = ctx->get<uint32_t>("cq_rlo", NR);
    uint64_t *rcnt = ctx->get<uint64_t>("cq_rcnt", NR);
    uint64_t *rcum = ctx->get<uint64_t>("cq_rcum", (size_t)NR + 1);
    if (NR) {
        launch(ctx, "cq_rbounds", k_cq_rbounds, dim3(grid_for(NR, BLOCK)), dim3(BLOCK), 0, R, s, rlo, rcnt);
        scan<uint64_t, OpAdd<uint64_t>>(ctx, rcnt, rcum, NR, true, rcum + NR);
    } else {
        ACC_HIP(hipMemsetAsync(rcum, 0, 8, st));
    }
    R.lo = rlo;
    R.cum = rcum;
    uint64_t *qcnt = ctx->get<uint64_t>("cq_qcnt", nq);
    uint64_t *xoff64 = ctx->get<uint64_t>("cq_xoff64", (size_t)nq + 1);
    launch(ctx, "cq_rcount", k_cq_rcount, dim3(grid_for(nq, BLOCK)), dim3(BLOCK), 0, Q, R, qcnt);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, qcnt, xoff64, nq, true, xoff64 + nq);
    ReadBack rb_pairs(ctx);
    const auto h_x = rb_pairs.u64(xoff64 + nq), h_covered = rb_pairs.u64(rcum + NR);
    rb_pairs.wait();
    const uint64_t X = h_x, covered = h_covered;
    if (X >= 0xFFFFFFFFull) fail(ACC_E_CAP, "too many (query, key) pairs after expanding the ranges (>= 2^32 - 1)");
    const uint32_t Xp = (uint32_t)X;
    uint32_t *xoff = ctx->get<uint32_t>("cq_xoff", (size_t)nq + 1);
    xkey = ctx->get<uint64_t>("cq_xkey", Xp);
    launch(ctx, "cq_roff", k_cq_roff, dim3(grid_for((size_t)nq + 1, BLOCK)), dim3(BLOCK), 0, nq + 1, (const uint64_t *)xoff64, xoff);
    Q.off = xoff;
    Q.key = xkey;
    Q.Qp = Xp;
    return covered;
}

void cfk_keydeps(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_queries *in, acc_keydeps_view *view)
{
    if (!cfk || !in || !view) fail(ACC_E_ARG, "null argument");
    const CfkResident s = resident_checked(cfk, in->mem);
    if (in->n_pairs >= 0xFFFFFFFFull) fail(ACC_E_CAP, "too many (query, key) pairs in one call (>= 2^32 - 1)");
    hipStream_t st = ctx->stream;
    ctx->kd_valid = false;
    const uint32_t nq = in->n_query, Qp = (uint32_t)in->n_pairs, mem = in->mem;
    if (nq == 0) {
        if (Qp) fail(ACC_E_ARG, "query key_off must start at 0, be non-decreasing and end at n_pairs");
        empty_result(ctx, view);
        return;
    }

    Queries Q{};
    Q.nq = nq;
    Q.Qp = Qp;
    Q.off = stage_in(ctx, "cq_in_off", in->key_off, (size_t)nq + 1, mem);
    Q.key = stage_in(ctx, "cq_in_key", in->key_code, Qp, mem);
    stage_ids(ctx, Q, in->txn_id, in->execute_at, nq, mem);

    // ---- validate: nothing below indexes by an offset or trusts key order before this has passed
    uint64_t *errs = ctx->get<uint64_t>("cq_errs", 1);
    ACC_HIP(hipMemsetAsync(errs, 0, 8, st));
    launch(ctx, "cq_validate", k_cq_validate, dim3(grid_for(nq, BLOCK)), dim3(BLOCK), 0, Q, errs);
    ReadBack rb_valid(ctx);
    const auto h_errs = rb_valid.u64(errs);
    rb_valid.wait();
    check_cq_errors(h_errs);

    // ---- locate: prefixes and chunks
    const Located L = located_bufs(ctx, Qp, false);
    if (Qp)
        launch(ctx, "cq_locate", k_cq_locate, dim3(grid_for(Qp, BLOCK)), dim3(BLOCK), 0, Q, s, L.pair_q, L.pair_a, L.pair_w, L.pair_t0,
               L.chunks);
    scan_located(ctx, s, Q, L, errs, view);
}

void cfk_keydeps_mixed(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_mixed_queries *in, acc_keydeps_view *view)
{
    if (!cfk || !in || !view) fail(ACC_E_ARG, "null argument");
    const CfkResident s = resident_checked(cfk, in->mem);
    if (in->end_inclusive > 1) fail(ACC_E_ARG, "end_inclusive must be 0 or 1");
    if (in->lane_seg > CH && in->lane_seg != ACC_CFQ_LANE_NONE) fail(ACC_E_ARG, "lane_seg must be 0..256 or ACC_CFQ_LANE_NONE");
    if (in->n_pairs >= 0xFFFFFFFFull) fail(ACC_E_CAP, "too many (query, key) pairs in one call (>= 2^32 - 1)");
    if (in->n_ranges >= 0xFFFFFFFFull) fail(ACC_E_CAP, "too many ranges in one call (>= 2^32 - 1)");
    hipStream_t st = ctx->stream;
    ctx->kd_valid = false;
    const uint32_t nq = in->n_query, Kp = (uint32_t)in->n_pairs, NR = (uint32_t)in->n_ranges, mem = in->mem;
    const uint32_t lane_seg = in->lane_seg == ACC_CFQ_LANE_NONE ? 0u : in->lane_seg ? in->lane_seg : LANE_SEG_DEFAULT;
    if (nq == 0) {
        if (Kp) fail(ACC_E_ARG, "query key_off must start at 0, be non-decreasing and end at n_pairs");
        if (NR) fail(ACC_E_ARG, "query rng_off must start at 0, be non-decreasing and end at n_ranges");
        empty_result(ctx, view);
        return;
    }

    Queries Q{};
    Q.nq = nq;
    stage_ids(ctx, Q, in->txn_id, in->execute_at, nq, mem);
    Ranges R{};
    uint64_t *errs = ctx->get<uint64_t>("cq_errs", 1);
    uint64_t *xkey = nullptr;
    const uint64_t covered = expand_queries(ctx, s, Q, R, Parts{ in->key_off, in->key_code, in->rng_off, in->rng_start, in->rng_end, Kp, NR,
                                                                  in->end_inclusive, mem }, KINDS_WITNESSES, errs, xkey);
    const uint32_t Xp = Q.Qp;

    // ---- expand: every pair's query, key and segment; the lane tier's pairs
    uint64_t *nlane = ctx->get<uint64_t>("cq_nlane", 1);
    ACC_HIP(hipMemsetAsync(nlane, 0, 8, st));
    Located L = located_bufs(ctx, Xp, lane_seg != 0);   // ACC_CFQ_LANE_NONE: every pair takes the chunk path
    L.nlane = nlane;
    if (Xp)
        launch(ctx, "cq_rexpand", k_cq_rexpand, dim3(grid_for(Xp, BLOCK)), dim3(BLOCK), 0, Q, R, s, lane_seg, xkey, L.pair_q, L.pair_a,
               L.pair_w, L.pair_t0, L.chunks, L.lane, L.lane_w, nlane);
    const uint64_t lane_pairs = scan_located(ctx, s, Q, L, errs, view);
    ctx->stat("cfq.range_pairs", covered);
    ctx->stat("cfq.lane_pairs", lane_pairs);
}

// The pairs' chunk offsets, the chunk total (the one host read: rb's sync, which completes what the caller queued on rb
// before) and the chunk -> pair map
static uint64_t chunk_layout(acc_ctx *ctx, ReadBack &rb, uint32_t Qp, const uint64_t *chunks, uint64_t *&chunk_off, uint32_t *&chunk_item)
{
    hipStream_t st = ctx->stream;
    chunk_off = ctx->get<uint64_t>("cq_chunk_off", (size_t)Qp + 1);
    if (Qp) scan<uint64_t, OpAdd<uint64_t>>(ctx, chunks, chunk_off, Qp, true, chunk_off + Qp);
    else ACC_HIP(hipMemsetAsync(chunk_off, 0, 8, st));
    const auto h_nc = rb.u64(chunk_off + Qp);
    rb.wait();
    const uint64_t NC = h_nc;
    if (NC >= (1ull << 33)) fail(ACC_E_CAP, "the queries read too many segment entries in one call (>= 2^41)");
    chunk_item = ctx->get<uint32_t>("cq_chunk_item", NC);
    if (NC) launch(ctx, "cq_items", k_cq_items, dim3(grid_for(Qp, BLOCK)), dim3(BLOCK), 0, Qp, (const uint64_t *)chunk_off, chunk_item);
    return NC;
}

// what build_keydeps hands the entry's emit pass, and what it reports back for the entry's stats
struct EmitArgs {
    const uint64_t *chunk_eoff, *epos, *gcnt, *goff;
    int tb;
    uint32_t *hit;
    uint64_t *gkey;
};

struct Built {
    uint64_t hits, sorted_hits;
};

// KeyDeps.Builder per query from the per-chunk counts of emitted entries (chunk_cnt, NC of them; the pairs' chunks at
// chunk_off): every offset, then emit(EmitArgs) writes each emitted entry's view index into its hit slot (and its
// (query, index) key when the query sorts), then the header, the one-wave tier up to cfq_wave_cap hits, the radix-sort
// tier beyond it, the unique scan, dep_txn, u_off and the view. Both scans of the resident store end here.
template <class Emit>
static Built build_keydeps(acc_ctx *ctx, const CfkResident &s, const Queries &Q, const uint32_t *pair_q, const uint64_t *chunk_off,
                           const uint64_t *chunk_cnt, uint64_t NC, uint64_t *errs, acc_keydeps_view *view, Emit emit)
{
    hipStream_t st = ctx->stream;
    const uint32_t nq = Q.nq, Qp = Q.Qp;
    uint32_t cap = ctx->opts.cfq_wave_cap ? ctx->opts.cfq_wave_cap : CAP_MAX;
    cap = std::min(cap, CAP_MAX);
    uint64_t *arena_off = ctx->get<uint64_t>("cq_arena_off", (size_t)nq + 1);
    uint64_t *kd_off = ctx->get<uint64_t>("cq_kd_off", (size_t)nq + 1);
    uint64_t *u_off = ctx->get<uint64_t>("cq_u_off", (size_t)nq + 1);
    uint64_t *chunk_eoff = ctx->get<uint64_t>("cq_chunk_eoff", NC + 1);
    if (NC) scan<uint64_t, OpAdd<uint64_t>>(ctx, chunk_cnt, chunk_eoff, NC, true, chunk_eoff + NC);
    else ACC_HIP(hipMemsetAsync(chunk_eoff, 0, 8, st));
    uint64_t *epos = ctx->get<uint64_t>("cq_epos", (size_t)Qp + 1);
    uint64_t *kept = ctx->get<uint64_t>("cq_kept", Qp);
    uint64_t *kpos = ctx->get<uint64_t>("cq_kpos", (size_t)Qp + 1);
    launch(ctx, "cq_epos", k_cq_epos, dim3(grid_for((size_t)Qp + 1, BLOCK)), dim3(BLOCK), 0, Qp, chunk_off,
           (const uint64_t *)chunk_eoff, epos, kept);
    if (Qp) scan<uint64_t, OpAdd<uint64_t>>(ctx, kept, kpos, Qp, true, kpos + Qp);
    else ACC_HIP(hipMemsetAsync(kpos, 0, 8, st));
    uint64_t *gcnt = ctx->get<uint64_t>("cq_gcnt", nq);
    uint64_t *goff = ctx->get<uint64_t>("cq_goff", (size_t)nq + 1);
    launch(ctx, "cq_qoff", k_cq_qoff, dim3(grid_for((size_t)nq + 1, BLOCK)), dim3(BLOCK), 0, nq, Q.off, (const uint64_t *)kpos,
           (const uint64_t *)epos, cap, arena_off, kd_off, gcnt);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, gcnt, goff, nq, true, goff + nq);
    ReadBack rb_sizes(ctx);
    const auto h_errs = rb_sizes.u64(errs), h_e = rb_sizes.u64(chunk_eoff + NC), h_tk = rb_sizes.u64(kpos + Qp), h_g = rb_sizes.u64(goff + nq);
    rb_sizes.wait();
    check_cq_errors(h_errs);
    const uint64_t E = h_e, TK = h_tk, G = h_g;
    if (TK + E >= 0x7FFFFFFFull) fail(ACC_E_CAP, "more than 2^31-1 KeyDeps ints in one call");

    // ---- emit
    const int tb = std::max(1, bits_for(s.n_txn ? s.n_txn - 1 : 0));
    const int qbits = bits_for(nq - 1);
    uint32_t *hit = ctx->get<uint32_t>("cq_hit", E);
    uint64_t *gkey = ctx->get<uint64_t>("cq_gkey", G);
    if (E) emit(EmitArgs{ chunk_eoff, epos, gcnt, goff, tb, hit, gkey });

    // ---- KeyDeps.Builder layout
    int32_t *arena = ctx->get<int32_t>("cq_arena", TK + E);
    uint32_t *key_idx = ctx->get<uint32_t>("cq_key_idx", TK);
    uint64_t *kd_key = ctx->get<uint64_t>("cq_kd_key", TK);
    uint32_t *dep_txn = ctx->get<uint32_t>("cq_dep_txn", E);
    uint64_t TU = 0;
    if (E) {
        launch(ctx, "cq_header", k_cq_header, dim3(grid_for(Qp, BLOCK)), dim3(BLOCK), 0, Q, pair_q,
               (const uint64_t *)kpos, (const uint64_t *)epos, (const uint64_t *)arena_off, arena, key_idx, kd_key);
        uint32_t *uflag = ctx->get<uint32_t>("cq_uflag", E);
        uint32_t *uval = ctx->get<uint32_t>("cq_uval", E);
        uint32_t *upos = ctx->get<uint32_t>("cq_upos", E + 1);
        if (E > G)
            launch_waves(ctx, "cq_build_wave", k_cq_build_wave, nq, nq, Q.off, (const uint64_t *)epos, (const uint64_t *)arena_off,
                         (const uint64_t *)kd_off, cap, (const uint32_t *)hit, arena, uflag, uval);
        if (G) {
            const uint64_t *sk = radix_sort_keys(ctx, "cq_rs", gkey, G, 0, tb + qbits);
            uint32_t *gflag = ctx->get<uint32_t>("cq_gflag", G);
            uint32_t *ginc = ctx->get<uint32_t>("cq_ginc", G);
            launch(ctx, "cq_guniq", k_cq_guniq, dim3(grid_for(G, BLOCK)), dim3(BLOCK), 0, G, sk, tb, Q.off, (const uint64_t *)epos,
                   (const uint64_t *)goff, gflag, uflag, uval);
            scan<uint32_t, OpAdd<uint32_t>>(ctx, gflag, ginc, G, false);
            launch(ctx, "cq_gbody", k_cq_gbody, dim3(grid_for(G, BLOCK)), dim3(BLOCK), 0, G, (const uint64_t *)gkey, sk,
                   (const uint32_t *)ginc, tb, (const uint64_t *)gcnt, (const uint64_t *)goff, (const uint64_t *)arena_off,
                   (const uint64_t *)kd_off, arena);
        }
        scan<uint32_t, OpAdd<uint32_t>>(ctx, uflag, upos, E, true, upos + E);
        launch(ctx, "cq_deps", k_cq_deps, dim3(grid_for(E, BLOCK)), dim3(BLOCK), 0, E, (const uint32_t *)uflag, (const uint32_t *)uval,
               (const uint32_t *)upos, dep_txn);
        launch(ctx, "cq_uoff", k_cq_uoff, dim3(grid_for((size_t)nq + 1, BLOCK)), dim3(BLOCK), 0, nq, Q.off, (const uint64_t *)epos,
               (const uint32_t *)upos, u_off);
        ReadBack rb_uniq(ctx);
        const auto h_tu = rb_uniq.u32(upos + E);
        rb_uniq.wait();
        TU = h_tu;
    } else {
        ACC_HIP(hipMemsetAsync(u_off, 0, ((size_t)nq + 1) * 8, st));
        ctx->sync();
    }
    *view = acc_keydeps_view{ nq, TK + E, TK, TU, E, arena_off, arena, kd_off, key_idx, u_off, dep_txn, kd_key };
    ctx->kd_view = *view;
    ctx->kd_valid = true;
    return Built{ E, G };
}

// From the located pairs on: chunk offsets, M and the tie count, the count pass, then emit and KeyDeps.Builder. Returns
// the lane tier's pairs (L.nlane, read back at the chunk layout's sync).
static uint64_t scan_located(acc_ctx *ctx, const CfkResident &s, const Queries &Q, const Located &L, uint64_t *errs, acc_keydeps_view *view)
{
    const uint64_t wl0 = ctx->wave_launches;
    const uint32_t Qp = Q.Qp;
    uint64_t *chunk_off = nullptr;
    uint32_t *chunk_item = nullptr;
    ReadBack rb_chunks(ctx);
    ReadBack::Word<uint64_t> h_lane;
    if (L.nlane) h_lane = rb_chunks.u64(L.nlane);
    const uint64_t NC = chunk_layout(ctx, rb_chunks, Qp, L.chunks, chunk_off, chunk_item);
    const uint64_t lane_pairs = h_lane;
    const Pairs P{ L.pair_q, L.pair_a, L.pair_w, chunk_off, chunk_item, Qp };
    const Lanes lanes{ L.lane, L.lane_w };

    // ---- M and the tie count, the count pass
    Part part{ ctx->get<uint64_t>("cq_part_m", NC), ctx->get<uint64_t>("cq_part_l", NC), ctx->get<int32_t>("cq_part_n", NC),
               ctx->get<uint32_t>("cq_part_f", NC) };
    uint64_t *chunk_cnt = ctx->get<uint64_t>("cq_chunk_cnt", NC);
    if (NC) {
        launch_waves(ctx, "cq_max", k_cq_max, NC, NC, Q, s, P, (const uint8_t *)L.pair_t0, part, chunk_cnt, errs);
        launch_waves(ctx, "cq_fold", k_cq_fold, Qp, P, part, errs);
        launch_waves(ctx, "cq_count", k_cq_count, NC, NC, Q, s, P, part, chunk_cnt);
        if (L.lane)
            launch(ctx, "cq_lane_max", k_cq_lane_max, dim3(grid_for(Qp, BLOCK)), dim3(BLOCK), 0, Q, s, P, lanes, part, chunk_cnt, errs);
    }
    const Built b = build_keydeps(ctx, s, Q, L.pair_q, chunk_off, chunk_cnt, NC, errs, view, [&](const EmitArgs &e) {
        launch_waves(ctx, "cq_emit", k_cq_emit, NC, NC, Q, s, P, part, e.chunk_eoff, e.epos, e.gcnt, e.goff, e.tb, e.hit, e.gkey);
        if (L.lane)
            launch(ctx, "cq_lane_emit", k_cq_lane_emit, dim3(grid_for(Qp, BLOCK)), dim3(BLOCK), 0, Q, s, P, lanes, part, e.chunk_eoff,
                   e.epos, e.gcnt, e.goff, e.tb, e.hit, e.gkey);
    });
    ctx->stat("cfq.pairs", Qp);
    ctx->stat("cfq.chunks", NC);
    ctx->stat("cfq.hits", b.hits);
    ctx->stat("cfq.sorted_hits", b.sorted_hits);
    ctx->stat("cfq.wave_launches", ctx->wave_launches - wl0);
    return lane_pairs;
}

// ================================================================ acc_cfk_map_reduce_full: the recovery scans
// CommandsForKey.mapReduceFull (local/CommandsForKey.java:553-612) for a batch of BeginRecovery queries
// (messages/BeginRecovery.java:330-380) on the resident segments, the recovery counterpart of the scan above. The
// front end is acc_cfk_keydeps_mixed's (rvalidate, rbounds, rcount, pair_segment); the rest:
//   window   per pair: pos = the lower bound of X = testTxnId among the segment's TxnIds, isKnown = the entry there
//            compares equal to X; the window TestStartedAt admits ([start, pos), [pos, end) or the segment; nothing for
//            WITH when X is no member), its 256-entry chunks. Every pair takes the chunk path.
//   count    one wave per chunk, four entries per lane: the per-entry tests (cfk_entry_passes, recovery_pred.hpp, over
//            cr::View), cheapest first (status, hasInfo, kind, executeAt > X), and only for WITH / WITHOUT entries that
//            passed them the binary search of X in the entry's missing[] (raw TxnIds, read in place; divergent per lane
//            by nature)
//   emit     the same walk (k_cr_scan<true>), compacting in position order; each entry as its store-view index (view_index)
//   build    build_keydeps. No M pass and no tie rule.

namespace cr {

__global__ __launch_bounds__(BLOCK) void k_cr_window(Queries Q, Ranges R, CfkResident s, RcParams p, uint64_t *__restrict__ x_key,
                                                     uint32_t *__restrict__ pair_q, uint32_t *__restrict__ pair_a,
                                                     uint32_t *__restrict__ pair_w, uint64_t *__restrict__ chunks)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= Q.Qp) return;
    uint32_t q, a = 0, w = 0;
    uint64_t k;
    bool range;
    const uint32_t seg = pair_segment(Q, R, s, i, q, k, range);
    if (seg < s.nk) {
        const uint32_t s0 = s.ent_off[seg], s1 = s.ent_off[seg + 1];
        const uint64_t Xm = Q.qm[q], Xl = Q.ql[q];
        const int32_t Xn = Q.qn[q];
        // Arrays.binarySearch(txns, testTxnId): found <=> X is a member; pos = its index or the insert point
        const uint32_t x = lower_bound_ts(s.em, s.el, s.en, s0, s1, Ts{ Xm, Xl, Xn });
        const bool known = x < s1 && ts_cmp(s.em[x], s.el[x], s.en[x], Xm, Xl, Xn) == 0;
        if (known || p.test_dep != ACC_DEP_WITH) {
            const uint32_t start = p.started_at == ACC_STARTED_AFTER ? x : s0;
            const uint32_t end = p.started_at == ACC_STARTED_BEFORE ? x : s1;
            a = start;
            w = end - start;
        }
    }
    x_key[i] = k;
    pair_q[i] = q;
    pair_a[i] = a;
    pair_w[i] = w;
    chunks[i] = (w + CH - 1) / CH;
}

struct Scan {
    uint32_t base, end, q, mask;
    uint64_t Xm, Xl;
    int32_t Xn;
};

__device__ __forceinline__ Scan scan_ctx(uint64_t cw, const Queries &Q, const Pairs &P, const RcParams &p)
{
    Scan c;
    const uint32_t item = P.item[cw];
    c.q = P.q[item];
    c.base = P.a[item] + (uint32_t)(cw - P.chunk_off[item]) * CH;
    c.end = P.a[item] + P.w[item];
    c.Xm = Q.qm[c.q]; c.Xl = Q.ql[c.q]; c.Xn = Q.qn[c.q];
    const int by = p.test_kinds < 0 ? witnessed_by((uint32_t)(c.Xl >> 1) & 7u) : p.test_kinds;   // validated: >= 0
    c.mask = (uint32_t)by;
    return c;
}

// one chunk's query against the resident segments, as cfk_entry_passes reads them: the status byte, the TxnId word's
// kind bits, the raw executeAt and missing[] columns
struct View {
    const CfkResident &s;
    const Scan &c;
    uint32_t mask;
    __device__ __forceinline__ uint32_t status(uint32_t e) const { return s.st[e]; }
    __device__ __forceinline__ uint32_t kind(uint32_t e) const { return (uint32_t)(s.el[e] >> 1) & 7u; }
    __device__ __forceinline__ bool executes_after_x(uint32_t e) const
    {
        return ts_cmp(s.xm[e], s.xl[e], s.xn[e], c.Xm, c.Xl, c.Xn) > 0;
    }
    __device__ __forceinline__ bool x_in_missing(uint32_t e) const
    {
        uint32_t lo = s.miss_off[e], hi = s.miss_off[e + 1];
        while (lo < hi) {
            const uint32_t m = (lo + hi) >> 1;
            const int d = ts_cmp(s.mm[m], s.ml[m], s.mn[m], c.Xm, c.Xl, c.Xn);
            if (d < 0) lo = m + 1; else if (d > 0) hi = m; else return true;
        }
        return false;
    }
};

// one wave per chunk evaluates the entry predicate. Count: the chunk's matches. Emit: the same walk, compacting in
// position order, each entry as its store-view index (and its (query, index) key when the query sorts)
template <bool EMIT>
__global__ __launch_bounds__(BLOCK) void k_cr_scan(uint64_t first, uint64_t nchunks, Queries Q, CfkResident s, Pairs P, RcParams p,
                                                   uint64_t *__restrict__ chunk_cnt, const uint64_t *__restrict__ chunk_eoff,
                                                   const uint64_t *__restrict__ epos, const uint64_t *__restrict__ gcnt,
                                                   const uint64_t *__restrict__ goff, int tb, uint32_t *__restrict__ hit,
                                                   uint64_t *__restrict__ gkey)
{
    const uint64_t cw = first + (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (cw >= nchunks) return;
    const Scan c = scan_ctx(cw, Q, P, p);
    const View v{ s, c, c.mask };
    const uint64_t lt = (1ull << lane_id()) - 1;
    uint32_t cnt = 0;
    uint64_t out = 0, gbase = 0;
    bool big = false;
    if constexpr (EMIT) {
        out = chunk_eoff[cw];
        if (chunk_eoff[cw + 1] == out) return;
        big = gcnt[c.q] != 0;
        gbase = big ? goff[c.q] - epos[Q.off[c.q]] : 0;   // hit slot -> slot among the sorting tier's hits
    }
#pragma unroll
    for (uint32_t u = 0; u < CH / 64; ++u) {
        const uint32_t e = c.base + u * 64 + lane_id();
        const bool m = e < c.end && cfk_entry_passes(v, p, e);
        const uint64_t bal = __ballot(m);
        if constexpr (EMIT) {
            if (m) {
                const uint32_t lo = view_index(s, e);
                const uint64_t o = out + (uint64_t)__popcll(bal & lt);
                hit[o] = lo;
                if (big) gkey[gbase + o] = ((uint64_t)c.q << tb) | lo;
            }
            out += (uint64_t)__popcll(bal);
        } else {
            cnt += (uint32_t)__popcll(bal);
        }
    }
    if constexpr (!EMIT) {
        if (lane_id() == 0) chunk_cnt[cw] = cnt;
    }
}

}  // namespace cr

void cfk_map_reduce_full(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_recovery_in *in, acc_keydeps_view *view)
{
    if (!cfk || !in || !view) fail(ACC_E_ARG, "null argument");
    const CfkResident s = resident_checked(cfk, in->mem);
    if (in->end_inclusive > 1) fail(ACC_E_ARG, "end_inclusive must be 0 or 1");
    const RcParams prm = recovery_params(in->started_at, in->test_dep, in->test_status, in->flags, in->test_kinds);
    if (in->n_pairs >= 0xFFFFFFFFull) fail(ACC_E_CAP, "too many (query, key) pairs in one call (>= 2^32 - 1)");
    if (in->n_ranges >= 0xFFFFFFFFull) fail(ACC_E_CAP, "too many ranges in one call (>= 2^32 - 1)");
    const uint64_t wl0 = ctx->wave_launches;
    ctx->kd_valid = false;
    const uint32_t nq = in->n_query, mem = in->mem;
    if (nq == 0) {
        if (in->n_pairs) fail(ACC_E_ARG, "query key_off must start at 0, be non-decreasing and end at n_pairs");
        if (in->n_ranges) fail(ACC_E_ARG, "query rng_off must start at 0, be non-decreasing and end at n_ranges");
        empty_result(ctx, view);
        return;
    }

    Queries Q{};
    Q.nq = nq;
    stage_ids(ctx, Q, in->test_txn, acc_ts_cols{ nullptr, nullptr, nullptr }, nq, mem);
    Ranges R{};
    uint64_t *errs = ctx->get<uint64_t>("cq_errs", 1);
    uint64_t *xkey = nullptr;
    const uint64_t covered = expand_queries(ctx, s, Q, R, Parts{ in->key_off, in->key_code, in->rng_off, in->rng_start, in->rng_end,
                                                                  (uint32_t)in->n_pairs, (uint32_t)in->n_ranges, in->end_inclusive, mem },
                                            prm.test_kinds < 0 ? KINDS_WITNESSED_BY : KINDS_UNCHECKED, errs, xkey);
    const uint32_t Qp = Q.Qp;

    // ---- window: pos, isKnown, the entries TestStartedAt admits, their chunks
    uint32_t *pair_q = ctx->get<uint32_t>("cq_pair_q", Qp), *pair_a = ctx->get<uint32_t>("cq_pair_a", Qp);
    uint32_t *pair_w = ctx->get<uint32_t>("cq_pair_w", Qp);
    uint64_t *chunks = ctx->get<uint64_t>("cq_chunks", Qp);
    if (Qp)
        launch(ctx, "cr_window", cr::k_cr_window, dim3(grid_for(Qp, BLOCK)), dim3(BLOCK), 0, Q, R, s, prm, xkey, pair_q, pair_a, pair_w,
               chunks);
    uint64_t *chunk_off = nullptr;
    uint32_t *chunk_item = nullptr;
    ReadBack rb_chunks(ctx);
    const uint64_t NC = chunk_layout(ctx, rb_chunks, Qp, chunks, chunk_off, chunk_item);
    const Pairs P{ pair_q, pair_a, pair_w, chunk_off, chunk_item, Qp };

    // ---- count, then emit and KeyDeps.Builder
    uint64_t *chunk_cnt = ctx->get<uint64_t>("cq_chunk_cnt", NC);
    const uint64_t *none = nullptr;   // the emit pass's arguments
    if (NC) launch_waves(ctx, "cr_count", cr::k_cr_scan<false>, NC, NC, Q, s, P, prm, chunk_cnt, none, none, none, none, 0, (uint32_t *)nullptr, (uint64_t *)nullptr);
    const Built b = build_keydeps(ctx, s, Q, pair_q, chunk_off, chunk_cnt, NC, errs, view, [&](const EmitArgs &e) {
        launch_waves(ctx, "cr_emit", cr::k_cr_scan<true>, NC, NC, Q, s, P, prm, (uint64_t *)nullptr, e.chunk_eoff, e.epos, e.gcnt,
                     e.goff, e.tb, e.hit, e.gkey);
    });
    ctx->stat("cfr.pairs", Qp);
    ctx->stat("cfr.chunks", NC);
    ctx->stat("cfr.hits", b.hits);
    ctx->stat("cfr.sorted_hits", b.sorted_hits);
    ctx->stat("cfr.range_pairs", covered);
    ctx->stat("cfr.wave_launches", ctx->wave_launches - wl0);
}

}  // namespace acc

