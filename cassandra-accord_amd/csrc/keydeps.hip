// keydeps.hip — batched PreAccept.calculatePartialDeps on CDNA4.
//
// For every txn T of a batch (one CommandsForKey snapshot), for every key k of T:
//   deps(T,k) = CommandsForKey.mapReduceActive(startedBefore = T.executeAt, T.kind().witnesses())
//               (local/CommandsForKey.java:614-650) minus p1 (messages/PreAccept.java:253-259),
// then the KeyDeps.Builder result (utils/RelationMultiMap.java:88-260) in Java layout.
//
// This file holds the CFK build and the run-based path with its tiers. The stages, each a host function over one
// record (CfkBuild, keydeps.hpp):
//   build_cfk      argument checks; staged inputs; prep and the order-rank dictionary of the 2N timestamps
//                  (dictionary.hip); the pairs sorted by (key, TxnId rank) by one of five sorts (sort_pairs); the
//                  columns: one segment per key = CommandsForKey.txns, tile counts, the run-based scan's class lists,
//                  rank directory and bumped committed list (build_columns). A TxnId-ordered batch with a packed pair
//                  sort runs the dictionary, and behind it the bumped committed (segment, executeAt) order made from
//                  the txn side (bc_from_txns), on the context's side lane beside the pair sort; the lane is still
//                  open when build_cfk returns and the next stage joins it (acc_ctx::lane_join).
//   keydeps_runs   no executeAt ties: a query is a union of sorted runs over its segment (see "v2" below). Count pass
//                  (a record per pair), mark pass and scans (result sizes, stream txns / big txns), then the stream
//                  passes on the context stream while the big txns' tiers (window, sorting, wave) run on a side
//                  stream, and the TxnId compaction; the sorting tiers and the global fallback follow only for txns
//                  the first round passed on.
//   keydeps_replay (keydeps_replay.hip) executeAt ties, where the reference's FAST bisection is order-dependent, or
//                  ACC_OPT_FORCE_REPLAY: the exact replay of every (T, k) query.
// keydeps_batch = build_cfk, then keydeps_of (replay or runs). keydeps_mixed (keydeps_mixed.hip) = the same with segment
// keys and the sparse compaction, then its range part. cfk_snapshot = build_cfk alone.
//
// Host syncs of a tie-free batch, and what each one reads:
//   1. prep (prep_batch): the varying-bit masks of the timestamp and key words, validation errors, sortedness,
//      the number of executeAts that differ from their TxnId, the keys of the bumped committed txns: they pick the
//      dictionary and the pair sort and size the side lane's sort.
//   2. columns (build_columns): the tile totals (bumped committed count: the size of the next sort), the error and
//      tie words of the dictionary kernels. A sorted-batch dictionary that met a tie is redone by the general sort
//      here and the columns built again (one more sync).
//   3. sizes (keydeps_runs): E, the number of big txns and of stream txns with a run record, the 9-16-key flag: they
//      size the result arrays and pick the launches. The host waits on an event behind the copy: the lean stream
//      pass, which needs none of them, is already enqueued and runs meanwhile (from a context's second call on).
//   4. compaction (finish): the result totals, gather-count checks, the tiers' counts. Again after the sorting tiers
//      or the global fallback (which has one sync of its own), when the first round left txns to them.
// The replay path has syncs 1 and 2, then one for E and one for the result totals.
#include "keydeps.hpp"

#include <vector>

namespace acc {

// ---------------------------------------------------------------- CFK build

// the per-txn record k_txn_info writes, done by k_pair_keys' first n threads when tinfo is set (one launch fewer)
struct TxnInfoArgs {
    uint32_t n = 0;
    const uint8_t *status = nullptr;
    const uint64_t *tl = nullptr;
    uint4 *tinfo = nullptr;
    uint32_t *bigflag = nullptr;
};

__device__ __forceinline__ void txn_info_one(uint32_t t, uint32_t n, const uint32_t *rank, const uint8_t *status,
                                             const uint64_t *tl, const uint32_t *key_off, uint4 *tinfo, uint32_t *bigflag)
{
    if (bigflag) bigflag[t] = 0;
    const uint32_t kind = (uint32_t)(tl[t] >> 1) & 7u;
    tinfo[t] = make_uint4(rank[t], rank[n + t], (uint32_t)status[t] | (kind << 3), key_off[t]);
}

__global__ __launch_bounds__(BLOCK) void k_pair_keys(size_t P, const uint64_t *__restrict__ key_code,
                                                     const uint32_t *__restrict__ owner, const uint32_t *__restrict__ key_off,
                                                     const uint32_t *__restrict__ rank,
                                                     const uint32_t *__restrict__ perm, PairPlan plan,
                                                     int rank_only, uint64_t *__restrict__ out, TxnInfoArgs ti)
{
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (ti.tinfo && i < ti.n) txn_info_one((uint32_t)i, ti.n, rank, ti.status, ti.tl, key_off, ti.tinfo, ti.bigflag);
    if (i >= P) return;
    size_t j = perm ? perm[i] : i;
    if (rank_only) { out[i] = rank[owner[j]]; return; }
    uint64_t kc = pext_runs(key_code[j], plan.rk);
    if (plan.mode == 4) {
        const uint32_t t = owner[j];
        out[i] = (kc << 32) | ((uint64_t)t << plan.sb) | (uint64_t)(j - key_off[t]);
        return;
    }
    out[i] = plan.mode == 1 ? ((kc << plan.rbits) | rank[owner[j]]) : plan.mode == 3 ? ((kc << 32) | i) : kc;
}

// packed (key << 32 | pair index) sort output: segment-start flags and the permutation
// sb >= 0 (mode 4): the low word is owner << sb | slot; the pair index is key_off[owner] + slot, the owner goes to pown
__global__ __launch_bounds__(BLOCK) void k_seg_flags_packed(size_t P, const uint64_t *__restrict__ sp, uint32_t *__restrict__ flag,
                                                            uint32_t *__restrict__ perm, int sb, const uint32_t *__restrict__ key_off,
                                                            uint32_t *__restrict__ pown)
{
    size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    const uint64_t x = sp[p];
    flag[p] = p == 0 || (x >> 32) != (sp[p - 1] >> 32);
    if (sb < 0) { perm[p] = (uint32_t)x; return; }
    const uint32_t t = (uint32_t)x >> sb, slot = (uint32_t)x & ((1u << sb) - 1u);
    perm[p] = key_off[t] + slot;
    pown[p] = t;
}

__global__ __launch_bounds__(BLOCK) void k_seg_flags(size_t P, const uint64_t *__restrict__ skeys, int key_shift,
                                                     uint32_t *__restrict__ flag)
{
    size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    flag[p] = p == 0 || (skeys[p] >> key_shift) != (skeys[p - 1] >> key_shift);
}

// Gather per-position CFK columns; fill seg_start; classify committed (C) / uncommitted (U).
// per-txn record for the CFK gather: one 16-B random read per pair instead of four
// .w = key_off[t] (the CFK gather turns (owner, slot) into the pair index from the same 16-B read)
// also zeroes the count pass's big-txn flags (no memset launch)
__global__ __launch_bounds__(BLOCK) void k_txn_info(uint32_t n, const uint32_t *__restrict__ rank, const uint8_t *__restrict__ status,
                                                    const uint64_t *__restrict__ tl, const uint32_t *__restrict__ key_off,
                                                    uint4 *__restrict__ tinfo, uint32_t *__restrict__ bigflag)
{
    uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < n) txn_info_one(t, n, rank, status, tl, key_off, tinfo, bigflag);
}

// per-pair copy of its txn's record, written in pair order (owner[] is monotone, so both reads stream): the CFK
// gather then does ONE random 16-B read per pair instead of the dependent owner[j] -> tinfo[owner[j]] pair
__global__ __launch_bounds__(BLOCK) void k_pair_tinfo(size_t P, const uint32_t *__restrict__ owner, const uint4 *__restrict__ tinfo,
                                                      uint4 *__restrict__ ptinfo)
{
    size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < P) ptinfo[j] = tinfo[owner[j]];
}

// inverse of the CFK permutation, only for the consumers that address pairs by index (exact replay, the global
// write tier, the range-domain KeyDeps): a random 4-B scatter per pair the common path does not pay
__global__ __launch_bounds__(BLOCK) void k_pair_pos(size_t P, const uint32_t *__restrict__ perm, uint32_t *__restrict__ pair_pos)
{
    size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p < P) pair_pos[perm[p]] = (uint32_t)p;
}

// ---------------------------------------------------------------- v2: run-based conflict scan
//
// Without executeAt ties (k_exec_ties), the reference scan of (T, k) equals the union of three kinds of
// sorted runs over the CFK segment (positions [s0, s1) in TxnId order), with S = T.executeAt,
// pos = insertPos(S), M = maxCommittedBefore and posM = first position with TxnId >= M:
//   R1[c]: uncommitted (HISTORICAL/PREACCEPTED/ACCEPTED) entries of kind class c in [s0, pos)
//   R2[c]: committed entries of kind class c in [posM, pos)   (TxnId >= M  =>  executeAt >= M)
//   R3   : committed entries before posM with executeAt >= M  (only "bumped" ones, executeAt != TxnId)
// for every class c witnessed by T.kind, minus T itself (p1). Runs are ranges of per-class position
// lists, so counts are O(1) prefix differences. M = max(last unbumped committed Write before pos
// [segmented prefix max], predecessor of S among bumped committed Writes [small sorted list]).

constexpr int NLIST = 6;   // U_R, U_W, U_S, C_R, C_W, C_S
constexpr int NCNT = 9;    // 6 list counts, bumped-committed count, last-unbumped-committed-write max, segment starts
constexpr int NRD = 8;     // the rank directory's columns (all but the segment count)
__device__ __forceinline__ bool cnt_is_max(int q) { return q == 7; }

// (kind_class: ts.hpp)
// witness mask over kinds -> mask over classes
__device__ __forceinline__ uint32_t wk_classes(uint32_t wk)
{
    return (wk & 1u) | (((wk >> 1) & 1u) << 1) | (((wk >> 3) & 1u) << 2);
}

// per-position code: bits 0-2 list id (7 = none), bit 3 bumped committed (class < 3), bit 4 unbumped committed Write
__device__ __forceinline__ uint32_t v2_code(uint32_t rank, uint32_t exec, uint32_t info)
{
    uint32_t st = info & 7u, kind = info >> 3, cls = kind_class(kind);
    bool u = st >= 1 && st <= 3, c = st >= 4 && st <= 6;
    uint32_t list = cls < 3 ? (u ? cls : c ? 3 + cls : 7u) : 7u;
    uint32_t bc = (c && cls < 3 && exec != rank) ? 1u : 0u;
    uint32_t ucw = (c && kind == 1 && exec == rank) ? 1u : 0u;
    return list | (bc << 3) | (ucw << 4);
}

constexpr int V2_ITEMS = 4;               // consecutive positions per thread: one 16-B load per column
constexpr int V2_TILE = BLOCK * V2_ITEMS;

// 4 consecutive positions' codes (s_rank / s_exec / s_info are allocated with 4 entries of padding)
// bqm: bit i set when position base + i is a bumped query (executeAt != TxnId)
__device__ __forceinline__ void v2_codes4(size_t P, size_t base, const uint32_t *__restrict__ s_rank, const uint32_t *__restrict__ s_exec,
                                          const uint8_t *__restrict__ s_info, uint32_t (&code)[V2_ITEMS], uint32_t (&rk)[V2_ITEMS],
                                          uint32_t &bqm)
{
    uint4 r = *reinterpret_cast<const uint4 *>(s_rank + base);
    uint4 e = *reinterpret_cast<const uint4 *>(s_exec + base);
    uint32_t inf = *reinterpret_cast<const uint32_t *>(s_info + base);
    rk[0] = r.x; rk[1] = r.y; rk[2] = r.z; rk[3] = r.w;
    const uint32_t ex[4] = { e.x, e.y, e.z, e.w };
    bqm = 0;
#pragma unroll
    for (int i = 0; i < V2_ITEMS; ++i) {
        code[i] = base + i < P ? v2_code(rk[i], ex[i], (inf >> (8 * i)) & 0xFFu) : 7u;
        bqm |= (base + i < P && ex[i] != rk[i] ? 1u : 0u) << i;
    }
}

// The CFK columns of four consecutive positions per thread (s_rank / s_exec / s_info from the per-pair txn records, the
// segment starts, optionally pair_pos) and the per-tile counts of the class lists (the multi-scan's reduce step) over
// the same 1024-position tile that k_v2_apply scans.
// pown (mode 4): each position's owner txn, its record read from tinfo (16 B per txn) instead of ptinfo (per pair)
// sp (mode 4, sb >= 0): the sorted packed pair keys (key << 32 | owner << sb | slot) are unpacked here: the segment
// flags and the pair index perm = key_off[owner] + slot are written, key_off[owner] coming with the owner's record
// (tinfo[t].w), so each pair costs one random 16-B read. Otherwise perm / seg_flag are inputs and the record is
// ptinfo[perm].
__global__ __launch_bounds__(BLOCK) void k_cfk_gather4(size_t P, uint32_t *__restrict__ perm, const uint4 *__restrict__ ptinfo,
                                                       const uint64_t *__restrict__ sp, int sb, const uint4 *__restrict__ tinfo,
                                                       uint32_t *__restrict__ seg_flag, uint32_t *__restrict__ s_rank,
                                                       uint32_t *__restrict__ s_exec, uint8_t *__restrict__ s_info,
                                                       uint32_t *__restrict__ pair_pos, uint32_t *__restrict__ tile_sums,
                                                       uint32_t ntiles)
{
    __shared__ uint32_t lds[WAVES];
    const size_t base = (size_t)blockIdx.x * V2_TILE + (size_t)threadIdx.x * V2_ITEMS;
    uint32_t c[NCNT] = {};
    if (base < P) {
        uint32_t j[V2_ITEMS], fl[V2_ITEMS];
        uint4 ti[V2_ITEMS];
        if (sp) {
            uint64_t x[V2_ITEMS];
            const uint64_t xp = base > 0 ? sp[base - 1] : 0;
#pragma unroll
            for (int i = 0; i < V2_ITEMS; ++i) x[i] = base + i < P ? sp[base + i] : 0;
            const uint32_t smask = (1u << sb) - 1u;
#pragma unroll
            for (int i = 0; i < V2_ITEMS; ++i) {
                const bool in = base + i < P;
                const uint64_t prev = i == 0 ? xp : x[i - 1];
                fl[i] = in && (base + i == 0 || (x[i] >> 32) != (prev >> 32)) ? 1u : 0u;
                ti[i] = in ? tinfo[(uint32_t)x[i] >> sb] : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int i = 0; i < V2_ITEMS; ++i) j[i] = ti[i].w + ((uint32_t)x[i] & smask);
            if (base + V2_ITEMS <= P) {
                *reinterpret_cast<uint4 *>(seg_flag + base) = make_uint4(fl[0], fl[1], fl[2], fl[3]);
                *reinterpret_cast<uint4 *>(perm + base) = make_uint4(j[0], j[1], j[2], j[3]);
            } else {
#pragma unroll
                for (int i = 0; i < V2_ITEMS; ++i)
                    if (base + i < P) { seg_flag[base + i] = fl[i]; perm[base + i] = j[i]; }
            }
        } else {
#pragma unroll
            for (int i = 0; i < V2_ITEMS; ++i) {
                const bool in = base + i < P;
                j[i] = in ? perm[base + i] : 0u;
                fl[i] = in ? seg_flag[base + i] : 0u;
            }
#pragma unroll
            for (int i = 0; i < V2_ITEMS; ++i) ti[i] = base + i < P ? ptinfo[j[i]] : make_uint4(0u, 0u, 0u, 0u);
        }
        uint32_t inf = 0;
#pragma unroll
        for (int i = 0; i < V2_ITEMS; ++i) {
            const size_t p = base + i;
            if (p >= P) break;
            if (pair_pos) pair_pos[j[i]] = (uint32_t)p;
            c[8] += fl[i] != 0;
            inf |= (ti[i].z & 0xFFu) << (8 * i);
            const uint32_t code = v2_code(ti[i].x, ti[i].y, ti[i].z & 0xFFu);
            const uint32_t l = code & 7u;
#pragma unroll
            for (int q = 0; q < NLIST; ++q) c[q] += l == (uint32_t)q;
            c[6] += (code >> 3) & 1u;
            if ((code >> 4) & 1u) c[7] = (uint32_t)p + 1;
        }
        // the column arrays carry V2_ITEMS entries of padding: whole 16-B / 4-B stores
        *reinterpret_cast<uint4 *>(s_rank + base) = make_uint4(ti[0].x, ti[1].x, ti[2].x, ti[3].x);
        *reinterpret_cast<uint4 *>(s_exec + base) = make_uint4(ti[0].y, ti[1].y, ti[2].y, ti[3].y);
        *reinterpret_cast<uint32_t *>(s_info + base) = inf;
    }
#pragma unroll
    for (int q = 0; q < NCNT; ++q) {
        uint32_t total;
        if (!cnt_is_max(q)) block_exclusive(c[q], OpAdd<uint32_t>(), lds, total);
        else block_exclusive(c[q], OpMax<uint32_t>(), lds, total);
        if (threadIdx.x == 0) tile_sums[(size_t)q * ntiles + blockIdx.x] = total;
    }
}

// The per-position prefix columns as a rank directory: one 64-B chunk per RD_W = 32 CFK positions, = one HBM line
// (16 MB at config 2's 8M positions, instead of a 32-B row per position): words 0-7 = the 8 running values at the
// chunk's first position (exclusive prefix counts of the 6 class lists, the bumped-committed count, the last unbumped
// committed Write as pos+1: prefix max), words 8-15 = one bit plane per column over the chunk's positions (list
// membership, bumped committed, unbumped committed Write). A query's "row" at p is the chunk's running values plus the
// popcounts of the planes below p (the last set bit for the Write column): one line read and a few ALU ops.
constexpr int RW_CBC = 6, RW_LUCW = 7;
constexpr uint32_t RD_W = 32;

__global__ __launch_bounds__(BLOCK) void k_v2_apply(size_t P, const uint32_t *__restrict__ s_rank, const uint32_t *__restrict__ s_exec,
                                                    const uint8_t *__restrict__ s_info, const uint32_t *__restrict__ seg_flag,
                                                    const uint32_t *__restrict__ tile_pref, const uint32_t *__restrict__ totals,
                                                    uint32_t ntiles, int rbits, V2Cols o, uint32_t *__restrict__ seg_incl,
                                                    uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ perm,
                                                    const uint64_t *__restrict__ key_code, uint64_t *__restrict__ seg_key,
                                                    const uint64_t *__restrict__ sp, Runs krun, uint64_t rk_mask,
                                                    uint32_t *__restrict__ bases, uint64_t *__restrict__ z0, uint32_t nz0,
                                                    uint64_t *__restrict__ z1, uint32_t nz1, const uint64_t *__restrict__ g,
                                                    uint64_t *__restrict__ stage)
{
    __shared__ uint32_t lds[WAVES];
    if (blockIdx.x == 0) {
        // the list bases for the count pass (list l at [bases[l], bases[l] + totals[l]) of the class-list arrays), the
        // count / mark passes' accumulators zeroed, the dictionary's error / tie words staged beside the totals
        if (threadIdx.x == 0) {
            uint32_t b = 0;
            for (int l = 0; l < NLIST; ++l) { bases[l] = b; b += totals[l]; }
            bases[NLIST] = b;
        }
        for (uint32_t i = threadIdx.x; i < nz0; i += BLOCK) z0[i] = 0;
        for (uint32_t i = threadIdx.x; i < nz1; i += BLOCK) z1[i] = 0;
        if (threadIdx.x < 3) stage[threadIdx.x] = g[4 + threadIdx.x];
    }
    const size_t base = (size_t)blockIdx.x * V2_TILE + (size_t)threadIdx.x * V2_ITEMS;
    uint32_t code[V2_ITEMS] = { 7u, 7u, 7u, 7u }, rk[V2_ITEMS] = {};
    uint32_t c[NCNT] = {};
    uint32_t fl[V2_ITEMS] = {};
    uint64_t kc[V2_ITEMS] = {};
    uint32_t bqm = 0;
    if (base < P) {
        v2_codes4(P, base, s_rank, s_exec, s_info, code, rk, bqm);
#pragma unroll
        for (int i = 0; i < V2_ITEMS; ++i) {
            uint32_t l = code[i] & 7u;
#pragma unroll
            for (int q = 0; q < NLIST; ++q) c[q] += l == (uint32_t)q;
            c[6] += (code[i] >> 3) & 1u;
            if ((code[i] >> 4) & 1u) c[7] = (uint32_t)(base + i) + 1;
            fl[i] = base + i < P ? seg_flag[base + i] : 0u;
            c[8] += fl[i] != 0;
        }
        if (seg_key && sp) {
            // mode 4: the key code from the sorted pair key itself (its compacted bits deposited back over key_code[0]'s
            // constant bits; the varying bits all lie in the runs), a sequential read instead of a gather
            const uint64_t kconst = key_code[0] & ~rk_mask;
#pragma unroll
            for (int i = 0; i < V2_ITEMS; ++i)
                if (fl[i]) {
                    const uint64_t c = sp[base + i] >> 32;
                    uint64_t w = kconst;
                    for (int r = 0; r < krun.n; ++r) {
                        const uint64_t m = krun.len[r] >= 64 ? ~0ull : ((1ull << krun.len[r]) - 1);
                        w |= ((c >> krun.dst[r]) & m) << krun.lo[r];
                    }
                    kc[i] = w;
                }
        } else if (seg_key) {   // segment starts' key codes: the gathers issued here, their latency hidden by the block scans
            uint32_t pi[V2_ITEMS] = {};
            if (base + V2_ITEMS <= P) {
                const uint4 pv = *reinterpret_cast<const uint4 *>(perm + base);
                pi[0] = pv.x; pi[1] = pv.y; pi[2] = pv.z; pi[3] = pv.w;
            } else {
                for (int i = 0; i < V2_ITEMS; ++i) if (base + i < P) pi[i] = perm[base + i];
            }
#pragma unroll
            for (int i = 0; i < V2_ITEMS; ++i) if (fl[i]) kc[i] = key_code[pi[i]];
        }
    }
    uint32_t run[NCNT];
#pragma unroll
    for (int q = 0; q < NCNT; ++q) {
        uint32_t total;
        uint32_t pre = tile_pref[(size_t)q * ntiles + blockIdx.x];
        if (!cnt_is_max(q)) run[q] = pre + block_exclusive(c[q], OpAdd<uint32_t>(), lds, total);
        else { uint32_t e = block_exclusive(c[q], OpMax<uint32_t>(), lds, total); run[q] = e > pre ? e : pre; }
    }
    // rank directory: the chunk's running values from its first thread (RD_W / V2_ITEMS = 8 threads per chunk), the bit
    // planes OR-reduced over those 8 threads (threads past P contribute nothing)
    static_assert(RD_W == 8 * V2_ITEMS, "eight threads per directory chunk");
    {
        uint32_t pl[NRD] = {};
#pragma unroll
        for (int i = 0; i < V2_ITEMS; ++i) {
            const uint32_t l = code[i] & 7u;
#pragma unroll
            for (int q = 0; q < NLIST; ++q) pl[q] |= (l == (uint32_t)q ? 1u : 0u) << i;
            pl[6] |= ((code[i] >> 3) & 1u) << i;
            pl[7] |= ((code[i] >> 4) & 1u) << i;
        }
        const uint32_t sh = V2_ITEMS * (threadIdx.x & 7u);
#pragma unroll
        for (int q = 0; q < NRD; ++q) {
            uint32_t x = pl[q] << sh;
            x |= __shfl_xor(x, 1, 64);
            x |= __shfl_xor(x, 2, 64);
            x |= __shfl_xor(x, 4, 64);
            pl[q] = x;
        }
        if ((threadIdx.x & 7u) == 0 && base < P) {
            uint4 *ch = o.rdir + 4 * (base / RD_W);
            ch[0] = make_uint4(run[0], run[1], run[2], run[3]);
            ch[1] = make_uint4(run[4], run[5], run[6], run[7]);
            ch[2] = make_uint4(pl[0], pl[1], pl[2], pl[3]);
            ch[3] = make_uint4(pl[4], pl[5], pl[6], pl[7]);
        }
    }
    if (base >= P) return;
    uint32_t lb[NLIST];
    {
        uint32_t b = 0;
#pragma unroll
        for (int l = 0; l < NLIST; ++l) { lb[l] = b; b += totals[l]; }
    }
    uint32_t segi[V2_ITEMS];
#pragma unroll
    for (int i = 0; i < V2_ITEMS; ++i) {   // segment numbers (seg_incl = inclusive count of segment starts) and starts
        const size_t p = base + i;
        if (p >= P) break;
        if (fl[i]) {
            seg_start[run[8]] = (uint32_t)p;
            if (seg_key) seg_key[run[8]] = kc[i];   // the segment's key code (range-domain queries)
        }
        run[8] += fl[i] != 0;
        segi[i] = run[8];
        if (p == P - 1) seg_start[run[8]] = (uint32_t)P;
    }
    if (base + V2_ITEMS <= P) *reinterpret_cast<uint4 *>(seg_incl + base) = make_uint4(segi[0], segi[1], segi[2], segi[3]);
    else for (int i = 0; i < V2_ITEMS; ++i) if (base + i < P) seg_incl[base + i] = segi[i];
#pragma unroll
    for (int i = 0; i < V2_ITEMS; ++i) {
        size_t p = base + i;
        if (p >= P) break;
        uint32_t l = code[i] & 7u;
        uint32_t r = rk[i];
        if (l < NLIST) {
            uint32_t idx = 0;
#pragma unroll
            for (int q = 0; q < NLIST; ++q) if ((uint32_t)q == l) idx = lb[q] + run[q];
            o.list_rank[idx] = r;
#pragma unroll
            for (int q = 0; q < NLIST; ++q) run[q] += (uint32_t)q == l;
        }
        if ((code[i] >> 3) & 1u) {
            uint32_t b = run[6]++;
            uint32_t seg = segi[i] - 1, e = s_exec[p];
            o.bc_rank[b] = r;
            o.bc_exec[b] = e;
            o.bc_kind[b] = (uint8_t)(s_info[p] >> 3);
            o.bc_pm_in[b] = ((uint64_t)seg << 32) | ((uint64_t)e + 1);
            if (o.bc_key) o.bc_key[b] = ((uint64_t)seg << rbits) | e;
        }
        if ((code[i] >> 4) & 1u) run[7] = (uint32_t)p + 1;
        if (p == P - 1 && P % RD_W == 0) {
            // position P opens a chunk of its own: its running values and empty planes
            uint4 *ch = o.rdir + 4 * (P / RD_W);
            ch[0] = make_uint4(run[0], run[1], run[2], run[3]);
            ch[1] = make_uint4(run[4], run[5], run[6], run[7]);
            ch[2] = make_uint4(0u, 0u, 0u, 0u);
            ch[3] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

// bumped committed sorted by (segment, executeAt): exec column and nearest-Write index (+1) per entry
__global__ __launch_bounds__(BLOCK) void k_v2_bcs_cols(uint32_t nbc, const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ svals,
                                                       const uint8_t *__restrict__ bc_kind, uint64_t rmask,
                                                       uint32_t *__restrict__ bcs_exec, uint64_t *__restrict__ lastw_in)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nbc) return;
    bcs_exec[i] = (uint32_t)(skeys[i] & rmask);
    lastw_in[i] = bc_kind[svals[i]] == 1 ? i + 1 : 0;
}

// ---- the same order from the txn side (build_cfk, on the side lane beside the pair sort). Segments are the distinct
// compacted key codes in ascending order, so (segment, executeAt) order = (compacted key code, executeAt rank) order,
// and "bumped committed" is a per-txn property (ts.hpp): the list can be made from the batch's txn-major arrays before
// any pair is sorted. The bumped txns are taken in executeAt order (the dictionary has sorted them), each contributing
// its keys, so a stable sort by key code alone finishes the order: keys of (kc << (rbits + 1)) | execRank << 1 | isWrite
// sorted on the kc bits, the low bits riding along.

// cnt[k] = key count of the k-th bumped txn in executeAt order when it is bumped committed, else 0; bt[k] = that txn
__global__ __launch_bounds__(BLOCK) void k_bcx_counts(uint32_t nb, const uint32_t *__restrict__ sperm, const uint32_t *__restrict__ bsrc,
                                                      const uint8_t *__restrict__ status, const uint64_t *__restrict__ tl,
                                                      const uint32_t *__restrict__ key_off, uint32_t *__restrict__ bt,
                                                      uint32_t *__restrict__ cnt)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= nb) return;
    const uint32_t t = bsrc[sperm[k]];
    bt[k] = t;
    cnt[k] = bumped_committed(status[t], (uint32_t)(tl[t] >> 1) & 7u, true) ? key_off[t + 1] - key_off[t] : 0u;
}

// One block per BLOCK bumped txns: their output range [off[k0], off[k0 + cnt]) is walked coalesced, each entry finding its
// txn in the block's offsets in LDS (txns that contribute nothing share their offset with the next one). off[] is the
// exclusive scan of k_bcx_counts' counts (off[nb] = the total = the prep pass's count, the size of out).
__global__ __launch_bounds__(BLOCK) void k_bcx_expand(uint32_t nb, uint32_t n, const uint32_t *__restrict__ bt, const uint32_t *__restrict__ off,
                                                      const uint32_t *__restrict__ key_off, const uint64_t *__restrict__ key_code,
                                                      const uint32_t *__restrict__ rank, const uint64_t *__restrict__ tl, Runs rk,
                                                      int rbits, uint64_t nout, uint64_t *__restrict__ out)
{
    __shared__ uint32_t so[BLOCK + 1], st[BLOCK];
    const uint32_t tid = threadIdx.x, k0 = blockIdx.x * BLOCK;
    if (k0 >= nb) return;
    const uint32_t cnt = min((uint32_t)BLOCK, nb - k0);
    if (tid < cnt) { so[tid] = off[k0 + tid]; st[tid] = bt[k0 + tid]; }
    if (tid == 0) so[cnt] = off[k0 + cnt];
    __syncthreads();
    const uint64_t hi = min((uint64_t)so[cnt], nout);
    for (uint64_t j = (uint64_t)so[0] + tid; j < hi; j += BLOCK) {
        const uint32_t lo = seg_of(so, cnt, (uint32_t)j);   // last i with so[i] <= j (j < so[cnt])
        const uint32_t t = st[lo];
        const uint64_t kc = pext_runs(key_code[key_off[t] + (uint32_t)(j - so[lo])], rk);
        const uint64_t w = ((uint32_t)(tl[t] >> 1) & 7u) == 1u ? 1u : 0u;
        out[j] = (kc << (rbits + 1)) | ((uint64_t)rank[n + t] << 1) | w;
    }
}

// k_v2_bcs_cols for the keys above: the executeAt rank and the Write bit are in the sorted key itself
__global__ __launch_bounds__(BLOCK) void k_bcx_cols(uint32_t nbc, const uint64_t *__restrict__ skeys, uint64_t rmask,
                                                    uint32_t *__restrict__ bcs_exec, uint64_t *__restrict__ lastw_in)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nbc) return;
    const uint64_t x = skeys[i];
    bcs_exec[i] = (uint32_t)((x >> 1) & rmask);
    lastw_in[i] = (x & 1u) ? i + 1 : 0;
}

__device__ __forceinline__ uint32_t rd_cbc(const uint4 *rdir, uint32_t p);   // the rank directory, below

// The eight per-tile column scans of the multi-scan (7 counts: exclusive sums; the last-unbumped-committed-Write
// column: exclusive max) in ONE launch, one workgroup per column, carrying the running value across chunks.
constexpr int V2TS_ITEMS = 32;
__global__ __launch_bounds__(BLOCK) void k_v2_tile_scans(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t nt,
                                                         uint32_t *__restrict__ totals)
{
    __shared__ uint32_t red[WAVES];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const bool mx = q == 7;
    const uint32_t *a = in + (size_t)q * nt;
    uint32_t *o = out + (size_t)q * nt;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nt; base += BLOCK * V2TS_ITEMS) {
        uint32_t v[V2TS_ITEMS];
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < V2TS_ITEMS; ++i) {
            const uint32_t idx = base + tid * V2TS_ITEMS + i;
            v[i] = idx < nt ? a[idx] : 0u;
            acc = mx ? max(acc, v[i]) : acc + v[i];
        }
        uint32_t tot;
        const uint32_t pre = mx ? block_exclusive(acc, OpMax<uint32_t>(), red, tot) : block_exclusive(acc, OpAdd<uint32_t>(), red, tot);
        uint32_t run = mx ? max(carry, pre) : carry + pre;
#pragma unroll
        for (int i = 0; i < V2TS_ITEMS; ++i) {
            const uint32_t idx = base + tid * V2TS_ITEMS + i;
            if (idx < nt) o[idx] = run;
            run = mx ? max(run, v[i]) : run + v[i];
        }
        carry = mx ? max(carry, tot) : carry + tot;
    }
    if (tid == 0) totals[q] = carry;
}

struct V2View {
    const uint32_t *perm, *pair_pos, *seg_incl, *seg_start, *s_rank, *s_exec;
    const uint8_t *s_info;
    const uint4 *rdir;
    const uint32_t *list_rank, *bases;
    const uint32_t *bc_rank, *bc_exec;
    const uint64_t *bc_pm;    // (segment << 32 | executeAt + 1) prefix maxima: the low word within a segment
    const uint8_t *bc_kind;
    const uint32_t *bcs_exec;
    const uint64_t *bcs_lastw;   // nearest Write index + 1 (prefix maximum, the low word)
    const uint4 *tinfo;   // per txn: rank, executeAt rank, status | kind << 3
    const uint32_t *irec32;  // the count pass's inline records as u32 (IREC_W words per pair; word 7 = E | flag)
    const uint4 *rec;        // the count pass's 64-B records (runs; inline entries beyond IREC_N)
};

struct Row { uint32_t c[8]; };

// the 8 running values at CFK position p from its rank-directory chunk
__device__ __forceinline__ Row ld_row(const V2View &v, uint32_t p)
{
    const uint4 *ch = v.rdir + 4 * (size_t)(p / RD_W);
    const uint4 a = ch[0], b = ch[1], c = ch[2], d = ch[3];
    const uint32_t r = p % RD_W, mask = (1u << r) - 1u;
    Row o;
    o.c[0] = a.x + __popc(c.x & mask); o.c[1] = a.y + __popc(c.y & mask);
    o.c[2] = a.z + __popc(c.z & mask); o.c[3] = a.w + __popc(c.w & mask);
    o.c[4] = b.x + __popc(d.x & mask); o.c[5] = b.y + __popc(d.y & mask);
    o.c[6] = b.z + __popc(d.z & mask);
    const uint32_t w = d.w & mask;
    o.c[7] = w ? (p - r) + (31u - (uint32_t)__clz(w)) + 1u : b.w;
    return o;
}
// the bumped-committed count below position p (column RW_CBC only)
__device__ __forceinline__ uint32_t rd_cbc(const uint4 *rdir, uint32_t p)
{
    const uint32_t *ch = reinterpret_cast<const uint32_t *>(rdir) + 16 * (size_t)(p / RD_W);
    const uint32_t r = p % RD_W;
    return ch[RW_CBC] + __popc(ch[8 + RW_CBC] & ((1u << r) - 1u));
}
__device__ __forceinline__ uint32_t ld_cbc(const V2View &v, uint32_t p) { return rd_cbc(v.rdir, p); }

struct V2Query {
    uint32_t trank, info, wk, wc, s0, pos, posm, m, bstart, bend;
    bool bq, has_m;
    Row r0, rp, rm;   // rows at s0, pos, posM
};

// The query of the pair at CFK position p (pair order (key, TxnId)): every per-txn input comes from the
// position-ordered columns, so neighbouring lanes read neighbouring rows. The loads are ordered for a short dependency
// chain: the pair's own row and columns; then its segment's bounds; then, together, the segment start's row, the
// bumped-committed count at the segment end, and -- speculatively, assuming M is the last unbumped committed Write
// before the pair (it is unless the segment holds bumped committed entries or the query's executeAt is bumped, ~1.5% of
// pairs, recomputed below) -- that Write's TxnId and its row.
__device__ __forceinline__ V2Query v2_query(const V2View &v, uint32_t p)
{
    V2Query q;
    const Row rpp = ld_row(v, p);
    const uint32_t seg = v.seg_incl[p] - 1;
    q.trank = v.s_rank[p];
    const uint32_t S = v.s_exec[p];
    q.info = v.s_info[p];
    q.s0 = v.seg_start[seg];
    const uint32_t s1 = v.seg_start[seg + 1];
    q.wk = witnesses(q.info >> 3);
    q.wc = wk_classes(q.wk);
    q.bq = S != q.trank;
    // level 3: issued together
    const uint32_t lu0 = rpp.c[RW_LUCW];
    const bool spec = !q.bq && lu0 > q.s0;   // the last unbumped committed Write before p lies in p's segment
    q.r0 = ld_row(v, q.s0);
    const uint32_t b1 = ld_cbc(v, s1);
    uint32_t mu = 0;
    Row rms = q.r0;
    if (spec) { mu = v.s_rank[lu0 - 1]; rms = ld_row(v, lu0 - 1); }
    const uint32_t b0 = q.r0.c[RW_CBC];
    if (!q.bq && b1 == b0) {
        // common path: no bumped committed entry in the segment, executeAt == TxnId
        q.pos = p;
        q.rp = rpp;
        q.has_m = spec;
        q.m = mu;
        q.posm = spec ? lu0 - 1 : q.s0;
        q.rm = rms;
        q.bend = q.rm.c[RW_CBC];
        q.bstart = q.bend;   // no bumped committed entry before posM in this segment (b1 == b0)
        return q;
    }
    q.pos = q.bq ? lower_bound(v.s_rank, p + 1, s1, S) : p;
    q.rp = q.bq ? ld_row(v, q.pos) : rpp;
    // M from the last unbumped committed Write before pos
    const uint32_t lu = q.rp.c[RW_LUCW];
    const bool has_mu = lu > q.s0;
    if (q.bq) mu = has_mu ? v.s_rank[lu - 1] : 0;
    // M from bumped committed Writes of this segment: predecessor of S by executeAt, then nearest Write
    bool has_mb = false;
    uint32_t mb = 0;
    if (b1 > b0) {
        uint32_t i = lower_bound(v.bcs_exec, b0, b1, S);
        if (i > b0) {
            uint32_t w = (uint32_t)v.bcs_lastw[i - 1];
            if (w > b0) { has_mb = true; mb = v.bcs_exec[w - 1]; }
        }
    }
    q.has_m = has_mu || has_mb;
    q.m = (has_mb && (!has_mu || mb > mu)) ? mb : mu;
    if (!q.has_m) q.posm = q.s0;
    else if (has_mu && q.m == mu) q.posm = lu - 1;
    else q.posm = lower_bound(v.s_rank, q.s0, q.pos, q.m);
    q.rm = q.posm == q.s0 ? q.r0 : (spec && q.posm == lu0 - 1) ? rms : ld_row(v, q.posm);
    q.bend = q.rm.c[RW_CBC];
    // first bumped committed entry whose prefix max (the low words, ascending over one segment) reaches M + 1
    q.bstart = q.has_m ? partition_point(b0, q.bend, [&](uint32_t i) { return (uint32_t)v.bc_pm[i] < q.m + 1; }) : q.bend;
    return q;
}

// per-pair results for the write pass, stored by pair index j (the write pass reads a txn's pairs contiguously):
//   irec[j] (32 B, every pair): word 7 = E, | REC_INLINE_FLAG for an inline record (the mark pass reads this word;
//           a separate 4-B E word per pair measured slower: the count pass's extra scattered store costs more than
//           the mark pass saves, config 3 +1.2 ms vs -0.1 ms);
//           inline (E <= REC_INLINE): the pair's dependency entries themselves (TxnId ranks, T and filtered R3 entries
//           already dropped), the first IREC_N in words 0-6, the rest (E > IREC_N) in words 0-7 of rec[j]. Gathered
//           here in CFK position order, where neighbouring pairs of a segment read the same class-list lines, instead
//           of by the write pass in txn order;
//   rec[j]  (64 B, run pairs, E > REC_INLINE): starts a[6] and lengths l[6] of R1/R2 per class (witnessed classes only),
//           R3 = [bs, bs + bl) filtered by executeAt >= M; word 15 = E.
// An inline entry is addressed as 16 * j + off (inl_entry).
constexpr uint32_t NO_M = 0xFFFFFFFFu;
constexpr uint32_t INLINE_M = 0xFFFFFFFEu;   // RunsT::m marker of an inline record
constexpr uint32_t REC_INLINE = 15;
constexpr uint32_t IREC_W = 8;               // u32 words per 32-B record
constexpr uint32_t IREC_N = 7;               // inline entries held by the 32-B record
constexpr uint32_t REC_INLINE_FLAG = 0x80000000u;

// inline entry off of pair j (idx = 16 * j + off)
__device__ __forceinline__ uint32_t inl_entry(const uint32_t *irec32, const uint4 *rec, uint32_t idx)
{
    const uint32_t j = idx >> 4, off = idx & 15u;
    return off < IREC_N ? irec32[IREC_W * (size_t)j + off] : reinterpret_cast<const uint32_t *>(rec)[16 * (size_t)j + off - IREC_N];
}

__device__ __forceinline__ void inl_put(uint32_t (&buf)[16], uint32_t &n, uint32_t x)
{
#pragma unroll
    for (uint32_t s = 0; s < REC_INLINE; ++s) if (s == n) buf[s] = x;   // static register indices (no scratch)
    ++n;
}

struct RecOut {
    uint4 *rec;         // run records, 4 x uint4 per pair
    uint4 *irec;        // inline records / E words, 2 x uint4 per pair
};

#ifdef ACC_PHASE_PROF
// tuning build only: per wave of k_v2_count, cycles of (query, R3 count, inline gather + record write) and lane counts
// (bumped query, segment with bumped committed entries, posM by search, sum of R3 candidates, run records)
__device__ unsigned long long *g_ct_prof;
#define CT_PH(i) ct_ph[i] = clock64()
#else
#define CT_PH(i) ((void)0)
#endif

#ifndef ACC_R3U
#define ACC_R3U 4   // R3 candidates loaded per round of the count pass's per-lane loops
#endif
#ifndef ACC_R3_COOP
#define ACC_R3_COOP 8   // a wave walks the R3 candidates cooperatively when one of its lanes has more
#endif
__device__ __forceinline__ uint64_t v2_count_one(const V2View &v, uint32_t p, const uint32_t *__restrict__ owner,
                                                  const RecOut &ro, uint32_t *__restrict__ bigflag)
{
#ifdef ACC_PHASE_PROF
    unsigned long long ct_ph[4];
#endif
    CT_PH(0);
    const uint32_t j = v.perm[p];   // independent of the query chain: issued first
    V2Query q = v2_query(v, p);
    CT_PH(1);
    uint32_t a[6] = {}, l[6] = {};
    uint64_t e = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (!((q.wc >> c) & 1u)) continue;
        a[2 * c] = v.bases[c] + q.r0.c[c];
        l[2 * c] = q.rp.c[c] - q.r0.c[c];
        a[2 * c + 1] = v.bases[3 + c] + q.rm.c[3 + c];
        l[2 * c + 1] = q.rp.c[3 + c] - q.rm.c[3 + c];
        e += l[2 * c] + l[2 * c + 1];
    }
    // the class runs' entries of a record that may be inline (L6 <= 16: e <= 15 needs it) are loaded before the R3
    // candidates are counted, so both sets of loads are in flight together (static slots, predicated)
    uint32_t pre[6], L6 = 0;
#pragma unroll
    for (int q2 = 0; q2 < 6; ++q2) { pre[q2] = L6; L6 += l[q2]; }
    uint32_t xs[REC_INLINE + 1];
    const bool may_inline = L6 <= REC_INLINE + 1;
#pragma unroll
    for (uint32_t s = 0; s <= REC_INLINE; ++s) {
        uint32_t idx = a[0] + s;
#pragma unroll
        for (int q2 = 1; q2 < 6; ++q2)
            if (s >= pre[q2]) idx = a[q2] + (s - pre[q2]);   // empty runs are overridden by the next one
        xs[s] = (may_inline && s < L6) ? v.list_rank[idx] : 0u;
    }
    // R3 candidates [bstart, bend): one lane walks its own (ACC_R3U loads in flight), or, when some lane of the wave has
    // more than ACC_R3_COOP (the lanes of a hot segment share nearly the same range), the wave loads the union of the
    // ranges 64 candidates at a time (coalesced) and every lane tests each candidate broadcast from its lane
    // (v_readlane): one memory round trip per 64 candidates instead of one per ACC_R3U
    const uint32_t nc = q.bend > q.bstart ? q.bend - q.bstart : 0u;
    uint32_t wmax = nc, clo = nc ? q.bstart : 0xFFFFFFFFu, chi = nc ? q.bend : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        wmax = max(wmax, (uint32_t)__shfl_xor((int)wmax, d, 64));
        clo = min(clo, (uint32_t)__shfl_xor((int)clo, d, 64));
        chi = max(chi, (uint32_t)__shfl_xor((int)chi, d, 64));
    }
    const bool coop = wmax > (uint32_t)ACC_R3_COOP && chi - clo <= 64u * 64u;   // wave-uniform
    if (coop) {
        for (uint32_t c = clo; c < chi; c += 64) {
            const uint32_t i = c + lane_id();
            const uint32_t exl = i < chi ? v.bc_exec[i] : 0u, kdl = i < chi ? (uint32_t)v.bc_kind[i] : 0u;
            const uint32_t cnt = min(64u, chi - c);
            for (uint32_t u = 0; u < cnt; ++u) {
                const uint32_t exu = (uint32_t)__builtin_amdgcn_readlane((int)exl, (int)u);
                const uint32_t kdu = (uint32_t)__builtin_amdgcn_readlane((int)kdl, (int)u);
                const uint32_t iu = c + u;
                e += (iu >= q.bstart && iu < q.bend && exu >= q.m && ((q.wk >> kdu) & 1u)) ? 1u : 0u;
            }
        }
    } else {
        for (uint32_t i = q.bstart; i < q.bend; i += ACC_R3U) {
            uint32_t ex[ACC_R3U], kd[ACC_R3U];
#pragma unroll
            for (uint32_t u = 0; u < ACC_R3U; ++u) {
                ex[u] = i + u < q.bend ? v.bc_exec[i + u] : 0u;
                kd[u] = i + u < q.bend ? (uint32_t)v.bc_kind[i + u] : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < ACC_R3U; ++u) e += (i + u < q.bend && ex[u] >= q.m && ((q.wk >> kd[u]) & 1u)) ? 1u : 0u;
        }
    }
    if (q.bq) {
        uint32_t st = q.info & 7u, kind = q.info >> 3;
        if (((q.wk >> kind) & 1u) && st != 0 && st != 7) --e;
    }
    CT_PH(2);
    const bool inl = e <= REC_INLINE;
    // an inline record: the class entries without T (L6 <= e + 1 <= 16: T itself is dropped at most once, so xs holds
    // every class entry), then the kept R3 entries
    uint32_t d = L6;   // position of T among them (at most one)
#pragma unroll
    for (uint32_t s = 0; s <= REC_INLINE; ++s)
        if (q.bq && s < L6 && xs[s] == q.trank) d = s;
    uint32_t buf[16] = {};
#pragma unroll
    for (uint32_t s = 0; s < REC_INLINE; ++s) buf[s] = s < d ? xs[s] : xs[s + 1];
    uint32_t n = L6 - (d < L6 ? 1u : 0u);
    if (coop) {
        const bool want = inl && q.has_m && nc;
        if (__ballot(want))
            for (uint32_t c = clo; c < chi; c += 64) {
                const uint32_t i = c + lane_id();
                const uint32_t exl = i < chi ? v.bc_exec[i] : 0u, kdl = i < chi ? (uint32_t)v.bc_kind[i] : 0u;
                const uint32_t xrl = i < chi ? v.bc_rank[i] : 0u;
                const uint32_t cnt = min(64u, chi - c);
                for (uint32_t u = 0; u < cnt; ++u) {
                    const uint32_t exu = (uint32_t)__builtin_amdgcn_readlane((int)exl, (int)u);
                    const uint32_t kdu = (uint32_t)__builtin_amdgcn_readlane((int)kdl, (int)u);
                    const uint32_t xru = (uint32_t)__builtin_amdgcn_readlane((int)xrl, (int)u);
                    const uint32_t iu = c + u;
                    if (want && iu >= q.bstart && iu < q.bend && exu >= q.m && ((q.wk >> kdu) & 1u) &&
                        !(q.bq && xru == q.trank))
                        inl_put(buf, n, xru);
                }
            }
    } else if (inl && q.has_m) {
        for (uint32_t i = q.bstart; i < q.bend; i += ACC_R3U) {   // R3 candidates, ACC_R3U at a time
            uint32_t ex[ACC_R3U], kd[ACC_R3U], xr[ACC_R3U];
#pragma unroll
            for (uint32_t u = 0; u < ACC_R3U; ++u) {
                const bool in = i + u < q.bend;
                ex[u] = in ? v.bc_exec[i + u] : 0u;
                kd[u] = in ? (uint32_t)v.bc_kind[i + u] : 0u;
                xr[u] = in ? v.bc_rank[i + u] : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < ACC_R3U; ++u)
                if (i + u < q.bend && ex[u] >= q.m && ((q.wk >> kd[u]) & 1u) && !(q.bq && xr[u] == q.trank))
                    inl_put(buf, n, xr[u]);
        }
    }
    if (inl) {
        uint4 *r = ro.irec + 2 * (size_t)j;
        r[0] = make_uint4(buf[0], buf[1], buf[2], buf[3]);
        r[1] = make_uint4(buf[4], buf[5], buf[6], REC_INLINE_FLAG | (uint32_t)e);
        if (e > IREC_N) {
            uint4 *r2 = ro.rec + 4 * (size_t)j;
            r2[0] = make_uint4(buf[7], buf[8], buf[9], buf[10]);
            r2[1] = make_uint4(buf[11], buf[12], buf[13], buf[14]);
        }
    } else {
        uint4 *ir = ro.irec + 2 * (size_t)j;
        ir[0] = make_uint4(0u, 0u, 0u, 0u);
        ir[1] = make_uint4(0u, 0u, 0u, (uint32_t)e);
        uint4 *r = ro.rec + 4 * (size_t)j;
        r[0] = make_uint4(a[0], a[1], a[2], a[3]);
        r[1] = make_uint4(a[4], a[5], l[0], l[1]);
        r[2] = make_uint4(l[2], l[3], l[4], l[5]);
        r[3] = make_uint4(q.bstart, q.has_m ? q.bend - q.bstart : 0u, q.has_m ? q.m : NO_M, (uint32_t)e);
        bigflag[owner[j]] = 1u;
    }
#ifdef ACC_PHASE_PROF
    CT_PH(3);
    {
        const uint32_t s1 = v.seg_start[v.seg_incl[p]];
        const bool mb = ld_cbc(v, s1) > q.r0.c[RW_CBC];
        const bool psearch = q.has_m && q.posm != q.s0 && !(q.rp.c[RW_LUCW] > q.s0 && q.m == v.s_rank[q.rp.c[RW_LUCW] - 1]);
        uint32_t r3 = q.bend - q.bstart;
        for (int d = 1; d < 64; d <<= 1) r3 += __shfl_xor(r3, d, 64);
        if (lane_id() == 0) {
            unsigned long long *row = g_ct_prof + 8 * (size_t)((blockIdx.x * BLOCK + threadIdx.x) >> 6);
            row[0] = ct_ph[1] - ct_ph[0]; row[1] = ct_ph[2] - ct_ph[1]; row[2] = ct_ph[3] - ct_ph[2];
            row[3] = (unsigned long long)__popcll(__ballot(q.bq));
            row[4] = (unsigned long long)__popcll(__ballot(mb));
            row[5] = (unsigned long long)__popcll(__ballot(psearch));
            row[6] = r3;
            row[7] = (unsigned long long)__popcll(__ballot(e > REC_INLINE)) | (1ull << 32);
        }
    }
#endif
    return e;
}

// Also: bigflag[T] = 1 for txns with a run record (they take the v2 tiers, the rest the stream pass) and per-block
// entry totals (blk_e) for the batch's E.
__global__ __launch_bounds__(BLOCK) void k_v2_count(size_t P, V2View v, const uint32_t *__restrict__ owner,
                                                    RecOut ro, uint32_t *__restrict__ bigflag,
                                                    uint64_t *__restrict__ blk_e)
{
    __shared__ uint64_t lds[WAVES];
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    uint64_t e = 0;
    if (p < P) e = v2_count_one(v, (uint32_t)p, owner, ro, bigflag);
    uint64_t total;
    block_exclusive(e, OpAdd<uint64_t>(), lds, total);
    if (threadIdx.x == 0) blk_e[blockIdx.x] = total;
}

// ---- write pass, three tiers by E_T (dependency entries of the txn; 98.7% of config-2 txns have <= 64):
//   small  (E <= 64,  <= 32 keys): one wave per txn, registers + 512 B of LDS staging, high occupancy
//   medium (E <= 1024, <= 64 keys): one wave per txn, bitonic sort of (value << 16 | key) in LDS
//   big    (E <= 8192, <= 64 keys): one block per txn, bitonic sort in 64 KiB of LDS
//   fallback (otherwise, rare):      global gather + two radix sorts
// Every tier: lane k derives the 7 runs of key k (R1/R2 per kind class, R3) from the count-pass record,
// the runs are gathered flattened by all lanes, T itself and non-qualifying R3 entries are dropped.

constexpr int NRUN = 7;
constexpr int MED_E = 1024, MED_K = 64;
constexpr int BIG_K = 64;
constexpr int BIG_E = 8192;                 // raw entries per block in LDS (32 KiB of u32 records)
constexpr int HUGE_E = 16384;               // second big launch (64 KiB + a 64 KiB merge buffer)

struct V2Out {
    const uint32_t *key_off;
    const uint64_t *dep_off, *arena_off;
    const uint32_t *cnz, *txn_of_rank;
    const uint4 *rec;        // run records, 4 x uint4 per pair (k_v2_count)
    const uint32_t *irec32;  // inline records, IREC_W words per pair (word 7 = E | REC_INLINE_FLAG)
    int32_t *arena;
    uint32_t *dep_scratch;   // at dep_off[j0] + idx, compacted later
    uint64_t *u_cnt;
    uint32_t *med_list, *big_list, *fb_list, *huge_list;
    uint64_t *gstat;         // [0] medium, [1] big, [2] count mismatches, [3] fallback txns, [4] fallback entries,
                             // [5] small, [6] huge (second big launch), [7] / [8] window tier (<= 8 / <= 16 keys)
};
constexpr int GSTAT_N = 12;

template <int MAXK>
struct RunsT {
    uint32_t start[MAXK][NRUN];
    uint32_t pre[MAXK][NRUN + 1];
    uint32_t kbase[MAXK + 1];
    uint32_t m[MAXK];
    uint32_t kc[MAXK];
    uint32_t total;
};

struct TxnCtx {
    uint32_t t, j0, j1, nk, E, trank, wk, wc;
    uint64_t e0;
    bool bq;
};

__device__ __forceinline__ TxnCtx txn_ctx(const V2View &v, const V2Out &o, uint32_t t)
{
    TxnCtx c;
    c.t = t;
    c.j0 = o.key_off[t]; c.j1 = o.key_off[t + 1]; c.nk = c.j1 - c.j0;
    c.e0 = o.dep_off[c.j0];
    c.E = (uint32_t)(o.dep_off[c.j1] - c.e0);
    uint4 ti = v.tinfo[t];
    c.trank = ti.x;
    c.bq = ti.y != c.trank;
    c.wk = witnesses(ti.z >> 3);
    c.wc = wk_classes(c.wk);
    return c;
}

// Key k's runs from its record (pair index jk); an inline record is one run of its own entries (m = INLINE_M,
// start = the pair index). Returns the key's raw length.
// A pair's count-pass record as loaded: its entry count, the inline record's word 7 and the four run-record words. The
// loads are independent and issued together (one memory round trip, not three in a chain); an inline record's run words
// are loaded and ignored.
struct RecRaw {
    uint64_t cnt;
    uint32_t w;
    uint4 r0, r1, r2, r3;
};

__device__ __forceinline__ RecRaw load_rec_raw(const uint4 *rec, const uint32_t *irec32, const uint64_t *cnt, uint32_t jk)
{
    RecRaw a;
    a.cnt = cnt[jk];
    a.w = irec32[IREC_W * (size_t)jk + 7];
    const uint4 *r = rec + 4 * (size_t)jk;
    a.r0 = r[0]; a.r1 = r[1]; a.r2 = r[2]; a.r3 = r[3];
    return a;
}

template <int MAXK>
__device__ __forceinline__ uint32_t load_record(RunsT<MAXK> &R, const RecRaw &a, uint32_t jk, uint32_t k)
{
    const uint32_t w = a.w;
    if (w & REC_INLINE_FLAG) {
        const uint32_t e = w & ~REC_INLINE_FLAG;
        R.start[k][0] = jk;
        R.pre[k][0] = 0;
#pragma unroll
        for (int q = 1; q <= NRUN; ++q) R.pre[k][q] = e;
        R.m[k] = INLINE_M;
        return e;
    }
    const uint4 r0 = a.r0, r1 = a.r1, r2 = a.r2, r3 = a.r3;
    const uint32_t s[6] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y };
    const uint32_t l[6] = { r1.z, r1.w, r2.x, r2.y, r2.z, r2.w };
    uint32_t acc = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) { R.start[k][q] = s[q]; R.pre[k][q] = acc; acc += l[q]; }
    R.start[k][6] = r3.x; R.pre[k][6] = acc; acc += r3.y;
    R.pre[k][7] = acc;
    R.m[k] = r3.z;
    return acc;
}

// Called by ONE wave: lane k < nk fills the runs of key k (pair j0 + k) from its loaded record. Returns the flattened
// raw length.
template <int MAXK>
__device__ uint32_t finish_runs(RunsT<MAXK> &R, const RecRaw &a, uint32_t j0, uint32_t nk)
{
    const uint32_t lane = lane_id();
    uint32_t ktot = 0;
    if (lane < nk && a.cnt != 0) {
        ktot = load_record(R, a, j0 + lane, lane);
    } else if (lane < nk) {
        for (int q = 0; q <= NRUN; ++q) R.pre[lane][q] = 0;
        R.m[lane] = NO_M;
    }
    if (lane < (uint32_t)MAXK) R.kc[lane] = 0;
    uint32_t incl = wave_inclusive(ktot, OpAdd<uint32_t>());
    if (lane < nk) R.kbase[lane] = incl - ktot;
    uint32_t total = shfl_idx(incl, 63);
    if (lane == 0) { R.kbase[nk] = total; R.total = total; }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    return total;
}

// Called by ONE wave: lane k < nk loads the 64-B record of key k and fills its runs.
template <int MAXK>
__device__ uint32_t compute_runs(RunsT<MAXK> &R, const V2View &v, const V2Out &o, const uint64_t *cnt, const TxnCtx &c)
{
    RecRaw a{};
    if (lane_id() < c.nk) a = load_rec_raw(o.rec, o.irec32, cnt, c.j0 + lane_id());
    return finish_runs(R, a, c.j0, c.nk);
}

// Element e of the flattened runs: value x, key k; returns whether it is an entry of the txn's deps.
template <int MAXK>
__device__ __forceinline__ bool fetch_elem(const RunsT<MAXK> &R, const V2View &v, const TxnCtx &c, uint32_t e,
                                           uint32_t &x, uint32_t &k)
{
    k = seg_of(R.kbase, c.nk, e);
    uint32_t off = e - R.kbase[k];
    if (R.m[k] == INLINE_M) {   // inline record: the entry itself (filters applied by the count pass)
        x = inl_entry(v.irec32, v.rec, 16 * R.start[k][0] + off);
        return true;
    }
    uint32_t r = 0;
    while (r + 1 < NRUN && R.pre[k][r + 1] <= off) ++r;
    uint32_t idx = R.start[k][r] + (off - R.pre[k][r]);
    bool keep;
    if (r < 6) {
        x = v.list_rank[idx];
        keep = true;
    } else {
        x = v.bc_rank[idx];
        keep = v.bc_exec[idx] >= R.m[k] && ((c.wk >> v.bc_kind[idx]) & 1u);
    }
    return keep && !(c.bq && x == c.trank);
}

// Gather the flattened runs into buf (compacted, at most cap entries). Returns the kept count.
template <int MAXK>
__device__ uint32_t gather_to(uint64_t *buf, uint32_t cap, const RunsT<MAXK> &R, const V2View &v, const TxnCtx &c,
                              uint32_t total)
{
    const uint32_t lane = lane_id();
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    uint32_t cursor = 0;
    for (uint32_t c0 = 0; c0 < total; c0 += 64) {
        uint32_t e = c0 + lane;
        bool keep = false;
        uint32_t x = 0, k = 0;
        if (e < total) keep = fetch_elem(R, v, c, e, x, k);
        uint64_t bal = __ballot(keep);
        if (keep) {
            uint32_t slot = cursor + (uint32_t)__popcll(bal & lt);
            if (slot < cap) buf[slot] = ((uint64_t)x << 16) | k;
        }
        cursor += (uint32_t)__popcll(bal);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    return cursor;
}

// register bitonic across the 64 lanes (ascending by lane)
__device__ __forceinline__ uint64_t wave_bitonic_reg(uint64_t x)
{
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            uint64_t y = shfl_xor64(x, (int)jj);
            bool up = (lane & k) == 0, lower = (lane & jj) == 0;
            uint64_t lo = x < y ? x : y, hi = x < y ? y : x;
            x = (lower == up) ? lo : hi;
        }
    }
    return x;
}

// Emit one chunk of up to 64 sorted entries (lane holds x). Returns the updated distinct count.
// TRANSLATE = false: the TxnId rank is written and the caller maps the txn's ranks to TxnIds in one bulk pass (a
// dependent global load per chunk would otherwise serialise the chunks)
template <bool TRANSLATE = true>
__device__ __forceinline__ uint32_t emit_chunk(uint64_t x, bool in, uint64_t prev, bool has_prev, uint32_t distinct,
                                               uint32_t *kc, const V2Out &o, const TxnCtx &c, uint64_t abase)
{
    const uint32_t lane = lane_id();
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    uint32_t val = (uint32_t)(x >> 16), kj = (uint32_t)(x & 0xFFFFu);
    bool nw = in && (!has_prev || (uint32_t)(prev >> 16) != val);
    uint64_t bal = __ballot(nw);
    uint32_t idx = distinct + (uint32_t)__popcll(bal & lt) + (nw ? 1u : 0u) - 1u;
    uint64_t peers = __ballot(in);
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        uint64_t bb = __ballot((kj >> b) & 1u);
        peers &= ((kj >> b) & 1u) ? bb : ~bb;
    }
    uint32_t before = (uint32_t)__popcll(peers & lt);
    if (in) {
        uint32_t slot = kc[kj] + before;
        uint64_t kbase = o.dep_off[c.j0 + kj] - c.e0;
        o.arena[abase + kbase + slot] = (int32_t)idx;
        if (nw) o.dep_scratch[c.e0 + idx] = TRANSLATE ? o.txn_of_rank[val] : val;
    }
    __builtin_amdgcn_wave_barrier();
    if (in && before == 0) kc[kj] += (uint32_t)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    return distinct + (uint32_t)__popcll(bal);
}

// Persistent over the routed list (count on the device: the v3 routing runs after the last host sync).
__global__ __launch_bounds__(BLOCK) void k_v2_write_medium(const uint64_t *__restrict__ cnt_dev, const uint32_t *__restrict__ list,
                                                           V2View v, const uint64_t *__restrict__ cnt, V2Out o)
{
    __shared__ uint64_t sbuf[WAVES][MED_E];
    __shared__ RunsT<MED_K> sruns[WAVES];
    const uint32_t wave = threadIdx.x >> 6, lane = lane_id();
    const uint32_t cnt_list = (uint32_t)*cnt_dev;
    RunsT<MED_K> &R = sruns[wave];
    uint64_t *buf = sbuf[wave];
    for (uint32_t i = blockIdx.x * WAVES + wave; i < cnt_list; i += gridDim.x * WAVES) {
        const uint32_t t = list[i];
        TxnCtx c = txn_ctx(v, o, t);
        uint32_t total = compute_runs(R, v, o, cnt, c);
        uint32_t got = gather_to(buf, MED_E, R, v, c, total);
        if (got != c.E) { if (lane == 0) atomicAdd((unsigned long long *)&o.gstat[2], 1ull); continue; }
        const uint64_t abase = o.arena_off[t] + (o.cnz[c.j1] - o.cnz[c.j0]);
        uint32_t n2 = 128;
        while (n2 < c.E) n2 <<= 1;
        for (uint32_t q = c.E + lane; q < n2; q += 64) buf[q] = ~0ull;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        wave_bitonic_lds(buf, n2);
        uint32_t distinct = 0;
        for (uint32_t q0 = 0; q0 < c.E; q0 += 64) {
            uint32_t q = q0 + lane;
            bool in = q < c.E;
            uint64_t x = in ? buf[q] : 0;
            uint64_t prev = q > 0 ? buf[q - 1] : 0;
            distinct = emit_chunk(x, in, prev, q > 0, distinct, R.kc, o, c, abase);
        }
        if (lane == 0) o.u_cnt[t] = distinct;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
}

// Locate element e of the flattened runs (LDS only): source index, key, R3 flag.
template <int MAXK>
__device__ __forceinline__ void locate_elem(const RunsT<MAXK> &R, uint32_t nk, uint32_t e, uint32_t &idx, uint32_t &k, bool &r3,
                                            bool &inl)
{
    k = seg_of(R.kbase, nk, e);
    uint32_t off = e - R.kbase[k];
    inl = R.m[k] == INLINE_M;
    if (inl) { idx = 16 * R.start[k][0] + off; r3 = false; return; }
    uint32_t r = 0;
    while (r + 1 < NRUN && R.pre[k][r + 1] <= off) ++r;
    idx = R.start[k][r] + (off - R.pre[k][r]);
    r3 = r == 6;
}

// Big tier: one block per txn (raw run length <= BIG_E). All four waves gather (dropped entries become
// all-ones sentinels that sort last), the block bitonic-sorts (value << 16 | key), then each wave emits a
// quarter of the sorted entries with per-key / distinct-value bases from a per-wave count pass.
constexpr int BIG_GU = 4;   // independent loads in flight per thread during the gather

// Sort records are u32 (TxnId rank << 6 | key index): half the LDS of u64 records, twice the blocks per CU. The
// host takes these tiers only when ranks fit 25 bits (2N <= 2^25). CAP = raw run elements per block: MED_CAP (routed
// by k_v3_route), BIG_E (the txns beyond MED_CAP, routed or passed on by the first launch via gstat[1]), HUGE_E
// (txns the BIG_E launch passes on via gstat[6] / huge_list); beyond that the global path.
// MED_CAP / BIG_E sort by merging: a key's entries are at most NRUN runs that are each sorted by TxnId rank (CFK
// position order within a class list; inline records are sorted by one thread), so after compacting the kept
// entries a merge tree over the non-empty runs (log2 of the run count levels, merge-path partitions per thread)
// sorts them in a few LDS passes instead of the O(n log^2 n) of a bitonic network. HUGE_E keeps the bitonic sort
// in place (no room for a second buffer).
constexpr int MED_CAP = 1024;
constexpr int RUN_SLOTS = NRUN * BIG_K;

template <int CAP>
constexpr bool big_merges() { return CAP <= HUGE_E; }

template <int CAP, int NT>
struct BigLds {
    uint32_t buf[CAP];
    uint32_t tmp[big_merges<CAP>() ? CAP : 1];
    uint32_t rs[big_merges<CAP>() ? RUN_SLOTS + 1 : 1];
    uint32_t ss[big_merges<CAP>() ? RUN_SLOTS : 1];   // compacted start of each (key, run) slot
    RunsT<BIG_K> R;
    uint32_t s_kept, s_nr;
    uint32_t wk_cnt[NT / 64][BIG_K];
    uint32_t wdist[NT / 64];
};

// Sorts the kept entries of buf[0, total) (dropped = all-ones) into ascending order; returns the array holding the
// E sorted entries (buf or tmp). Block-wide; R = the txn's runs (raw layout: key-major, runs in slot order).
template <int CAP, int NT>
__device__ uint32_t *big_merge_sort(BigLds<CAP, NT> &L, uint32_t nk, uint32_t total, uint32_t E)
{
    uint32_t *buf = L.buf, *tmp = L.tmp, *rs = L.rs;
    const RunsT<BIG_K> &R = L.R;
    const uint32_t tid = threadIdx.x;
    __shared__ uint32_t lds[NT / 64];
    // ---- compaction (order kept): tmp[kept index] = entry; buf[raw e] = kept entries before e
    const uint32_t CHR = (total + NT - 1) / NT;
    const uint32_t r0 = min(total, tid * CHR), r1 = min(total, r0 + CHR);
    uint32_t cnt = 0;
    for (uint32_t e = r0; e < r1; ++e) cnt += buf[e] != 0xFFFFFFFFu;
    uint32_t tot;
    uint32_t pos = block_exclusive<uint32_t, OpAdd<uint32_t>, NT / 64>(cnt, OpAdd<uint32_t>(), lds, tot);
    for (uint32_t e = r0; e < r1; ++e) {
        const uint32_t x = buf[e];
        buf[e] = pos;
        if (x != 0xFFFFFFFFu) tmp[pos++] = x;
    }
    __syncthreads();
    // ---- run slots (key k, run q) -> compacted starts; inline keys (one unsorted slot of <= REC_INLINE) sorted here
    for (uint32_t k = tid; k < nk; k += NT) {
        const uint32_t kb = R.kbase[k];
        uint32_t st[NRUN + 1];
#pragma unroll
        for (int q = 0; q <= NRUN; ++q) {
            const uint32_t raw = kb + R.pre[k][q];
            st[q] = raw >= total ? E : buf[raw];
        }
        if (R.m[k] == INLINE_M) {
            for (uint32_t i = st[0] + 1; i < st[NRUN]; ++i) {   // insertion sort
                const uint32_t x = tmp[i];
                uint32_t j = i;
                while (j > st[0] && tmp[j - 1] > x) { tmp[j] = tmp[j - 1]; --j; }
                tmp[j] = x;
            }
        }
        // slot starts; a slot's end is the next slot's start (raw layout is key-major, slot-ordered)
#pragma unroll
        for (int q = 0; q < NRUN; ++q) L.ss[k * NRUN + q] = st[q];
    }
    __syncthreads();
    // ---- non-empty runs -> rs[0, NR), rs[NR] = E (one wave; slots in order)
    if (tid < 64) {
        const uint32_t lane = lane_id();
        const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        const uint32_t ns = nk * NRUN;
        uint32_t nr = 0;
        for (uint32_t s0 = 0; s0 < ns; s0 += 64) {
            const uint32_t sl = s0 + lane;
            uint32_t a = 0, b = 0;
            if (sl < ns) {
                a = L.ss[sl];
                b = sl + 1 < ns ? L.ss[sl + 1] : E;
            }
            const bool ne = sl < ns && b > a;
            const uint64_t bal = __ballot(ne);
            if (ne) rs[nr + (uint32_t)__popcll(bal & lt)] = a;
            nr += (uint32_t)__popcll(bal);
        }
        if (lane == 0) { rs[nr] = E; L.s_nr = nr; }
    }
    __syncthreads();
    uint32_t NR = L.s_nr;
    uint32_t *src = tmp, *dst = buf;
    const uint32_t CH = (E + NT - 1) / NT;
    while (NR > 1) {
        const uint32_t NP = (NR + 1) / 2;
        const uint32_t o0 = min(E, tid * CH), o1 = min(E, o0 + CH);
        if (o0 < o1) {
            uint32_t lo = 0, hi = NP;   // last pair with start <= o0
            while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (rs[2 * m] <= o0) lo = m; else hi = m; }
            uint32_t p = lo, q = o0;
            while (q < o1) {
                const uint32_t a0 = rs[2 * p], a1 = rs[min(2 * p + 1, NR)], b1 = rs[min(2 * p + 2, NR)];
                const uint32_t la = a1 - a0, lb = b1 - a1, end = min(o1, b1), d = q - a0;
                uint32_t i0 = d > lb ? d - lb : 0, i1 = min(d, la);
                while (i0 < i1) {
                    const uint32_t m = (i0 + i1) >> 1;
                    if (src[a0 + m] < src[a1 + d - 1 - m]) i0 = m + 1; else i1 = m;
                }
                uint32_t i = i0, j = d - i0;
                for (; q < end; ++q) {
                    const bool takeA = j >= lb || (i < la && src[a0 + i] < src[a1 + j]);
                    dst[q] = takeA ? src[a0 + i] : src[a1 + j];
                    i += takeA; j += !takeA;
                }
                ++p;
            }
        }
        __syncthreads();
        uint32_t nv = 0;
        if (tid < NP) nv = rs[2 * tid];
        __syncthreads();
        if (tid < NP) rs[tid] = nv;
        if (tid == 0) rs[NP] = E;
        __syncthreads();
        NR = NP;
        uint32_t *sw = src; src = dst; dst = sw;
    }
    return src;
}

template <int CAP, int NT>
__device__ void big_one(BigLds<CAP, NT> &L, uint32_t t, const V2View &v, const uint64_t *__restrict__ cnt, const V2Out &o)
{
    uint32_t *buf = L.buf;
    RunsT<BIG_K> &R = L.R;
    constexpr int NW = NT / 64;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
    TxnCtx c = txn_ctx(v, o, t);
    bool oversize = c.nk > BIG_K || c.E > CAP;
    if (!oversize) {
        if (tid < 64) compute_runs(R, v, o, cnt, c);
        if (tid < BIG_K)
            for (int w = 0; w < NW; ++w) L.wk_cnt[w][tid] = 0;
        if (tid == 0) L.s_kept = 0;
        __syncthreads();
        oversize = R.total > CAP;
    }
    if (oversize) {
        if (tid == 0) {
            if (CAP == MED_CAP && c.nk <= BIG_K) {
                uint32_t f = (uint32_t)atomicAdd((unsigned long long *)&o.gstat[1], 1ull);
                o.big_list[f] = t;
            } else if (CAP == BIG_E && c.nk <= BIG_K) {
                uint32_t f = (uint32_t)atomicAdd((unsigned long long *)&o.gstat[6], 1ull);
                o.huge_list[f] = t;
            } else {
                uint32_t f = (uint32_t)atomicAdd((unsigned long long *)&o.gstat[3], 1ull);
                atomicAdd((unsigned long long *)&o.gstat[4], (unsigned long long)c.E);
                o.fb_list[f] = t;
            }
        }
        return;
    }
    const uint32_t total = R.total;
    uint32_t n2 = 128;
    while (n2 < total) n2 <<= 1;
    // ---- gather: raw element e -> buf[e] (all-ones sentinel when dropped)
    uint32_t kept = 0;
    for (uint32_t e0 = tid; e0 < n2; e0 += BIG_GU * NT) {
        uint32_t idx[BIG_GU], kk[BIG_GU], x[BIG_GU];
        bool r3[BIG_GU], in[BIG_GU], il[BIG_GU];
#pragma unroll
        for (int u = 0; u < BIG_GU; ++u) {
            const uint32_t e = e0 + u * NT;
            in[u] = e < total;
            idx[u] = 0; kk[u] = 0; r3[u] = false; il[u] = false;
            if (in[u]) locate_elem(R, c.nk, e, idx[u], kk[u], r3[u], il[u]);
        }
#pragma unroll
        for (int u = 0; u < BIG_GU; ++u)
            x[u] = in[u] ? (il[u] ? inl_entry(v.irec32, v.rec, idx[u]) : r3[u] ? v.bc_rank[idx[u]] : v.list_rank[idx[u]]) : 0u;
#pragma unroll
        for (int u = 0; u < BIG_GU; ++u) {
            const uint32_t e = e0 + u * NT;
            bool keep = in[u] && (il[u] || !(c.bq && x[u] == c.trank));
            if (keep && r3[u]) keep = v.bc_exec[idx[u]] >= R.m[kk[u]] && ((c.wk >> v.bc_kind[idx[u]]) & 1u);
            kept += keep;
            if (e < n2) buf[e] = keep ? ((x[u] << 6) | kk[u]) : 0xFFFFFFFFu;
        }
    }
    kept = wave_inclusive(kept, OpAdd<uint32_t>());
    if (lane == 63) atomicAdd(&L.s_kept, kept);
    __syncthreads();
    if (L.s_kept != c.E) {
        if (tid == 0) atomicAdd((unsigned long long *)&o.gstat[2], 1ull);
        return;
    }
    if constexpr (big_merges<CAP>()) {
        buf = big_merge_sort<CAP, NT>(L, c.nk, total, c.E);
    } else {
        // ---- bitonic sort over n2 (one compare-exchange per pair index)
        for (uint32_t k = 2; k <= n2; k <<= 1) {
            for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
                for (uint32_t pi = tid; pi < (n2 >> 1); pi += NT) {
                    const uint32_t i = ((pi & ~(jj - 1)) << 1) | (pi & (jj - 1));
                    const uint32_t l = i | jj;
                    const uint32_t xa = buf[i], ya = buf[l];
                    const bool up = (i & k) == 0;
                    if ((xa > ya) == up) { buf[i] = ya; buf[l] = xa; }
                }
                __syncthreads();
            }
        }
    }
    // ---- emit: wave w owns sorted positions [w*Q, (w+1)*Q), Q a multiple of 64
    const uint32_t E = c.E;
    const uint32_t Q = ((E + NW * 64 - 1) / (NW * 64)) * 64;
    const uint32_t q_lo = min(E, wave * Q), q_hi = min(E, q_lo + Q);
    uint32_t nd = 0;
    for (uint32_t q0 = q_lo; q0 < q_hi; q0 += 64) {
        const uint32_t q = q0 + lane;
        const bool in = q < q_hi;
        const uint32_t xq = in ? buf[q] : 0;
        const bool nw = in && (q == 0 || (buf[q - 1] >> 6) != (xq >> 6));
        nd += (uint32_t)__popcll(__ballot(nw));
        if (in) atomicAdd(&L.wk_cnt[wave][xq & 63u], 1u);
    }
    if (lane == 0) L.wdist[wave] = nd;
    __syncthreads();
    if (tid < BIG_K) {   // exclusive prefix over waves, per key
        uint32_t run = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) { uint32_t x = L.wk_cnt[w][tid]; L.wk_cnt[w][tid] = run; run += x; }
    }
    __syncthreads();
    uint32_t distinct = 0;
    for (int w = 0; w < (int)wave; ++w) distinct += L.wdist[w];
    const uint64_t abase = o.arena_off[t] + (o.cnz[c.j1] - o.cnz[c.j0]);
    auto widen = [](uint32_t r) { return ((uint64_t)(r >> 6) << 16) | (r & 63u); };
    for (uint32_t q0 = q_lo; q0 < q_hi; q0 += 64) {
        const uint32_t q = q0 + lane;
        const bool in = q < q_hi;
        const uint64_t xq = in ? widen(buf[q]) : 0;
        const uint64_t prev = (in && q > 0) ? widen(buf[q - 1]) : 0;
        distinct = emit_chunk<false>(xq, in, prev, q > 0, distinct, L.wk_cnt[wave], o, c, abase);
    }
    if (wave == NW - 1 && lane == 0) o.u_cnt[t] = distinct;
    __syncthreads();   // the block's rank writes are visible to the block
    // ranks -> TxnIds over the txn's distinct entries, four independent load chains per thread
    uint32_t U = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) U += L.wdist[w];
    uint32_t *dsc = o.dep_scratch + c.e0;
    for (uint32_t i0 = tid; i0 < U; i0 += 4 * NT) {
        uint32_t r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = i0 + (uint32_t)u * NT < U ? dsc[i0 + (uint32_t)u * NT] : 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) if (i0 + (uint32_t)u * NT < U) r[u] = o.txn_of_rank[r[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u) if (i0 + (uint32_t)u * NT < U) dsc[i0 + (uint32_t)u * NT] = r[u];
    }
}

// Persistent over the routed list: blocks loop (a grid of one block per listed txn made the 128-KiB launch pay a
// block launch + exit per big txn). CAP = MED_CAP reads its count from gstat[0], BIG_E from gstat[1], HUGE_E from
// gstat[6].
template <int CAP, int NT>
__global__ __launch_bounds__(NT) void k_v2_write_big(const uint32_t *__restrict__ list, V2View v,
                                                     const uint64_t *__restrict__ cnt, V2Out o)
{
    __shared__ BigLds<CAP, NT> L;
    const uint32_t cnt_list = (uint32_t)o.gstat[CAP > BIG_E ? 6 : CAP == MED_CAP ? 0 : 1];
    for (uint32_t b = blockIdx.x; b < cnt_list; b += gridDim.x) {
        big_one<CAP, NT>(L, list[b], v, cnt, o);
        __syncthreads();
    }
}

// ---- window tier: the KeyDeps of a big txn through per-key bitmaps over its rank span, no sorting.
//
// A big txn (config 2 / 3: the uncommitted window's txns on hot keys, 10^3-10^4 entries) takes its dependency entries
// from ranks below its executeAt S. Every entry of key k at rank x in [base, S), base = S - WIN_W * 32, sets bit
// x - base of key k's bitmap; the union's bitmap is the OR of the keys' bitmaps. A key's entries are distinct TxnIds
// (its runs are disjoint classes), so the builder's per-key ascending index lists (RelationMultiMap.java:245-257) are
// the key's set bits in order and each entry's index into the sorted unique TxnIds (:201-226) is a prefix popcount of
// the union: O(E + keys * span / 32) work instead of a merge sort. Entries below base (a cold key's last committed
// Write far back) go to a short sorted list that precedes the bitmap span. A txn whose list overflows is passed on to
// the sorting tier (k_v2_write_big<BIG_E>).
// One wave sorts buf[0, 64 R) ascending with R entries per lane in registers (element r * 64 + lane; positions >=
// n_valid read as all-ones pads): partners closer than 64 are lanes (shuffles), the others registers of the same lane.
template <int R>
__device__ __forceinline__ void wave_reg_sort_u32(uint32_t *buf, uint32_t n_valid)
{
    const uint32_t lane = lane_id();
    uint32_t v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = (uint32_t)r * 64 + lane;
        v[r] = i < n_valid ? buf[i] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (uint32_t k = 2; k <= 64u * R; k <<= 1) {
#pragma unroll
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            if (jj >= 64) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int r2 = r ^ (int)(jj / 64);
                    if (r2 > r) {
                        const bool up = (((uint32_t)r * 64 + lane) & k) == 0;
                        const uint32_t a = v[r], b = v[r2];
                        if ((a > b) == up) { v[r] = b; v[r2] = a; }
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t y = xor_lanes(v[r], (int)jj);
                    const bool up = (((uint32_t)r * 64 + lane) & k) == 0, lower = (lane & jj) == 0;
                    const uint32_t lo = min(v[r], y), hi = max(v[r], y);
                    v[r] = (lower == up) ? lo : hi;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = (uint32_t)r * 64 + lane;
        if (i < n_valid) buf[i] = v[r];
    }
}

constexpr uint32_t WIN_W = 512;      // bitmap words per key: 16384 ranks below S
constexpr uint32_t WIN_OUT = 1024;   // entries below the span

// A txn's metadata as the tier uses it: staged in LDS one list item ahead by the prefetch wave (below)
template <int WK>
struct WinTxn {
    uint32_t t, j0, nk, E, S, trank, tz;
    uint64_t e0, abase;
    uint32_t koff[WK];   // dep_off[j0 + k] - e0: key k's first entry among the txn's
};

template <int WK>
struct WinLds {
    uint32_t bm[WK][WIN_W];
    uint32_t un[WIN_W];
    uint16_t pre[WK + 1][WIN_W];   // exclusive prefix popcounts per series (series WK... = the union, index nk)
    uint32_t out[WIN_OUT];         // (rank << 6 | key) of the entries below the span
    uint32_t out2[WIN_OUT];        // ... sorted, when the waves' sorted quarters are merged
    RunsT<WK> R[2];                // [list item of the block & 1]: the current txn's runs, the next one's
    WinTxn<WK> T[2];
    uint32_t kc[WK], out_k[WK], ser_tot[WK + 1];
    uint32_t n_out, kept, d_out, bad, minr;
};

// The loads of the next list item, in flight in the prefetch wave's registers while the block works on the current txn.
// They depend on the list item alone, a chain three levels deep (list -> txn -> pairs); one level is issued per phase of
// the current iteration, so each has landed when the next level needs it.
struct WinPre {
    uint32_t t, j0, j1;
    uint4 ti;
    uint64_t ao, dk;   // dk: lane k <= nk: dep_off[j0 + k]
    uint32_t cz0, cz1;
    RecRaw rr;         // lane k < nk: key k's record
};

// x in a vector register: a load indexed by it is a vector load. The prefetch chain starts from a block-uniform list index;
// as scalar loads its levels would be waited for at the next block barrier (scalar loads and LDS share a counter), as
// vector loads they stay in flight across the barriers until their values are used.
__device__ __forceinline__ uint32_t in_vgpr(uint32_t x)
{
    asm volatile("" : "+v"(x));
    return x;
}

__device__ __forceinline__ void win_pre_txn(WinPre &p, const V2View &v, const V2Out &o, uint32_t t)
{
    p.t = t;
    p.j0 = o.key_off[t]; p.j1 = o.key_off[t + 1];
    p.ti = v.tinfo[t];
    p.ao = o.arena_off[t];
}

__device__ __forceinline__ void win_pre_keys(WinPre &p, const V2Out &o, const uint64_t *cnt)
{
    const uint32_t lane = lane_id(), nk = p.j1 - p.j0;
    p.dk = lane <= nk ? o.dep_off[p.j0 + lane] : 0ull;
    p.cz0 = o.cnz[p.j0]; p.cz1 = o.cnz[p.j1];
    p.rr = RecRaw{};
    if (lane < nk) p.rr = load_rec_raw(o.rec, o.irec32, cnt, p.j0 + lane);
}

// (one wave) the landed loads into the LDS record and runs of the next iteration
template <int WK>
__device__ __forceinline__ void win_pre_land(WinTxn<WK> &T, RunsT<WK> &R, const WinPre &p)
{
    const uint32_t lane = lane_id(), nk = p.j1 - p.j0;
    const uint64_t e0 = shfl_idx(p.dk, 0), e1 = shfl_idx(p.dk, (int)nk);
    if (lane < nk) T.koff[lane] = (uint32_t)(p.dk - e0);
    if (lane == 0) {
        T.t = p.t; T.j0 = p.j0; T.nk = nk; T.E = (uint32_t)(e1 - e0);
        T.S = p.ti.y; T.trank = p.ti.x; T.tz = p.ti.z;
        T.e0 = e0; T.abase = p.ao + (p.cz1 - p.cz0);
    }
    finish_runs(R, p.rr, p.j0, nk);
}

// locate_elem with fixed trip counts (MAXK a power of two): the LDS reads of a thread's WIN_GU elements are independent and
// interleave, where the data-dependent loops of locate_elem run one element after the other
template <int MAXK>
__device__ __forceinline__ void locate_elem_flat(const RunsT<MAXK> &R, uint32_t nk, uint32_t e, uint32_t &idx, uint32_t &k, bool &r3,
                                                 bool &inl)
{
    static_assert((MAXK & (MAXK - 1)) == 0, "a power of two");
    k = 0;
#pragma unroll
    for (uint32_t st = MAXK / 2; st > 0; st >>= 1) {
        const uint32_t m = k + st, kb = R.kbase[m];
        if (m < nk && kb <= e) k = m;
    }
    const uint32_t off = e - R.kbase[k];
    inl = R.m[k] == INLINE_M;
    uint32_t r = 0;   // the last run that starts at or before off (the run starts ascend)
#pragma unroll
    for (int q = 1; q < NRUN; ++q) r += R.pre[k][q] <= off ? 1u : 0u;
    if (inl) { idx = 16 * R.start[k][0] + off; r3 = false; return; }
    idx = R.start[k][r] + (off - R.pre[k][r]);
    r3 = r == 6;
}

#ifdef ACC_PHASE_PROF
// tuning build only: per workgroup of the window tier, summed over its txns: cycles in the span's low end, bitmap gather,
// union words (+ the block sort of a long list below), below-span sort and writes beside the prefix popcounts, the span's
// writes; then txns, entries, span words, entries below; [9] the wait between txns
__device__ unsigned long long *g_win_prof;
#define WN_PH(k) do { if (tid == 0) { const unsigned long long t_ = clock64(); wp[k] += t_ - wq; wq = t_; } } while (0)
#else
#define WN_PH(k) ((void)0)
#endif
constexpr int WIN_GU = 8;  // independent elements per thread and round of the gather (a round: 2,048 raw elements)
constexpr int WIN_U = 4;   // TxnId loads in flight per union word of a thread in the span's writes
template <int WK>
__global__ __launch_bounds__(BLOCK) void k_v2_write_win(const uint32_t *__restrict__ list, const uint64_t *__restrict__ cnt_dev,
                                                       V2View v, const uint64_t *__restrict__ cnt, V2Out o)
{
    __shared__ WinLds<WK> L;
    static_assert(sizeof(WinLds<WK>) <= 64 * 1024, "the window tier's LDS");
    static_assert(WIN_W <= 2 * BLOCK, "a thread takes at most two union words");
    static_assert(WIN_OUT <= 4 * BLOCK, "a thread maps at most four TxnIds below the span");
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
    const uint32_t n_list = (uint32_t)*cnt_dev;
    // The last wave prefetches: the next list item's txn record, offsets and count-pass records are loaded during the
    // current txn's phases and land in L.T / L.R [cur ^ 1], so an iteration starts with its runs and offsets in LDS
    // instead of walking the chain list -> key_off / tinfo -> dep_off -> cnt / records with the block waiting on each.
    const bool pw = wave == WAVES - 1;
    WinPre np{};
    if (pw && blockIdx.x < n_list) {   // the block's first item: the chain in one go
        win_pre_txn(np, v, o, list[blockIdx.x]);
        win_pre_keys(np, o, cnt);
        win_pre_land(L.T[0], L.R[0], np);
    }
    __syncthreads();
#ifdef ACC_PHASE_PROF
    unsigned long long wp[10] = {}, wq = clock64();
#endif
    uint32_t cur = 0;
    // (every path to the next iteration, the two `continue`s too, lands the prefetch before its barrier and flips cur here)
    for (uint32_t b = blockIdx.x; b < n_list; b += gridDim.x, cur ^= 1u) {
        WN_PH(9);
        const bool pre = pw && b + gridDim.x < n_list;   // (never reads list[] at or past n_list)
        const WinTxn<WK> &T = L.T[cur];
        RunsT<WK> &R = L.R[cur];
        TxnCtx c;
        c.t = T.t; c.j0 = T.j0; c.nk = T.nk; c.j1 = c.j0 + c.nk; c.e0 = T.e0; c.E = T.E; c.trank = T.trank;
        const uint32_t t = c.t, S = T.S;
        c.bq = S != c.trank;
        c.wk = witnesses(T.tz >> 3);
        c.wc = wk_classes(c.wk);
        const uint64_t abase = T.abase;
        uint32_t tn = 0;
        if (pre) tn = list[in_vgpr(b + gridDim.x)];   // level 1
        if (tid < (uint32_t)WK) { L.kc[tid] = 0; L.out_k[tid] = 0; }
        if (tid == 0) { L.n_out = 0; L.kept = 0; L.bad = 0; L.minr = 0xFFFFFFFFu; }
        __syncthreads();
        // the span's low end: the smallest rank an entry can have (a class run's first entry, an inline record's first
        // entry, any entry of a short R3 run), so the bitmaps cover only [min, S) instead of 16,384 ranks below S
        uint32_t mn = 0xFFFFFFFFu;
        if (tid < c.nk) {
            const uint32_t k = tid;
            if (R.m[k] == INLINE_M) {
                if (R.pre[k][1] > 0) mn = v.irec32[IREC_W * (size_t)R.start[k][0]];
            } else {
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    if (R.pre[k][q + 1] > R.pre[k][q]) mn = min(mn, v.list_rank[R.start[k][q]]);
                if (R.pre[k][7] - R.pre[k][6] > 256) mn = 0u;   // (a long R3 run: from 0; a short one: below)
            }
        }
        // the short R3 runs' smallest ranks, the block's threads side by side, every key's load issued before the first is
        // used (one thread walking a run, or one key after the other, waits on one load at a time)
        uint32_t r3v[WK];
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)WK; ++k) {
            r3v[k] = 0xFFFFFFFFu;
            if (k < c.nk && R.m[k] != INLINE_M) {
                const uint32_t l3 = R.pre[k][7] - R.pre[k][6];
                if (l3 <= 256 && tid < l3) r3v[k] = v.bc_rank[R.start[k][6] + tid];
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)WK; ++k) mn = min(mn, r3v[k]);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) mn = min(mn, xor_lanes(mn, d));
        if (lane == 0) atomicMin(&L.minr, mn);
        if (pre) win_pre_txn(np, v, o, tn);   // level 2 (issued, not waited for)
        __syncthreads();
        const uint32_t lo_span = S > WIN_W * 32 ? S - WIN_W * 32 : 0u;
        uint32_t base = max(lo_span, min(L.minr, S));
        uint32_t nw = (S - base + 31) / 32;
        // a sparse span (fewer than one entry per 16 ranks: deps on old commands far below S) is all overhead, the
        // (nk + 1) bitmaps zeroed, scanned and walked word by word: every entry goes to the sorted list instead
        if (c.E <= WIN_OUT && (uint64_t)nw * 32 > 16ull * c.E) { base = S; nw = 0; }
        WN_PH(0);
        for (uint32_t i = tid; i < c.nk * nw; i += BLOCK) L.bm[i / nw][i % nw] = 0;
        __syncthreads();
        const uint32_t total = R.total;
        // ---- gather: bits of the span, the entries below it to the list
        uint32_t kept = 0;
        for (uint32_t e0 = tid; e0 < total; e0 += WIN_GU * BLOCK) {
            uint32_t idx[WIN_GU], kk[WIN_GU], x[WIN_GU];
            bool r3[WIN_GU], in[WIN_GU], il[WIN_GU];
#pragma unroll
            for (int u = 0; u < WIN_GU; ++u) {
                const uint32_t e = e0 + u * BLOCK;
                in[u] = e < total;
                idx[u] = 0; kk[u] = 0; r3[u] = false; il[u] = false;
                if (in[u]) locate_elem_flat(R, c.nk, e, idx[u], kk[u], r3[u], il[u]);
            }
#pragma unroll
            for (int u = 0; u < WIN_GU; ++u)
                x[u] = in[u] ? (il[u] ? inl_entry(v.irec32, v.rec, idx[u]) : r3[u] ? v.bc_rank[idx[u]] : v.list_rank[idx[u]]) : 0u;
            // an R3 element's filter columns with its rank, not after it (r3 implies in)
            uint32_t ex[WIN_GU], kd[WIN_GU];
#pragma unroll
            for (int u = 0; u < WIN_GU; ++u) {
                ex[u] = r3[u] ? v.bc_exec[idx[u]] : 0u;
                kd[u] = r3[u] ? (uint32_t)v.bc_kind[idx[u]] : 0u;
            }
#pragma unroll
            for (int u = 0; u < WIN_GU; ++u) {
                bool keep = in[u] && (il[u] || !(c.bq && x[u] == c.trank));
                if (keep && r3[u]) keep = ex[u] >= R.m[kk[u]] && ((c.wk >> kd[u]) & 1u);
                if (!keep) continue;
                ++kept;
                if (x[u] >= base) {
                    const uint32_t d = x[u] - base;
                    if (d < nw * 32) atomicOr(&L.bm[kk[u]][d >> 5], 1u << (d & 31));
                    else L.bad = 1;   // an entry at or above S: impossible for a scan below S
                } else {
                    const uint32_t i = atomicAdd(&L.n_out, 1u);
                    if (i < WIN_OUT) L.out[i] = (x[u] << 6) | kk[u];
                    atomicAdd(&L.out_k[kk[u]], 1u);
                }
            }
        }
        if (pre) win_pre_keys(np, o, cnt);   // level 3 (the pair range landed during the gather)
        kept = wave_inclusive(kept, OpAdd<uint32_t>());
        if (lane == 63) atomicAdd(&L.kept, kept);
        __syncthreads();
        if (L.kept != c.E || L.bad) {
            if (tid == 0) atomicAdd((unsigned long long *)&o.gstat[2], 1ull);
            if (pre) win_pre_land(L.T[cur ^ 1u], L.R[cur ^ 1u], np);
            __syncthreads();
            continue;
        }
        const uint32_t n_out = L.n_out;
        WN_PH(1);
#ifdef ACC_PHASE_PROF
        if (tid == 0) { wp[6] += 1; wp[7] += c.E; wp[8] += (uint64_t)nw << 32 | min(n_out, 0xFFFFFFFFu); }
#endif
        if (n_out > WIN_OUT) {   // too many entries below the span: the sorting tier
            if (tid == 0) {
                const uint32_t f = (uint32_t)atomicAdd((unsigned long long *)&o.gstat[1], 1ull);
                o.big_list[f] = t;
            }
            if (pre) win_pre_land(L.T[cur ^ 1u], L.R[cur ^ 1u], np);
            __syncthreads();
            continue;
        }
        // ---- union words
        for (uint32_t w = tid; w < nw; w += BLOCK) {
            uint32_t u = 0;
            for (uint32_t k = 0; k < c.nk; ++k) u |= L.bm[k][w];
            L.un[w] = u;
        }
        // ---- the entries below the span, sorted (rank, key). Up to 512: one wave in registers (no block barriers) beside
        // the other waves' prefix popcounts. Beyond: every wave sorts a quarter in registers, then each entry finds its
        // place among the other quarters' by binary search (the entries are distinct) and goes there in out2
        const bool blk_sort = n_out > 512;
        const uint32_t *srt = L.out;
        if (blk_sort) {
            const uint32_t Q = (n_out + WAVES - 1) / WAVES;   // <= 256
            const uint32_t q0 = min(wave * Q, n_out);
            wave_reg_sort_u32<4>(L.out + q0, min(Q, n_out - q0));
            __syncthreads();
            for (uint32_t i = tid; i < n_out; i += BLOCK) {
                const uint32_t x = L.out[i], own = i / Q;
                uint32_t pos = i - own * Q;
                for (uint32_t oq = 0; oq < (uint32_t)WAVES; ++oq) {
                    if (oq == own) continue;
                    const uint32_t s0 = min(oq * Q, n_out);
                    pos += lower_bound(L.out, s0, min(s0 + Q, n_out), x) - s0;
                }
                L.out2[pos] = x;
            }
            srt = L.out2;
        }
        __syncthreads();
        WN_PH(2);
        const bool side = n_out > 1 && !blk_sort;   // wave 0 sorts; the other waves take the prefix popcounts
        if (side && wave == 0) {
            if (n_out <= 128) wave_reg_sort_u32<2>(L.out, n_out);
            else if (n_out <= 256) wave_reg_sort_u32<4>(L.out, n_out);
            else wave_reg_sort_u32<8>(L.out, n_out);
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        }
        // ---- exclusive prefix popcounts of every series (keys 0..nk-1, union = nk): a wave per series, 8 words a lane
        const uint32_t pw0 = side ? 1u : 0u;
        if (wave >= pw0) {
            for (uint32_t s = wave - pw0; s <= c.nk; s += WAVES - pw0) {
                const uint32_t *words = s < c.nk ? L.bm[s] : L.un;
                uint32_t run = 0;
                for (uint32_t w0 = 0; w0 < nw; w0 += 512) {
                    const uint32_t wl = w0 + lane * 8;
                    uint32_t pc[8], sum = 0;
#pragma unroll
                    for (int i = 0; i < 8; ++i) { pc[i] = wl + i < nw ? (uint32_t)__popc(words[wl + i]) : 0u; sum += pc[i]; }
                    const uint32_t incl = wave_inclusive(sum, OpAdd<uint32_t>());
                    uint32_t r = run + incl - sum;
#pragma unroll
                    for (int i = 0; i < 8; ++i) if (wl + i < nw) { L.pre[s][wl + i] = (uint16_t)r; r += pc[i]; }
                    run += shfl_idx(incl, 63);
                }
                if (lane == 0) L.ser_tot[s] = run;
            }
        }
        uint32_t *dsc = o.dep_scratch + c.e0;
        uint32_t *drank = blk_sort ? L.out : L.out2;   // (the buffer the sorted entries are not in)
        // ---- the sorted entries below the span (one wave): distinct TxnIds first in the union, each key's first slots;
        // their ranks go to LDS and the block maps them to TxnIds with the span's (a load per chunk here would serialise
        // the chunks)
        if (wave == 0 && n_out) {
            const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
            uint32_t distinct = 0;
            for (uint32_t q0 = 0; q0 < n_out; q0 += 64) {
                const uint32_t q = q0 + lane;
                const bool in = q < n_out;
                const uint32_t xq = in ? srt[q] : 0u;
                const uint32_t kj = xq & 63u;
                const bool nw_ = in && (q == 0 || (srt[q - 1] >> 6) != (xq >> 6));
                const uint64_t bal = __ballot(nw_);
                const uint32_t idx = distinct + (uint32_t)__popcll(bal & lt) + (nw_ ? 1u : 0u) - 1u;
                uint64_t peers = __ballot(in);
#pragma unroll
                for (int bb = 0; bb < 6; ++bb) {
                    const uint64_t m = __ballot((kj >> bb) & 1u);
                    peers &= ((kj >> bb) & 1u) ? m : ~m;
                }
                const uint32_t before = (uint32_t)__popcll(peers & lt);
                if (in) {
                    o.arena[abase + T.koff[kj] + L.kc[kj] + before] = (int32_t)idx;
                    if (nw_) drank[idx] = xq >> 6;
                }
                __builtin_amdgcn_wave_barrier();
                if (in && before == 0) L.kc[kj] += (uint32_t)__popcll(peers);
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                distinct += (uint32_t)__popcll(bal);
            }
            if (lane == 0) L.d_out = distinct;
        } else if (tid == 0) {
            L.d_out = 0;
        }
        if (pre) win_pre_land(L.T[cur ^ 1u], L.R[cur ^ 1u], np);
        __syncthreads();
        WN_PH(3);
        // ---- the span. The union's words give its TxnId ranks: a thread takes WIN_U set bits of each of its (at most
        // two: WIN_W <= 2 BLOCK) words per round, loads their TxnIds together and stores them in place (no rank pass, no
        // read-back).
        const uint32_t d_out = L.d_out, nu = L.ser_tot[c.nk];
        uint32_t bits[2], rb[2], at[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const uint32_t w = tid + (uint32_t)u * BLOCK;
            const bool okw = w < nw;
            bits[u] = okw ? L.un[w] : 0u;
            rb[u] = base + 32 * w;
            at[u] = okw ? d_out + L.pre[c.nk][w] : 0u;
        }
        uint32_t r[2][WIN_U], br[4];
        bool h[2][WIN_U];
        // the first round's loads, and those of the TxnIds below the span (d_out <= WIN_OUT = 4 a thread), stay in flight
        // over the key items
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < WIN_U; ++q) {
                h[u][q] = bits[u] != 0;
                r[u][q] = h[u][q] ? rb[u] + (uint32_t)__builtin_ctz(bits[u]) : 0u;
                bits[u] &= bits[u] - 1;
            }
#pragma unroll
        for (int q = 0; q < 4; ++q) br[q] = tid + (uint32_t)q * BLOCK < d_out ? drank[tid + (uint32_t)q * BLOCK] : 0u;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < WIN_U; ++q)
                if (h[u][q]) r[u][q] = o.txn_of_rank[r[u][q]];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (tid + (uint32_t)q * BLOCK < d_out) br[q] = o.txn_of_rank[br[q]];
        // a key's words give its keysToTxnIds indices (union index = word prefix + popcount): item (key, word), the key's
        // first entry from LDS
        const uint32_t items = c.nk * nw;
        for (uint32_t i = tid; i < items; i += BLOCK) {
            const uint32_t s = i / nw, w = i - s * nw;
            uint32_t kb = L.bm[s][w];
            if (!kb) continue;
            const uint32_t ubase = d_out + L.pre[c.nk][w];
            const uint32_t uw = L.un[w];
            int32_t *dst = o.arena + abase + T.koff[s] + L.out_k[s] + L.pre[s][w];
            uint32_t j = 0;
            while (kb) {
                const uint32_t b2 = (uint32_t)__builtin_ctz(kb);
                dst[j] = (int32_t)(ubase + (uint32_t)__popc(uw & ((1u << b2) - 1u)));
                kb &= kb - 1;
                ++j;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (tid + (uint32_t)q * BLOCK < d_out) dsc[tid + (uint32_t)q * BLOCK] = br[q];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < WIN_U; ++q)
                if (h[u][q]) dsc[at[u]++] = r[u][q];
        while (bits[0] | bits[1]) {   // words with more than WIN_U set bits
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int q = 0; q < WIN_U; ++q) {
                    h[u][q] = bits[u] != 0;
                    r[u][q] = h[u][q] ? rb[u] + (uint32_t)__builtin_ctz(bits[u]) : 0u;
                    bits[u] &= bits[u] - 1;
                }
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int q = 0; q < WIN_U; ++q)
                    if (h[u][q]) r[u][q] = o.txn_of_rank[r[u][q]];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int q = 0; q < WIN_U; ++q)
                    if (h[u][q]) dsc[at[u]++] = r[u][q];
        }
        if (tid == 0) o.u_cnt[t] = d_out + nu;
        __syncthreads();
        WN_PH(4);
    }
#ifdef ACC_PHASE_PROF
    if (tid == 0)
        for (int k = 0; k < 10; ++k) atomicAdd(&g_win_prof[k], wp[k]);
#endif
}
#undef WN_PH

// ---- global path for txns beyond the wave path: gather to global, two radix sorts

__global__ __launch_bounds__(BLOCK) void k_v2_big_gather(uint32_t nbig, const uint32_t *__restrict__ big_list,
                                                         const uint64_t *__restrict__ big_off, V2View v,
                                                         const uint64_t *__restrict__ cnt, const uint32_t *__restrict__ key_off,
                                                         int rbits, int kbits, uint64_t *__restrict__ gkey)
{
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t b = blockIdx.x * WAVES + wave;
    if (b >= nbig) return;
    const uint32_t t = big_list[b];
    uint64_t *out = gkey + big_off[b];
    // reuse the wave appenders with an unbounded global buffer: WCAP guard off via a large cursor window
    const uint32_t lane = lane_id();
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const uint64_t tb = (uint64_t)b << (rbits + kbits);
    uint32_t cursor = 0;
    const uint32_t j0 = key_off[t], j1 = key_off[t + 1];
    for (uint32_t j = j0; j < j1; ++j) {
        if (cnt[j] == 0) continue;
        V2Query q = v2_query(v, v.pair_pos[j]);
        uint32_t kj = j - j0;
        for (int r = 0; r < 7; ++r) {
            const uint32_t *src;
            uint32_t a, e;
            bool r3 = r == 6;
            if (r3) {
                if (!q.has_m) continue;
                a = q.bstart; e = q.bend; src = v.bc_rank;
            } else {
                int c = r >> 1;
                if (!((q.wc >> c) & 1u)) continue;
                const int col = (r & 1) ? 3 + c : c;
                a = (r & 1) ? q.rm.c[col] : q.r0.c[col];
                e = q.rp.c[col];
                src = v.list_rank + v.bases[(r & 1) ? 3 + c : c];
            }
            for (uint32_t c = a; c < e; c += 64) {
                uint32_t i = c + lane;
                bool keep = false;
                uint32_t x = 0;
                if (i < e) {
                    x = src[i];
                    keep = !(q.bq && x == q.trank);
                    if (r3) keep = keep && v.bc_exec[i] >= q.m && ((q.wk >> v.bc_kind[i]) & 1u);
                }
                uint64_t bal = __ballot(keep);
                if (keep) out[cursor + (uint32_t)__popcll(bal & lt)] = tb | ((uint64_t)x << kbits) | kj;
                cursor += (uint32_t)__popcll(bal);
            }
        }
    }
}

// sorted by (txn, value, key): dense rank of value within txn; TxnId array for first occurrences
__global__ __launch_bounds__(BLOCK) void k_v2_big_newflag(uint64_t m, const uint64_t *__restrict__ skey, int kbits,
                                                          uint32_t *__restrict__ flag)
{
    uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    flag[i] = i == 0 || (skey[i] >> kbits) != (skey[i - 1] >> kbits);
}

__global__ __launch_bounds__(BLOCK) void k_v2_big_rank(uint64_t m, const uint64_t *__restrict__ skey, const uint32_t *__restrict__ incl,
                                                       const uint32_t *__restrict__ big_list, const uint64_t *__restrict__ big_off,
                                                       int rbits, int kbits, const uint32_t *__restrict__ key_off,
                                                       const uint64_t *__restrict__ dep_off, const uint32_t *__restrict__ txn_of_rank,
                                                       uint32_t *__restrict__ dep_scratch, uint64_t *__restrict__ u_cnt,
                                                       uint32_t *__restrict__ idx_by_pos1, uint64_t *__restrict__ key2)
{
    uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    uint64_t x = skey[i];
    uint32_t b = (uint32_t)(x >> (rbits + kbits));
    uint32_t val = (uint32_t)((x >> kbits) & ((1ull << rbits) - 1));
    uint32_t kj = (uint32_t)(x & ((1ull << kbits) - 1));
    uint64_t start = big_off[b];
    uint32_t base_incl = start == 0 ? 0 : incl[start - 1];
    uint32_t idx = incl[i] - base_incl - 1;
    uint32_t t = big_list[b];
    bool nw = i == start || (skey[i] >> kbits) != (skey[i - 1] >> kbits);
    if (nw) dep_scratch[dep_off[key_off[t]] + idx] = txn_of_rank[val];
    if (i + 1 == big_off[b + 1]) u_cnt[t] = idx + 1;
    idx_by_pos1[i] = idx;
    // arena order of the txn: (key, value); value of the second sort = this position
    key2[i] = ((uint64_t)b << (kbits + rbits)) | ((uint64_t)kj << rbits) | val;
}

__global__ __launch_bounds__(BLOCK) void k_v2_big_arena(uint64_t m, const uint32_t *__restrict__ sval2, const uint64_t *__restrict__ skey2,
                                                        const uint32_t *__restrict__ idx_by_pos1, const uint32_t *__restrict__ big_list,
                                                        const uint64_t *__restrict__ big_off, int rbits, int kbits,
                                                        const uint32_t *__restrict__ key_off, const uint32_t *__restrict__ cnz,
                                                        const uint64_t *__restrict__ arena_off, int32_t *__restrict__ arena)
{
    uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    uint32_t b = (uint32_t)(skey2[i] >> (kbits + rbits));
    uint32_t t = big_list[b];
    uint32_t kd = cnz[key_off[t + 1]] - cnz[key_off[t]];
    arena[arena_off[t] + kd + (i - big_off[b])] = (int32_t)idx_by_pos1[sval2[i]];
}

// per fallback txn: raw entry count; maxk[0] = the largest key count of a fallback txn (width of the key field of the
// global-tier sort keys: a txn may list any number of keys, Keys has no cap)
__global__ __launch_bounds__(BLOCK) void k_fb_sizes(uint32_t nfb, const uint32_t *__restrict__ fb_list,
                                                    const uint32_t *__restrict__ key_off, const uint64_t *__restrict__ dep_off,
                                                    uint64_t *__restrict__ fb_e, uint64_t *__restrict__ maxk)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint64_t nk = 0;
    if (i < nfb) {
        uint32_t t = fb_list[i];
        fb_e[i] = dep_off[key_off[t + 1]] - dep_off[key_off[t]];
        nk = key_off[t + 1] - key_off[t];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nk = max(nk, shfl_xor(nk, d));
    if (lane_id() == 0 && nk) atomicMax((unsigned long long *)maxk, (unsigned long long)nk);
}



// ---------------------------------------------------------------- v3: streaming write pass
//
// A txn with at most ST_G keys, at most ST_N2 dependency entries and at most ST_RAW raw run elements (config 2: ~99% of
// txns) is finished by one kernel, k_v3_stream: a tile of txns per block, one lane per key, takes the
// inline entries of its count-pass records and gathers the entries of its run records, sorts the (rank, key) entries
// in LDS, counts the distinct TxnIds, takes the tile's output offsets (arena, keys, TxnIds) from a decoupled look-back
// over the previous tiles' sizes and writes the final KeyDeps arrays (arena_off / kd_off / u_off, arena, key_idx,
// dep_txn) directly: one read of 64 B of record per pair, writes of the outputs only.
// The other ("big") txns take the v2 tiers into scratch arrays addressed by prefix sums over the big txns in txn
// order (k_v3_bigfill gives them per-pair offsets, so the tiers' indexing is unchanged), report their sizes to the
// stream pass; their KeyDeps headers, key indices and entries go straight to the final arrays.

constexpr int ST_G = 16;                      // lanes per txn of the stream pass (one key per lane)
constexpr int ST_N2 = 128;                    // its dependency entries (LDS sort buffer, power of two)
constexpr int ST_SLOT = ST_N2;                // TxnId scratch slot per stream txn (t * ST_SLOT)
constexpr uint32_t ST_RAW = 1024;             // raw run elements of a stream txn
constexpr int MK_G = 8;                       // lanes per txn of the mark pass

// Per txn, MK_G lanes: its KeyDeps sizes A = Kd + E (arena ints) and K = Kd (keys with >= 1 dependency) from the
// count-pass records' word 7 (the exclusive scans of A and K are the txns' arena / key offsets, so the stream pass needs
// no look-back), and the classification: a stream txn has <= ST_G keys and <= ST_N2 entries (and, with run records:
// bigflag = 1 from the count pass, <= ST_RAW raw run elements), else it is big (bigflag = 1: the v2 tiers). (8 lanes per
// txn measured faster than 16 for the 8-key txns of configs 2 / 3; a 16-lane stream pass with 8 lanes per txn lost:
// its sort and gather sizes are wave-uniform maxima over twice the txns.)
__global__ __launch_bounds__(BLOCK) void k_v3_mark(uint32_t n, const uint32_t *__restrict__ key_off,
                                                   const uint32_t *__restrict__ irec32, const uint4 *__restrict__ rec,
                                                   uint32_t *__restrict__ psz, uint32_t raw_cap,
                                                   uint32_t *__restrict__ bigflag, uint64_t *__restrict__ szA,
                                                   uint64_t *__restrict__ szK, uint64_t *__restrict__ any16,
                                                   uint64_t *__restrict__ eb, uint64_t *__restrict__ flagw)
{
    const uint32_t t = (blockIdx.x * BLOCK + threadIdx.x) / MK_G, sub = threadIdx.x & (MK_G - 1);
    if (t >= n) return;   // group-uniform: shuffles stay inside the group
    const uint32_t j0 = key_off[t], nk = key_off[t + 1] - j0;
    const bool run_rec = bigflag[t] != 0;
    // could be big: a run record, more than ST_G keys, or more than 8 keys (8 inline records hold at most 8 * 15 <= ST_N2
    // entries; more may sum past ST_N2)
    const bool maybe_big = run_rec || nk > 8u;
    uint32_t e = 0, kd = 0, raw = 0;
    for (uint32_t c0 = 0; c0 < nk; c0 += MK_G) {
        if (c0 + sub < nk) {
            const uint32_t w = irec32[IREC_W * (size_t)(j0 + c0 + sub) + 7];
            const uint32_t ej = w & ~REC_INLINE_FLAG;
            e += ej;
            kd += ej != 0;
            if (run_rec && !(w & REC_INLINE_FLAG)) {
                const uint4 *r = rec + 4 * (size_t)(j0 + c0 + sub);
                const uint4 r1 = r[1], r2 = r[2], r3 = r[3];
                raw += r1.z + r1.w + r2.x + r2.y + r2.z + r2.w + r3.y;
            }
            if (maybe_big) psz[j0 + c0 + sub] = ej;   // the big txns' per-pair entry counts (k_v3_bigfill)
        }
    }
#pragma unroll
    for (int d = 1; d < MK_G; d <<= 1) {
        e += __shfl_xor(e, d, 64);
        kd += __shfl_xor(kd, d, 64);
        raw += __shfl_xor(raw, d, 64);
    }
    // (an all-inline txn of 9-16 keys can hold up to 240 entries: beyond ST_N2 it is big)
    const bool big = nk > (uint32_t)ST_G || e > (uint32_t)ST_N2 || (run_rec && raw > raw_cap);
    if (sub == 0) {
        bigflag[t] = big ? 1u : 0u;
        // the two list flags in one word, scanned beside the sizes (k_v3_lists): big in the low half; in the high half a
        // stream txn with a run record (the RUNS stream pass)
        flagw[t] = (big ? 1ull : 0ull) | (run_rec && !big ? 1ull << 32 : 0ull);
        szA[t] = (uint64_t)kd + e;
        szK[t] = kd;
        eb[t] = big ? e : 0u;   // the big txns' entries: their TxnId scratch bases by the same multi-scan
        // a big txn of 9-16 keys with entries: the 16-key window tier has work (read at the host sync after the scans)
        if (big && e && nk > 8 && nk <= 16 && !*any16) atomicOr((unsigned long long *)any16, 1ull);
    }
}


// the big txns and the stream txns with a run record, each list in txn order: a txn's places are the two halves of the
// exclusive prefix of the mark pass's flag words (fewer than 2^30 txns: each half stays a count of its own)
__global__ __launch_bounds__(BLOCK) void k_v3_lists(uint32_t n, const uint64_t *__restrict__ flagw,
                                                    const uint64_t *__restrict__ fpos, uint32_t *__restrict__ blist,
                                                    uint32_t *__restrict__ rlist)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n) return;
    const uint64_t f = flagw[t];
    if (!f) return;
    const uint64_t p = fpos[t];
    if (f & 1u) blist[(uint32_t)p] = t;
    else rlist[(uint32_t)(p >> 32)] = t;
}
// tier routing of the big txns (thread per list entry, one atomic per list per block). With ranks within 25 bits: the
// window tier (<= 8 or <= 16 keys; gstat[7] / gstat[8]), else medium (E <= MED_E, <= MED_K keys) or the u32-record
// block tier; with wider ranks: the u64 wave tier (E <= MED_E, <= MED_K keys) or the global path.
__global__ __launch_bounds__(BLOCK) void k_v3_route(uint32_t nbig, const uint32_t *__restrict__ blist,
                                                    const uint32_t *__restrict__ key_off, const uint64_t *__restrict__ eb,
                                                    int big_ok, int win_ok, uint32_t *__restrict__ med_list,
                                                    uint32_t *__restrict__ big_list, uint32_t *__restrict__ fb_list,
                                                    uint32_t *__restrict__ w8_list, uint32_t *__restrict__ w16_list,
                                                    uint64_t *__restrict__ gstat)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool med = false, bg = false, fb = false, w8 = false, w16 = false;
    uint32_t t = 0;
    uint64_t E = 0;
    if (i < nbig) {
        t = blist[i];
        E = eb[t];
        const uint32_t nk = key_off[t + 1] - key_off[t];
        const bool win = E > 0 && big_ok && win_ok && nk <= 16;
        w8 = win && nk <= 8;
        w16 = win && nk > 8;
        med = E > 0 && !win && E <= (uint64_t)MED_E && nk <= (uint32_t)MED_K;
        bg = E > 0 && !win && !med && big_ok;
        fb = E > 0 && !win && !med && !big_ok;
    }
    __shared__ uint64_t lds[WAVES];
    __shared__ uint64_t base[5];
    const uint64_t packed = (med ? 1ull : 0ull) | (bg ? 1ull << 12 : 0ull) | (fb ? 1ull << 24 : 0ull) |
                            (w8 ? 1ull << 36 : 0ull) | (w16 ? 1ull << 48 : 0ull);
    uint64_t total;
    const uint64_t pre = block_exclusive(packed, OpAdd<uint64_t>(), lds, total);
    uint64_t efb = fb ? E : 0;
    uint64_t efb_tot;
    __syncthreads();
    block_exclusive(efb, OpAdd<uint64_t>(), lds, efb_tot);
    if (threadIdx.x < 5) {
        const int slot[5] = { 0, 1, 3, 7, 8 };
        const uint64_t cnt = (total >> (12 * threadIdx.x)) & 4095u;
        base[threadIdx.x] = cnt ? atomicAdd((unsigned long long *)&gstat[slot[threadIdx.x]], (unsigned long long)cnt) : 0ull;
    }
    if (threadIdx.x == 0 && efb_tot) atomicAdd((unsigned long long *)&gstat[4], (unsigned long long)efb_tot);
    __syncthreads();
    if (med) med_list[base[0] + (pre & 4095u)] = t;
    if (bg) big_list[base[1] + ((pre >> 12) & 4095u)] = t;
    if (fb) fb_list[base[2] + ((pre >> 24) & 4095u)] = t;
    if (w8) w8_list[base[3] + ((pre >> 36) & 4095u)] = t;
    if (w16) w16_list[base[4] + ((pre >> 48) & 4095u)] = t;
}

struct V3Big {
    const uint32_t *blist, *key_off;
    const uint32_t *psz;                      // per pair of a big txn: its entry count (k_v3_mark)
    const uint64_t *dB;                       // per txn: exclusive prefix of the big txns' E (TxnId scratch bases)
    const uint64_t *arena_off, *kd_off;       // the batch's final offsets (from the mark pass's scans)
    uint64_t *vdep_off, *vcnt;                // per pair of a big txn (dep_off / cnt of the v2 tiers)
    uint32_t *vcnz;                           // per pair of a big txn (cnz)
    uint64_t *u_cnt;                          // per txn (big txns only)
    int32_t *arena;
    uint32_t *key_idx;
};

// per big txn (one wave): the v2 tiers' per-pair offsets, and the KeyDeps header and key indices straight into the
// final arena / key_idx (the tiers then write the entries at arena_off[t] too: no copy into place afterwards)
__global__ __launch_bounds__(BLOCK) void k_v3_bigfill(uint32_t nbig, V3Big b)
{
    const uint32_t lane = lane_id();
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (uint32_t i = blockIdx.x * WAVES + (threadIdx.x >> 6); i < nbig; i += gridDim.x * WAVES) {
        const uint32_t t = b.blist[i], j0 = b.key_off[t], j1 = b.key_off[t + 1], nk = j1 - j0;
        const uint64_t dbase = b.dB[t], kbase = b.kd_off[t], abase = b.arena_off[t];
        const uint64_t E = b.dB[t + 1] - dbase, Kd = b.kd_off[t + 1] - kbase;
        uint64_t ecur = 0, kcur = 0;
        for (uint32_t c0 = 0; c0 < nk; c0 += 64) {
            const uint32_t j = j0 + c0 + lane;
            const bool in = c0 + lane < nk;
            const uint32_t e = in ? b.psz[j] : 0u;
            const uint64_t einc = wave_inclusive((uint64_t)e, OpAdd<uint64_t>());
            const uint64_t nzb = __ballot(e != 0);
            const uint32_t kb = (uint32_t)__popcll(nzb & lt);
            if (in) {
                const uint64_t eoff = ecur + einc - e;
                b.vdep_off[j] = dbase + eoff;
                b.vcnt[j] = e;
                b.vcnz[j] = (uint32_t)(kbase + kcur + kb);
                if (e) {
                    b.arena[abase + kcur + kb] = (int32_t)(Kd + eoff + e);
                    b.key_idx[kbase + kcur + kb] = c0 + lane;
                }
            }
            ecur += shfl_idx(einc, 63);
            kcur += (uint64_t)__popcll(nzb);
        }
        if (lane == 0) {
            b.vdep_off[j1] = dbase + E;
            b.vcnz[j1] = (uint32_t)(kbase + Kd);
            b.u_cnt[t] = 0;
        }
    }
}

struct V3Stream {
    V2View v;
    const uint32_t *key_off, *bigflag, *txn_of_rank;
    const uint32_t *list;                     // LIST: the txns of the pass (else every txn, the stream ones taken)
    const uint4 *rec, *irec;
    const uint64_t *arena_off, *kd_off;       // from the size scans
    uint64_t *u_cnt_out;
    int32_t *arena;
    uint32_t *key_idx, *dep_scr;              // dep_scr: TxnIds at the txn's slot t * ST_SLOT, compacted by k_v3_ucompact
    uint64_t *err;                            // gather count mismatches
    // a pass enqueued ahead of the size read-back (e_dev set): the batch's E as the size scan left it, the pairs P and
    // the ints the arena buffer holds. Every wave leaves before its first store when P + E does not fit.
    const uint64_t *e_dev;
    uint64_t pairs, arena_cap;
    uint32_t t0;                              // !LIST: the pass takes the txns [t0, t0 + n)
    uint32_t n, ntiles;
};

// inclusive prefix over the G lanes of a group
template <int G>
__device__ __forceinline__ uint32_t group_inclusive(uint32_t x, uint32_t sub)
{
#pragma unroll
    for (uint32_t d = 1; d < (uint32_t)G; d <<= 1) {
        const uint32_t u = __shfl_up(x, d, 64);
        if (sub >= d) x += u;
    }
    return x;
}

template <class T>
__device__ __forceinline__ T gshfl_xor(T v, int m)
{
    return xor_lanes(v, m);   // (group_reg_sort runs in the whole wave: no lane of k_v3_stream returns early)
}
// Sorts buf[0, G * R) of a G-lane group ascending (positions >= n_valid read as all-ones pads) with R entries per lane
// in registers, element i = r * G + sub: partners at distance < G are lanes of the group (shuffles), the others registers
// of the same lane. Writes the sorted entries back.
template <class EntT, int G, int R>
__device__ __forceinline__ void group_reg_sort(EntT *buf, uint32_t sub, uint32_t n_valid)
{
    EntT v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = r * G + sub;
        v[r] = i < n_valid ? buf[i] : ~(EntT)0;
    }
#pragma unroll
    for (uint32_t k = 2; k <= (uint32_t)(G * R); k <<= 1) {
#pragma unroll
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            if (jj >= (uint32_t)G) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int r2 = r ^ (int)(jj / G);
                    if (r2 > r) {
                        const bool up = (((uint32_t)r * G + sub) & k) == 0;
                        const EntT a = v[r], b = v[r2];
                        if ((a > b) == up) { v[r] = b; v[r2] = a; }
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const EntT y = gshfl_xor(v[r], (int)jj);
                    const bool up = (((uint32_t)r * G + sub) & k) == 0, lower = (sub & jj) == 0;
                    const EntT lo = v[r] < y ? v[r] : y, hi = v[r] < y ? y : v[r];
                    v[r] = (lower == up) ? lo : hi;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) buf[r * G + sub] = v[r];
}

#ifdef ACC_PHASE_PROF
// tuning build only (tools/build_prof.sh): per-phase wave cycles of k_v3_stream, one row of 8 per wave (no atomics)
__device__ unsigned long long *g_st_prof;
__device__ unsigned long long *g_sr_prof;   // the RUNS instance's rows (its own waves: the lean pass's rows stay as they were)
#define ST_PH(i) ph[i] = clock64()
#else
#define ST_PH(i) ((void)0)
#endif

// The share of the lean pass enqueued ahead of the size read-back: the first 1 / ACC_AHEAD_DIV of the txns. The whole
// pass ahead (1) fills every CU before the window tier arrives, whose 37-KB blocks then wait for LDS until the lean
// grid is spent (v2_write_win 0.56 -> 0.67 ms, and it ends the phase); a share that lasts about as long as the
// read-back and the side-stream launches take keeps the GPU busy there and leaves the tier its places.
#ifndef ACC_AHEAD_DIV
#define ACC_AHEAD_DIV 8
#endif
// EntT: u32 (rank << 4 | key) when ranks fit 28 bits, else u64
#ifndef ACC_ST_WAVES
#define ACC_ST_WAVES 24   // resident waves per CU the stream pass is compiled for (32: a 64-VGPR budget that spills)
#endif
// G lanes per txn (one key each), N2 entries per txn at most. LIST = false: every txn (the stream ones taken); true: the
// txns of s.list[0, s.n).
template <class EntT, int NT, int G, int N2, bool LIST, bool RUNS>
__global__ __launch_bounds__(NT, ACC_ST_WAVES * 64 / NT) void k_v3_stream(V3Stream s)
{
    constexpr int TT = NT / G;   // txns per tile
    constexpr uint32_t KB = G <= 8 ? 3 : 4;   // key bits under the rank in an entry
    static_assert(G <= 16, "entries keep the key index in 4 bits");
#ifdef ACC_PHASE_PROF
    uint64_t ph[8];
#endif
    ST_PH(0);
    // wave-uniform, and the kernel has no block barrier: no wave waits for one that left
    if (s.e_dev && s.pairs + *s.e_dev > s.arena_cap) return;
    __shared__ EntT ent[TT][N2];
    __shared__ uint32_t kc[TT][G];
    __shared__ uint32_t kbase[TT][G];
    __shared__ uint16_t stA[TT][G + N2];
    const uint32_t tid = threadIdx.x, lane = lane_id(), sub = lane & (G - 1), grp = tid / G, g0 = lane & (64 - G);
    const uint64_t gmask = ((1ull << G) - 1) << g0;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    // no block barriers: every wave is independent (its txns' arena / key offsets come from the size scans)
    const uint32_t tile = blockIdx.x * (NT / 64) + (tid >> 6);   // wave tile: 64 / G txns
    const uint32_t slot = tile * (64 / G) + lane / G;
    const bool valid = slot < s.n;
    const uint32_t t = LIST ? (valid ? s.list[slot] : 0u) : s.t0 + slot;
    TxnCtx c{};
    bool big = false;
    uint64_t aoff = 0, koff = 0;
    if (valid) {
        c.t = t;
        // independent loads issued together (the txn record is read even for big txns, which ignore it)
        c.j0 = s.key_off[t]; c.j1 = s.key_off[t + 1];
        const uint32_t bf = s.bigflag[t];
        const uint4 ti = s.v.tinfo[t];
        aoff = s.arena_off[t]; koff = s.kd_off[t];
        c.nk = c.j1 - c.j0;
        big = bf != 0;
        c.trank = ti.x;
        c.bq = ti.y != c.trank;
        c.wk = witnesses(ti.z >> 3);
    }
    const bool sm = valid && !big;
    EntT *buf = ent[grp];
    ST_PH(1);
    // ---- records: inline entries straight to LDS; a run record's runs stay in its lane's registers (RUNS only: the
    // lean pass leaves a txn with a run record to the RUNS pass, which the mark pass listed it for)
    uint32_t e = 0, rawk = 0;
    bool run = false;
    uint4 r0 = {}, r1 = {}, r2 = {}, r3 = {};
    if (sm && sub < c.nk) {
        const uint4 *ir = s.irec + 2 * (size_t)(c.j0 + sub);
        r0 = ir[0]; r1 = ir[1];
        const uint32_t w = r1.w;
        if (w & REC_INLINE_FLAG) {
            e = w & ~REC_INLINE_FLAG;
            if (e > IREC_N) {   // entries 7.. in the first half of the 64-B slot
                const uint4 *r = s.rec + 4 * (size_t)(c.j0 + sub);
                r2 = r[0]; r3 = r[1];
            }
        } else {
            run = true;
            e = w;
            if constexpr (RUNS) {
                const uint4 *r = s.rec + 4 * (size_t)(c.j0 + sub);
                r0 = r[0]; r1 = r[1]; r2 = r[2]; r3 = r[3];
                rawk = r1.z + r1.w + r2.x + r2.y + r2.z + r2.w + r3.y;
            }
        }
    }
    const uint32_t ein = run ? 0u : e;
    const uint32_t e_incl = group_inclusive<G>(e, sub), in_incl = group_inclusive<G>(ein, sub);
    const uint32_t E = __shfl(e_incl, (int)(g0 + G - 1), 64);
    const uint32_t E_in = __shfl(in_incl, (int)(g0 + G - 1), 64);
    const uint64_t nzb = __ballot(e != 0) & gmask;
    const uint32_t Kd = (uint32_t)__popcll(nzb);
    const uint64_t A = sm ? (uint64_t)Kd + E : 0;
    kbase[grp][sub] = e_incl - e;
    kc[grp][sub] = 0;
    if (sm && !run) {
        const uint32_t w[REC_INLINE] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w };
        const uint32_t b0 = in_incl - ein;
#pragma unroll
        for (uint32_t q = 0; q < REC_INLINE; ++q)
            if (q < e) buf[b0 + q] = ((EntT)w[q] << KB) | (EntT)sub;
    }
    ST_PH(2);
    // ---- run records, one key at a time (its runs broadcast from the owning lane): the group gathers the flattened
    // runs R1/R2 per class and R3, dropping T itself and R3 entries below M or of unwitnessed kinds, after the inline
    // entries
    const uint64_t runmask = __ballot(sm && run) & gmask;
    uint32_t wnrun = RUNS ? (uint32_t)__popcll(runmask) : 0u;
#pragma unroll
    for (int d = G; d < 64; d <<= 1) wnrun = max(wnrun, xor_lanes(wnrun, d));
    uint32_t cursor = E_in;
    uint64_t rem = runmask;
    for (uint32_t ri = 0; ri < wnrun; ++ri) {
        const bool has = rem != 0;
        const int src = has ? (int)__builtin_ctzll(rem) : (int)lane;
        rem &= rem - 1;
        uint32_t st[NRUN], len[NRUN];
        st[0] = __shfl(r0.x, src, 64); st[1] = __shfl(r0.y, src, 64); st[2] = __shfl(r0.z, src, 64);
        st[3] = __shfl(r0.w, src, 64); st[4] = __shfl(r1.x, src, 64); st[5] = __shfl(r1.y, src, 64);
        st[6] = __shfl(r3.x, src, 64);
        len[0] = __shfl(r1.z, src, 64); len[1] = __shfl(r1.w, src, 64); len[2] = __shfl(r2.x, src, 64);
        len[3] = __shfl(r2.y, src, 64); len[4] = __shfl(r2.z, src, 64); len[5] = __shfl(r2.w, src, 64);
        len[6] = __shfl(r3.y, src, 64);
        const uint32_t mk = __shfl(r3.z, src, 64);
        const uint32_t raw = has ? __shfl(rawk, src, 64) : 0u;
        const uint32_t kj = (uint32_t)(src - (int)g0);
        uint32_t wr = raw;
#pragma unroll
        for (int d = G; d < 64; d <<= 1) wr = max(wr, xor_lanes(wr, d));
        for (uint32_t c0 = 0; c0 < wr; c0 += G) {
            const uint32_t off = c0 + sub;
            bool keep = false;
            uint32_t x = 0;
            if (off < raw) {
                uint32_t idx = 0, acc = 0;
                bool r3run = false, found = false;
#pragma unroll
                for (int q = 0; q < NRUN; ++q) {
                    if (!found && off < acc + len[q]) { found = true; idx = st[q] + (off - acc); r3run = q == 6; }
                    acc += len[q];
                }
                if (r3run) {
                    x = s.v.bc_rank[idx];
                    keep = s.v.bc_exec[idx] >= mk && ((c.wk >> s.v.bc_kind[idx]) & 1u);
                } else {
                    x = s.v.list_rank[idx];
                    keep = true;
                }
                keep = keep && !(c.bq && x == c.trank);
            }
            const uint64_t bal = __ballot(keep) & gmask;
            if (keep) {
                const uint32_t at = cursor + (uint32_t)__popcll(bal & lt);
                if (at < (uint32_t)N2) buf[at] = ((EntT)x << KB) | (EntT)kj;
            }
            cursor += (uint32_t)__popcll(bal);
        }
    }
    ST_PH(3);
    bool ok = sm && (RUNS || !runmask);   // (the lean pass skips a txn with a run record: the RUNS pass takes it)
    if (ok && cursor != E) {
        if (sub == 0) atomicAdd((unsigned long long *)s.err, 1ull);
        ok = false;
    }
    uint32_t wE = ok ? E : 0;
#pragma unroll
    for (int d = G; d < 64; d <<= 1) wE = max(wE, xor_lanes(wE, d));
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    // ---- sort each group's entries: registers + shuffles up to 4 per lane (wave-uniform choice), LDS bitonic beyond
    if (wE <= (uint32_t)G) group_reg_sort<EntT, G, 1>(buf, sub, ok ? E : 0);
    else if (wE <= 2u * G) group_reg_sort<EntT, G, 2>(buf, sub, ok ? E : 0);
    else if (wE <= 4u * G) group_reg_sort<EntT, G, 4>(buf, sub, ok ? E : 0);
    else {
        uint32_t n2 = G;
        while (n2 < E) n2 <<= 1;
        if (!ok) n2 = 0;
        for (uint32_t q = E + sub; q < n2; q += G) buf[q] = ~(EntT)0;
        uint32_t wn2 = n2;
#pragma unroll
        for (int d = G; d < 64; d <<= 1) wn2 = max(wn2, xor_lanes(wn2, d));
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        for (uint32_t k = 2; k <= wn2; k <<= 1) {
            for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
                if (k <= n2) {
                    for (uint32_t pi = sub; pi < (n2 >> 1); pi += G) {
                        const uint32_t i = ((pi & ~(jj - 1)) << 1) | (pi & (jj - 1));
                        const uint32_t l = i | jj;
                        const EntT xa = buf[i], ya = buf[l];
                        const bool up = (i & k) == 0;
                        if ((xa > ya) == up) { buf[i] = ya; buf[l] = xa; }
                    }
                }
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    ST_PH(4);
    // ---- KeyDeps in LDS: the arena (header ints and per-key TxnId indices) staged as u16; the distinct TxnIds go
    // straight to the txn's fixed scratch slot t * ST_SLOT
    uint32_t distinct = 0;
    if (ok && e != 0) stA[grp][(uint32_t)__popcll(nzb & lt)] = (uint16_t)(Kd + e_incl);
    for (uint32_t q0 = 0; q0 < wE; q0 += G) {
        const uint32_t q = q0 + sub;
        const bool in = ok && q < E;
        const EntT x = in ? buf[q] : (EntT)0;
        const EntT pv = (in && q > 0) ? buf[q - 1] : (EntT)0;
        const uint32_t kj = (uint32_t)(x & ((1u << KB) - 1u));
        const bool nw = in && (q == 0 || (x >> KB) != (pv >> KB));
        const uint64_t bal = __ballot(nw) & gmask;
        const uint32_t idx = distinct + (uint32_t)__popcll(bal & lt) + (nw ? 1u : 0u) - 1u;
        uint64_t peers = __ballot(in) & gmask;
#pragma unroll
        for (uint32_t bb = 0; bb < KB; ++bb) {
            const uint64_t m = __ballot((kj >> bb) & 1u);
            peers &= ((kj >> bb) & 1u) ? m : ~m;
        }
        const uint32_t before = (uint32_t)__popcll(peers & lt);
        if (in) {
            stA[grp][Kd + kbase[grp][kj] + kc[grp][kj] + before] = (uint16_t)idx;
            if (nw) s.dep_scr[(size_t)t * ST_SLOT + idx] = s.txn_of_rank[(uint32_t)(x >> KB)];
        }
        __builtin_amdgcn_wave_barrier();
        if (in && before == 0) kc[grp][kj] += (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        distinct += (uint32_t)__popcll(bal);
    }
    if (ok && sub == 0) s.u_cnt_out[t] = distinct;
    ST_PH(5);
    // ---- the staged arena and key indices to their places
    if (!valid) return;
    if (ok) {
        for (uint32_t q = sub; q < (uint32_t)A; q += G) s.arena[aoff + q] = (int32_t)stA[grp][q];
        if (e != 0) s.key_idx[koff + (uint32_t)__popcll(nzb & lt)] = sub;
    }
#ifdef ACC_PHASE_PROF
    ST_PH(6);
    if (lane == 0) {
        unsigned long long *row = (LIST ? g_sr_prof : g_st_prof) + 8 * (size_t)tile;
        for (int i = 0; i < 6; ++i) row[i] = ph[i + 1] - ph[i];
        row[7] = 1;
    }
#endif
}

// Sparse batches (a mixed batch's range txns have no KeyDeps of their own here): the txns with TxnIds, compacted with
// their u_off, so k_v3_ucompact's chunks span a few txns each instead of long runs of empty ones.
__global__ __launch_bounds__(BLOCK) void k_v3_neflag(uint32_t n, const uint64_t *__restrict__ u_cnt, uint32_t *__restrict__ flag)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < n) flag[t] = u_cnt[t] != 0;
}

__global__ __launch_bounds__(BLOCK) void k_v3_nelist(uint32_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                     const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ u_off,
                                                     uint32_t *__restrict__ ne_t, uint64_t *__restrict__ ne_uoff)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < n && flag[t]) { ne_t[pos[t]] = t; ne_uoff[pos[t]] = u_off[t]; }
    if (t == 0) ne_uoff[*cnt] = u_off[n];
}

// KeyDeps.txnIds: each txn's distinct TxnIds from its scratch (stream txns: at its slot t * ST_SLOT of dep_scr; big
// txns: at vdep_off of its first pair in dep_big) to dep_txn[u_off[t] ...). A block takes a fixed chunk
// of UC_CHUNK outputs (the uncommitted window's txns are consecutive and hold most TxnIds: partitioning by txns left a
// few blocks with most of the work), finds the txns spanning it by binary search over u_off, and strides over the
// chunk in windows of BLOCK txns (u_off / source bases in LDS, each output's txn by binary search there).
constexpr uint32_t UC_CHUNK = 4096;

// tmap (optional): the txns are tmap[0, *n_dev) with offsets u_off[0, *n_dev] (the non-empty txns of a sparse batch,
// k_v3_nelist), else 0..n-1 over the batch's u_off.
__global__ __launch_bounds__(BLOCK) void k_v3_ucompact(uint32_t n, const uint64_t *__restrict__ u_off,
                                                       const uint64_t *__restrict__ arena_off, const uint64_t *__restrict__ kd_off,
                                                       const uint32_t *__restrict__ bigflag, const uint32_t *__restrict__ key_off,
                                                       const uint64_t *__restrict__ vdep_off, const uint32_t *__restrict__ dep_scr,
                                                       const uint32_t *__restrict__ dep_big,
                                                       const uint32_t *__restrict__ tmap, const uint32_t *__restrict__ n_dev,
                                                       uint32_t *__restrict__ dep_txn, const uint64_t *__restrict__ u_all,
                                                       uint64_t *__restrict__ totals)
{
    __shared__ uint64_t uo[BLOCK + 1];
    __shared__ uint64_t src[BLOCK];
    __shared__ uint32_t s_t[2];
    const uint32_t tid = threadIdx.x;
    if (tid == 0 && blockIdx.x == gridDim.x - 1) {   // the batch totals beside the status words: one host copy
        totals[0] = arena_off[n]; totals[1] = kd_off[n]; totals[2] = u_all[n];
    }
    if (tmap) n = *n_dev;
    const uint64_t total = u_off[n];
    const uint64_t c0 = (uint64_t)blockIdx.x * UC_CHUNK;
    if (c0 >= total) return;
    const uint64_t c1 = min(total, c0 + UC_CHUNK);
    if (tid == 0) { s_t[0] = seg_of(u_off, n, c0); s_t[1] = seg_of(u_off, n, c1 - 1); }
    __syncthreads();
    const uint32_t tlo = s_t[0], thi = s_t[1];
    auto source = [&](uint32_t j) {
        const uint32_t t = tmap ? tmap[j] : j;
        return bigflag[t] ? (vdep_off[key_off[t]] | (1ull << 63)) : (uint64_t)t * ST_SLOT;
    };
    if (thi - tlo >= 8 * BLOCK) {
        // sparse chunk (long runs of txns without TxnIds, e.g. the range txns of a mixed batch): every output finds its
        // txn by a binary search of u_off over the chunk's txn span
        for (uint64_t i = c0 + tid; i < c1; i += BLOCK) {
            const uint32_t lo = tlo + seg_of(u_off + tlo, thi + 1 - tlo, i);
            const uint64_t sb = source(lo), off = i - u_off[lo];
            dep_txn[i] = (sb >> 63) ? dep_big[(sb & ~(1ull << 63)) + off] : dep_scr[sb + off];
        }
        return;
    }
    // dense chunk: windows of BLOCK txns, offsets and sources staged in LDS
    for (uint32_t tw = tlo; tw <= thi; tw += BLOCK) {
        const uint32_t nt = min((uint32_t)BLOCK, thi + 1 - tw);
        __syncthreads();
        if (tid < nt) {
            uo[tid] = u_off[tw + tid];
            src[tid] = source(tw + tid);
        }
        if (tid == 0) uo[nt] = u_off[tw + nt];
        __syncthreads();
        const uint64_t lo = max(c0, uo[0]), hi = min(c1, uo[nt]);
        constexpr int U = 4;   // outputs per thread whose scratch and TxnId loads are in flight together
        for (uint64_t i0 = lo + tid; i0 < hi; i0 += U * BLOCK) {
            uint32_t x[U];
            bool big[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t i = i0 + (uint64_t)u * BLOCK;
                x[u] = 0; big[u] = false;
                if (i < hi) {
                    const uint32_t a = seg_of(uo, nt, i);
                    const uint64_t sb = src[a], off = i - uo[a];
                    big[u] = (sb >> 63) != 0;
                    x[u] = big[u] ? dep_big[(sb & ~(1ull << 63)) + off] : dep_scr[sb + off];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (i0 + (uint64_t)u * BLOCK < hi) dep_txn[i0 + (uint64_t)u * BLOCK] = x[u];
        }
    }
}

// ---------------------------------------------------------------- host orchestration

// What the prep words fix of the pair sort, before any rank exists: the key compaction, the rank and slot widths, and
// whether the sort will be a packed keys-only one (modes 3 and 4, which sort_pairs then tells apart).
static bool pair_plan(CfkBuild &cb)
{
    PairPlan &pp = cb.pp;
    pp.rk = make_runs(cb.dict.hg[3]);
    pp.rbits = cb.dict.rbits;
    pp.sb = std::max(1, bits_for(cb.dict.hg[6]));   // bounds the key slot within a txn (hg[6] = OR of the key counts)
    return cb.dict.batch_sorted && pp.rk.bits <= 32;
}

// The bumped committed entries in (segment, executeAt) order from the txn side (kernels k_bcx_*), enqueued on the side
// lane behind the sorted-batch dictionary: counts of the bumped txns in executeAt order, their exclusive scan, the expand,
// a keys-only sort on the key-code bits (nbc from the prep sync sizes it), the columns and the nearest-Write scan.
static void bc_from_txns(acc_ctx *ctx, CfkBuild &cb)
{
    const uint32_t n = cb.n, nb = cb.dict.nb;
    const uint64_t nbc = cb.dict.nbc;
    const PairPlan &pp = cb.pp;
    const int rbits = cb.dict.rbits;
    uint32_t *bt = ctx->get<uint32_t>("bcx_txn", nb);
    uint32_t *cnt = ctx->get<uint32_t>("bcx_cnt", nb);
    uint32_t *off = ctx->get<uint32_t>("bcx_off", (size_t)nb + 1);
    uint64_t *keys = ctx->get<uint64_t>("bcx_key", nbc);
    cb.bcs_exec = ctx->get<uint32_t>("v2_bcs_exec", nbc);
    uint64_t *lw_in = ctx->get<uint64_t>("v2_bcs_lw_in64", nbc);
    cb.bcs_lastw64 = ctx->get<uint64_t>("v2_bcs_lastw64", nbc);
    cb.bc_side = true;
    if (nbc == 0) return;   // (then nothing reads the arrays: every segment's range of the list is empty)
    ctx->stat("keydeps.bc_sort_passes", (uint64_t)((pp.rk.bits + 7) / 8));
    launch(ctx, "bcx_counts", k_bcx_counts, dim3(grid_for(nb, BLOCK)), dim3(BLOCK), 0, nb, cb.dict.sb_vals, cb.dict.bsrc, cb.status,
           cb.tl, cb.key_off, bt, cnt);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, cnt, off, nb, true, off + nb);
    launch(ctx, "bcx_expand", k_bcx_expand, dim3(grid_for(nb, BLOCK)), dim3(BLOCK), 0, nb, n, (const uint32_t *)bt,
           (const uint32_t *)off, cb.key_off, cb.key_code, (const uint32_t *)cb.dict.rank, cb.tl, pp.rk, rbits, nbc, keys);
    const uint64_t *sk = radix_sort_keys(ctx, "rs_bcx", keys, nbc, rbits + 1, pp.rk.bits);
    launch(ctx, "bcx_cols", k_bcx_cols, dim3(grid_for(nbc, BLOCK)), dim3(BLOCK), 0, (uint32_t)nbc, sk,
           (uint64_t)((1ull << rbits) - 1), cb.bcs_exec, lw_in);
    scan<uint64_t, OpMax<uint64_t>>(ctx, lw_in, cb.bcs_lastw64, nbc, false);
}

// The sorted pairs of a batch: the permutation (entry -> input pair index) and what the column kernels have to know
// about the sort that made it. The mode itself is in the record's PairPlan.
struct PairSort {
    Sorted ps{ nullptr, nullptr };     // vals: the permutation [P + V2_ITEMS] (mode 4: written by the CFK gather, which
                                       // unpacks sp_m4); keys: the sorted composites (modes 0-2)
    const uint64_t *sp_m4 = nullptr;   // mode 4: the sorted packed keys, unpacked by the CFK gather
    int key_shift = 0;                 // modes 0-2: the composite's bits below the key
    uint32_t *seg_flag = nullptr;      // [P] segment-start flags
    bool flags_done = false;           // seg_flag is written (mode 3) or will be by the CFK gather (mode 4)
    bool tinfo_done = false;           // modes 3, 4: the txn records were written by the pair-key launch
};

// Pairs sorted by (key, TxnId rank) by the cheapest of five sorts (PairPlan::mode, stat keydeps.pair_sort_mode):
// a batch given in TxnId order needs no rank in the sort key, and a key code of few varying bits leaves room to pack
// the pair index (or the pair's txn and slot) into a keys-only sort.
// keys_only (modes 3 and 4, the dictionary still running on the side lane): the pair-key launch reads no rank and leaves
// the txn records to k_txn_info, which build_columns launches once the ranks are there.
static PairSort sort_pairs(acc_ctx *ctx, CfkBuild &cb, bool keys_only)
{
    const uint32_t n = cb.n;
    const size_t P = cb.P;
    const uint32_t *key_off = cb.key_off;
    const uint64_t *key_code = cb.key_code;
    const uint32_t *owner = cb.owner, *rank = cb.dict.rank;
    const int rbits = cb.dict.rbits;
    PairPlan &pp = cb.pp;   // rk, rbits, sb: pair_plan
    uint64_t *pkey = ctx->get<uint64_t>("pair_key", P);
    const unsigned gP = grid_for(P, BLOCK);
    PairSort s;
    s.seg_flag = ctx->get<uint32_t>("seg_flag", P);
    if (cb.dict.batch_sorted && pp.rk.bits <= 32) {
        // pair index order is already TxnId order within every key: a stable keys-only sort of (key << 32 | pair index),
        // 8 B per element; the segment flags pass unpacks the permutation. Mode 4 packs (owner, slot) instead of the
        // pair index and the CFK gather unpacks it (one random read of the owner's record per pair, which carries
        // key_off[owner] for the pair index)
        const bool m4 = bits_for((uint64_t)n - 1) + pp.sb <= 32;
        pp.mode = m4 ? 4 : 3;
        TxnInfoArgs ti;   // the txn records (k_txn_info) by the same launch: the ranks are final unless ties turn up
        if (!keys_only) { ti.n = n; ti.status = cb.status; ti.tl = cb.tl; ti.tinfo = cb.tinfo; ti.bigflag = cb.bigflag; }
        launch(ctx, "pair_keys", k_pair_keys, dim3(grid_for(std::max<size_t>(P, n), BLOCK)), dim3(BLOCK), 0, P, key_code,
               owner, key_off, rank, (const uint32_t *)nullptr, pp, 0, pkey, ti);
        s.tinfo_done = !keys_only;
        const uint64_t *sp = radix_sort_keys(ctx, "rs_pair", pkey, P, 32, pp.rk.bits);
        uint32_t *perm = ctx->get<uint32_t>("pair_perm", P + V2_ITEMS);
        if (m4) s.sp_m4 = sp;
        else launch(ctx, "seg_flags", k_seg_flags_packed, dim3(gP), dim3(BLOCK), 0, P, sp, s.seg_flag, perm, -1, key_off,
                    (uint32_t *)nullptr);
        s.ps = { nullptr, perm };
        s.flags_done = true;
    } else if (cb.dict.batch_sorted) {
        pp.mode = 0;   // pair index order is already TxnId order within every key: stable sort by key
        launch(ctx, "pair_keys", k_pair_keys, dim3(gP), dim3(BLOCK), 0, P, key_code, owner, key_off, rank,
               (const uint32_t *)nullptr, pp, 0, pkey, TxnInfoArgs{});
        s.ps = radix_sort(ctx, "rs_pair", pkey, nullptr, P, pp.rk.bits);
    } else if (pp.rk.bits + rbits <= 64) {
        pp.mode = 1;
        launch(ctx, "pair_keys", k_pair_keys, dim3(gP), dim3(BLOCK), 0, P, key_code, owner, key_off, rank,
               (const uint32_t *)nullptr, pp, 0, pkey, TxnInfoArgs{});
        s.ps = radix_sort(ctx, "rs_pair", pkey, nullptr, P, pp.rk.bits + rbits);
        s.key_shift = rbits;
    } else {
        pp.mode = 2;
        launch(ctx, "pair_keys", k_pair_keys, dim3(gP), dim3(BLOCK), 0, P, key_code, owner, key_off, rank,
               (const uint32_t *)nullptr, pp, 1, pkey, TxnInfoArgs{});
        Sorted byrank = radix_sort(ctx, "rs_pair_r", pkey, nullptr, P, rbits);
        launch(ctx, "pair_keys", k_pair_keys, dim3(gP), dim3(BLOCK), 0, P, key_code, owner, key_off, rank,
               (const uint32_t *)byrank.vals, pp, 0, pkey, TxnInfoArgs{});
        s.ps = radix_sort(ctx, "rs_pair", pkey, byrank.vals, P, pp.rk.bits);
    }
    return s;
}

// The rank-dependent columns of the CFK (txn records, the gather into (key, TxnId) order, tile counts, the run-based
// scan's column set), then the build's host sync: ctx->pinned receives the tile totals, g[4..6] as staged by
// k_v2_apply, and the bumped-query count. Run again when the deferred tie check finds the sorted-batch ranks invalid.
// lane_open (first run of a build that forked the side lane): the main stream waits for the ranks before the txn records.
// The lane stays open across the build's sync (acc_ctx::sync frees nothing meanwhile).
static void build_columns(acc_ctx *ctx, CfkBuild &cb, const PairSort &s, bool tinfo_done, bool lane_open)
{
    const uint32_t n = cb.n;
    const size_t P = cb.P;
    const uint32_t *rank = cb.dict.rank;
    const PairPlan &pp = cb.pp;
    const unsigned gP = grid_for(P, BLOCK);
    const uint32_t nt = (uint32_t)((P + V2_TILE - 1) / V2_TILE);
    uint4 *ptinfo = s.sp_m4 ? nullptr : ctx->get<uint4>("pair_tinfo", P);
    uint32_t *tile_sums = ctx->get<uint32_t>("v2_tile_sums", (size_t)NCNT * nt);
    uint32_t *tile_pref = ctx->get<uint32_t>("v2_tile_pref", (size_t)NCNT * nt);
    uint32_t *totals = ctx->get<uint32_t>("v2_totals", 16);
    uint64_t rk_mask = 0;   // the bits the key compaction keeps (k_v2_apply rebuilds segment key codes from them)
    for (int r = 0; r < pp.rk.n; ++r) rk_mask |= (pp.rk.len[r] >= 64 ? ~0ull : ((1ull << pp.rk.len[r]) - 1)) << pp.rk.lo[r];
    if (lane_open) ctx->lane_wait();
    if (!tinfo_done)
        launch(ctx, "txn_info", k_txn_info, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, rank, cb.status, cb.tl, cb.key_off,
               cb.tinfo, cb.bigflag);
    if (!s.sp_m4)
        launch(ctx, "pair_tinfo", k_pair_tinfo, dim3(gP), dim3(BLOCK), 0, P, (const uint32_t *)cb.owner, (const uint4 *)cb.tinfo,
               ptinfo);
    launch(ctx, "cfk_gather", k_cfk_gather4, dim3(nt), dim3(BLOCK), 0, P, s.ps.vals, (const uint4 *)ptinfo, s.sp_m4, pp.sb,
           (const uint4 *)cb.tinfo, s.seg_flag, cb.s_rank, cb.s_exec, cb.s_info,
           cb.opts.seg_keys ? cb.pair_pos : (uint32_t *)nullptr, tile_sums, nt);
    launch(ctx, "v2_tile_scans", k_v2_tile_scans, dim3(NCNT), dim3(BLOCK), 0, (const uint32_t *)tile_sums, tile_pref, nt, totals);
    launch(ctx, "v2_apply", k_v2_apply, dim3(nt), dim3(BLOCK), 0, P, (const uint32_t *)cb.s_rank, (const uint32_t *)cb.s_exec,
           (const uint8_t *)cb.s_info, (const uint32_t *)s.seg_flag, (const uint32_t *)tile_pref, (const uint32_t *)totals, nt,
           cb.dict.rbits, cb.cols, cb.seg_incl, cb.seg_start, (const uint32_t *)s.ps.vals, cb.key_code, cb.seg_key, s.sp_m4,
           pp.rk, rk_mask, cb.bases, cb.tot, 4u, cb.gstat, (uint32_t)GSTAT_N, (const uint64_t *)cb.g,
           reinterpret_cast<uint64_t *>(totals) + 4);
    ACC_HIP(hipMemcpyAsync(ctx->pinned, totals, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
}

// pair_pos on demand, for the consumers that address pairs by index (exact replay, the global write tier) when the
// build was not asked for it
static void need_pair_pos(acc_ctx *ctx, CfkBuild &cb)
{
    if (cb.have_pair_pos) return;
    launch(ctx, "pair_pos", k_pair_pos, dim3(grid_for(cb.P, BLOCK)), dim3(BLOCK), 0, cb.P, (const uint32_t *)cb.perm, cb.pair_pos);
    cb.have_pair_pos = true;
}

// Stage 1: the CommandsForKey of a batch. Argument checks, staged inputs, prep and dictionary (dictionary.hip), the pair
// sort, the columns, and the build's host sync, at which validation errors and executeAt ties are known.
CfkBuild build_cfk(acc_ctx *ctx, const acc_batch_in *in, CfkOpts opts)
{
    if (!in) fail(ACC_E_ARG, "null argument");
    if (in->mem != ACC_MEM_HOST && in->mem != ACC_MEM_DEVICE) fail(ACC_E_ARG, "mem must be ACC_MEM_HOST or ACC_MEM_DEVICE");
    CfkBuild cb;
    cb.opts = opts;
    const uint32_t n = cb.n = in->n_txn;
    const size_t P = cb.P = (size_t)in->n_pairs;
    if (P >= 0xFFFFFFFFull) fail(ACC_E_ARG, "n_pairs must be < 2^32");
    hipStream_t st = ctx->stream;
    ctx->kd_valid = false;

    // ---- stage inputs
    cb.key_off = stage_in(ctx, "in_key_off", in->key_off, (size_t)n + 1, in->mem);
    if (n == 0 || P == 0) {
        // no pairs: every txn has KeyDeps.NONE
        uint64_t *arena_off = ctx->get<uint64_t>("arena_off", (size_t)n + 1);
        uint64_t *kd_off = ctx->get<uint64_t>("kd_off", (size_t)n + 1);
        uint64_t *u_off = ctx->get<uint64_t>("u_off", (size_t)n + 1);
        ACC_HIP(hipMemsetAsync(arena_off, 0, ((size_t)n + 1) * 8, st));
        ACC_HIP(hipMemsetAsync(kd_off, 0, ((size_t)n + 1) * 8, st));
        ACC_HIP(hipMemsetAsync(u_off, 0, ((size_t)n + 1) * 8, st));
        ctx->kd_view = acc_keydeps_view{ n, 0, 0, 0, 0, arena_off, ctx->get<int32_t>("arena", 1), kd_off,
                                         ctx->get<uint32_t>("key_idx", 1), u_off, ctx->get<uint32_t>("dep_txn", 1) };
        ctx->kd_valid = true;
        ctx->sync();
        return cb;
    }
    cb.tm = stage_in(ctx, "in_tm", in->txn_id.msb, n, in->mem);
    cb.tl = stage_in(ctx, "in_tl", in->txn_id.lsb, n, in->mem);
    cb.tn = stage_in(ctx, "in_tn", in->txn_id.node, n, in->mem);
    cb.em = stage_in(ctx, "in_em", in->execute_at.msb, n, in->mem);
    cb.el = stage_in(ctx, "in_el", in->execute_at.lsb, n, in->mem);
    cb.en = stage_in(ctx, "in_en", in->execute_at.node, n, in->mem);
    cb.status = stage_in(ctx, "in_status", in->status, n, in->mem);
    cb.key_code = stage_in(ctx, "in_key_code", in->key_code, P, in->mem);

    // ---- prep + dictionary
    cb.g = ctx->get<uint64_t>("g", PREP_G_WORDS);
    cb.owner = ctx->get<uint32_t>("owner", P);
    // the sorted-batch dictionary's tie check is read at the columns' sync below (one host sync fewer)
    prep_batch(ctx, n, P, cb.tm, cb.tl, cb.tn, cb.em, cb.el, cb.en, cb.status, cb.key_off, cb.key_code, cb.owner, cb.g, cb.dict);
    // A TxnId-ordered batch whose pair sort packs its keys (modes 3, 4) reads no rank until the txn records are written:
    // the sorted-batch dictionary, and behind it the bumped committed order made from the txn side, run on the side lane
    // (aux[0]) while the context stream sorts the pairs. The main stream waits for the ranks in build_columns; the lane
    // itself is still open when build_cfk returns and is joined by whoever comes next (keydeps_runs ahead of its count
    // pass, keydeps_of ahead of the replay, cfk_snapshot, the tie branch below), so its tail runs under the build's host
    // sync. A failure in between leaves the lane to acc_ctx::recover. Every other case keeps one stream.
    const bool overlap = pair_plan(cb) && cb.dict.fast_ok && cb.pp.rk.bits + cb.dict.rbits + 1 <= 64;
    ctx->stat("keydeps.build_overlap", overlap ? 1 : 0);
    ctx->stat("keydeps.bc_sort_passes", 0);
    ctx->stat("keydeps.stream_ahead", 0);   // (set by keydeps_runs: the replay path has no stream pass)
    ctx->stat("keydeps.stream_ahead_redo", 0);
    if (overlap) ctx->lane_fork();
    else build_dictionary(ctx, n, cb.tm, cb.tl, cb.tn, cb.em, cb.el, cb.en, cb.g, cb.dict, true);

    // ---- pairs sorted by (key, TxnId rank)
    cb.tinfo = ctx->get<uint4>("tinfo", n);
    cb.bigflag = ctx->get<uint32_t>("v3_bigflag", n);
    const PairSort ps = sort_pairs(ctx, cb, overlap);
    if (overlap) {
        // (enqueued after the pair sort: the context stream's long kernels are not held up by the lane's many launches)
        ctx->launch_stream = ctx->aux[0];
        build_dictionary(ctx, n, cb.tm, cb.tl, cb.tn, cb.em, cb.el, cb.en, cb.g, cb.dict, true);
        ctx->lane_mark();   // the ranks
        bc_from_txns(ctx, cb);
        ctx->launch_stream = nullptr;
    }
    cb.perm = ps.ps.vals;
    if (!ps.flags_done)
        launch(ctx, "seg_flags", k_seg_flags, dim3(grid_for(P, BLOCK)), dim3(BLOCK), 0, P, (const uint64_t *)ps.ps.keys,
               ps.key_shift, ps.seg_flag);

    // ---- the columns: one segment per key = CommandsForKey.txns, and the run-based scan's structures (class lists,
    // prefix counts, bumped committed list)
    cb.seg_incl = ctx->get<uint32_t>("seg_incl", P + V2_ITEMS);   // written by k_v2_apply (the multi-scan's column 8)
    cb.seg_start = ctx->get<uint32_t>("seg_start", P + 1);
    cb.seg_key = opts.seg_keys ? ctx->get<uint64_t>("seg_key", P + 1) : nullptr;   // per segment its key code
    cb.s_rank = ctx->get<uint32_t>("s_rank", P + V2_ITEMS);   // padded for the 16-B column loads
    cb.s_exec = ctx->get<uint32_t>("s_exec", P + V2_ITEMS);
    cb.s_info = ctx->get<uint8_t>("s_info", P + V2_ITEMS);
    cb.pair_pos = ctx->get<uint32_t>("pair_pos", P);
    cb.have_pair_pos = opts.seg_keys;   // written by the CFK gather when asked for
    cb.bases = ctx->get<uint32_t>("v2_bases", 16);
    cb.cols.rdir = ctx->get<uint4>("v2_rdir", 4 * (P / RD_W + 1));
    cb.cols.list_rank = ctx->get<uint32_t>("v2_list_rank", P);
    cb.cols.bc_rank = ctx->get<uint32_t>("v2_bc_rank", P);
    cb.cols.bc_exec = ctx->get<uint32_t>("v2_bc_exec", P);
    cb.cols.bc_kind = ctx->get<uint8_t>("v2_bc_kind", P);
    cb.cols.bc_pm_in = ctx->get<uint64_t>("v2_bc_pm_in", P);
    cb.cols.bc_key = cb.bc_side ? nullptr : ctx->get<uint64_t>("v2_bc_key", P);
    // the count / mark passes' accumulators, zeroed by the column kernels (txn records, k_v2_apply); bigflag above
    cb.tot = ctx->get<uint64_t>("v3_tot", 4);   // E, stream txns with a run record << 32 | big txns, a 9-16-key big txn
    cb.gstat = ctx->get<uint64_t>("v2_gstat", GSTAT_N + 6);   // + the batch totals and E / big counts (k_v3_ucompact)
    build_columns(ctx, cb, ps, ps.tinfo_done, overlap);
    if (cb.dict.ties_pending && ctx->pinned[6]) {
        // an executeAt equals another timestamp: the sorted-batch ranks are not dense ranks; the general dictionary,
        // then the rank-dependent columns again (the pair order does not depend on ranks in a sorted batch)
        check_errors(ctx->pinned[4]);
        ctx->lane_join();   // the general dictionary rewrites the ranks the lane reads, and reuses its scan and sort words
        redo_general_dictionary(ctx, n, cb.tm, cb.tl, cb.tn, cb.em, cb.el, cb.en, cb.g, cb.dict);
        if (cb.bc_side) {
            // the lane's list was made with the sorted-batch ranks: not used. The batch takes the replay path if the general dictionary finds the tie too, else keydeps_runs
            // sorts cols.bc_key as written with the new ranks.
            cb.bc_side = false;
            cb.cols.bc_key = ctx->get<uint64_t>("v2_bc_key", P);
            ctx->stat("keydeps.bc_sort_passes", 0);
        }
        build_columns(ctx, cb, ps, false, false);
    }
    cb.dict.ties_pending = false;
    memcpy(cb.htot, ctx->pinned, sizeof cb.htot);
    check_errors(ctx->pinned[4]);
    cb.ties = ctx->pinned[6] != 0;
    // the two predicates of "bumped committed" (per txn in the prep pass, per position in the columns) must agree
    if (cb.bc_side && !cb.ties && (uint64_t)cb.htot[6] != cb.dict.nbc)
        fail(ACC_E_STATE, "internal: bumped committed count of the prep pass differs from the columns'");
    ctx->stat("keydeps.path_replay", cb.ties || (ctx->flags & ACC_OPT_FORCE_REPLAY) ? 1 : 0);
    ctx->stat("keydeps.exec_ties", cb.ties ? 1 : 0);
    ctx->stat("keydeps.batch_sorted", cb.dict.batch_sorted ? 1 : 0);
    ctx->stat("keydeps.pair_sort_mode", (uint64_t)cb.pp.mode);
    cb.cfk = true;
    return cb;
}

// The run-based path's global fallback, for the nfb txns (efb raw entries) the tiers listed in wo.fb_list. The caller
// runs the TxnId compaction again afterwards.
static void global_fallback(acc_ctx *ctx, CfkBuild &cb, const V2View &vv, const V2Out &wo, uint64_t nfb, uint64_t efb)
{
    hipStream_t st = ctx->stream;
    const int rbits = cb.dict.rbits;
    const uint32_t *key_off = cb.key_off, *txn_of_rank = cb.dict.txn_of_rank, *fb_list = wo.fb_list, *vcnz = wo.cnz;
    const uint64_t *vdep_off = wo.dep_off, *arena_off = wo.arena_off;
    uint32_t *const dep_scr = wo.dep_scratch;
    uint64_t *const u_cnt = wo.u_cnt;
    int32_t *const arena = wo.arena;
    need_pair_pos(ctx, cb);
    uint64_t *vcnt = ctx->get<uint64_t>("cnt", cb.P);
    // txns beyond the block tiers (> 64 keys, > HUGE_E raw entries, or ranks beyond 25 bits): gather to global
    // memory, sort by (txn, value, key) for the TxnId array and by (txn, key, value) for the arena order
    uint64_t *fb_e = ctx->get<uint64_t>("v2_fb_e", nfb);
    uint64_t *fb_off = ctx->get<uint64_t>("v2_fb_off", nfb + 1);
    uint64_t *fb_maxk = ctx->get<uint64_t>("v2_fb_maxk", 1);
    ACC_HIP(hipMemsetAsync(fb_maxk, 0, sizeof(uint64_t), st));
    launch(ctx, "v2_fb_sizes", k_fb_sizes, dim3(grid_for(nfb, BLOCK)), dim3(BLOCK), 0, (uint32_t)nfb,
           (const uint32_t *)fb_list, key_off, (const uint64_t *)vdep_off, fb_e, fb_maxk);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, fb_e, fb_off, nfb, true, fb_off + nfb);
    ACC_HIP(hipMemcpyAsync(ctx->pinned, fb_maxk, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ctx->sync();
    const int bbits = bits_for(nfb - 1);
    const int kbits = std::max(1, bits_for(ctx->pinned[0] - 1));   // key index within its txn
    if (bbits + rbits + kbits > 64) fail(ACC_E_CAP, "too many oversized txns for the global KeyDeps path");
    uint64_t *gkey = ctx->get<uint64_t>("v2_gkey", efb);
    launch(ctx, "v2_big_gather", k_v2_big_gather, dim3((unsigned)((nfb + WAVES - 1) / WAVES)), dim3(BLOCK), 0,
           (uint32_t)nfb, (const uint32_t *)fb_list, (const uint64_t *)fb_off, vv, (const uint64_t *)vcnt, key_off,
           rbits, kbits, gkey);
    Sorted s1 = radix_sort(ctx, "rs_big1", gkey, nullptr, efb, bbits + rbits + kbits);
    uint32_t *nflag = ctx->get<uint32_t>("v2_big_nflag", efb);
    uint32_t *nincl = ctx->get<uint32_t>("v2_big_nincl", efb);
    launch(ctx, "v2_big_newflag", k_v2_big_newflag, dim3(grid_for(efb, BLOCK)), dim3(BLOCK), 0, efb,
           (const uint64_t *)s1.keys, kbits, nflag);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, nflag, nincl, efb, false);
    uint32_t *idx1 = ctx->get<uint32_t>("v2_big_idx1", efb);
    uint64_t *key2 = ctx->get<uint64_t>("v2_big_key2", efb);
    launch(ctx, "v2_big_rank", k_v2_big_rank, dim3(grid_for(efb, BLOCK)), dim3(BLOCK), 0, efb, (const uint64_t *)s1.keys,
           (const uint32_t *)nincl, (const uint32_t *)fb_list, (const uint64_t *)fb_off, rbits, kbits, key_off,
           (const uint64_t *)vdep_off, (const uint32_t *)txn_of_rank, dep_scr, u_cnt, idx1, key2);
    Sorted s2 = radix_sort(ctx, "rs_big2", key2, nullptr, efb, bbits + kbits + rbits);
    launch(ctx, "v2_big_arena", k_v2_big_arena, dim3(grid_for(efb, BLOCK)), dim3(BLOCK), 0, efb,
           (const uint32_t *)s2.vals, (const uint64_t *)s2.keys, (const uint32_t *)idx1, (const uint32_t *)fb_list,
           (const uint64_t *)fb_off, rbits, kbits, key_off, (const uint32_t *)vcnz, (const uint64_t *)arena_off, arena);
}

// Stage 2 of a batch without executeAt ties: the run-based path. The bumped committed entries sorted by (segment,
// executeAt); the count pass (one record per pair, E); the mark pass and the scans that size the result and split the
// txns into stream txns and big txns; the big txns' tiers on a side stream while the stream passes run; the TxnId
// compaction (finish), with the sorting tiers and the global fallback behind it for what the first round passed on.
static void keydeps_runs(acc_ctx *ctx, CfkBuild &cb, acc_keydeps_view *view)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = cb.n;
    const size_t P = cb.P;
    const unsigned gP = grid_for(P, BLOCK);
    const int rbits = cb.dict.rbits, segbits = bits_for(P);
    const uint32_t *key_off = cb.key_off, *owner = cb.owner, *txn_of_rank = cb.dict.txn_of_rank;
    const V2Cols &cols = cb.cols;
    uint32_t *const bigflag = cb.bigflag;
    uint64_t *const tot = cb.tot, *const gstat = cb.gstat;
    const uint32_t nbc = cb.htot[6];
    uint32_t *bcs_exec = cb.bcs_exec;
    uint64_t *bcs_lw64 = cb.bcs_lastw64;
    uint64_t *bc_pm64 = ctx->get<uint64_t>("v2_bc_pm64", nbc);
    if (cb.bc_side) {
        // the build made the (segment, executeAt) order on its side lane: only the segmented executeAt maximum over
        // the position-ordered list is left. The count pass reads the lane's bcs_exec / bcs_lastw: the join goes first,
        // so the cross-stream wait is served while the stream is idle behind the build's sync and the count pass
        // follows the scan without a bubble.
        ctx->lane_join();
        scan<uint64_t, OpMax<uint64_t>>(ctx, cols.bc_pm_in, bc_pm64, nbc, false);
    } else {
        ctx->lane_join();   // (no lane is open here: a build that forked one either kept bc_side or joined at its tie branch)
        if (segbits + rbits > 64) fail(ACC_E_ARG, "batch too large for the (segment, executeAt) composite key");
        if (!cols.bc_key) fail(ACC_E_STATE, "internal: no bumped committed sort keys");
        Sorted bcs = radix_sort(ctx, "rs_bc", cols.bc_key, nullptr, nbc, segbits + rbits);
        ctx->stat("keydeps.bc_sort_passes", nbc ? (uint64_t)((segbits + rbits + 7) / 8) : 0);
        bcs_exec = ctx->get<uint32_t>("v2_bcs_exec", nbc);
        uint64_t *bcs_lw_in = ctx->get<uint64_t>("v2_bcs_lw_in64", nbc);
        bcs_lw64 = ctx->get<uint64_t>("v2_bcs_lastw64", nbc);
        launch(ctx, "v2_bcs_cols", k_v2_bcs_cols, dim3(grid_for(nbc, BLOCK)), dim3(BLOCK), 0, nbc, (const uint64_t *)bcs.keys,
               (const uint32_t *)bcs.vals, (const uint8_t *)cols.bc_kind, (uint64_t)((1ull << rbits) - 1), bcs_exec, bcs_lw_in);
        // nearest-Write index and the segmented executeAt maximum: two prefix maxima in one launch (read as low words)
        const uint64_t *si[2] = { bcs_lw_in, cols.bc_pm_in };
        uint64_t *so[2] = { bcs_lw64, bc_pm64 };
        const size_t sn[2] = { nbc, nbc };
        scan_multi<uint64_t, OpMax<uint64_t>>(ctx, 2, si, so, sn, false, (uint64_t *const *)nullptr);
    }

    V2View vv{};
    vv.perm = cb.perm; vv.pair_pos = cb.pair_pos; vv.seg_incl = cb.seg_incl; vv.seg_start = cb.seg_start;
    vv.s_rank = cb.s_rank; vv.s_exec = cb.s_exec; vv.s_info = cb.s_info; vv.rdir = cols.rdir; vv.tinfo = cb.tinfo;
    vv.list_rank = cols.list_rank; vv.bases = cb.bases; vv.bc_rank = cols.bc_rank; vv.bc_exec = cols.bc_exec; vv.bc_pm = bc_pm64;
    vv.bc_kind = cols.bc_kind; vv.bcs_exec = bcs_exec; vv.bcs_lastw = bcs_lw64;
    // ---- count pass: per-pair records, big-txn flags, E
    if (P >= 0x80000000ull) fail(ACC_E_CAP, "n_pairs must be < 2^31 (count-pass record format)");
    RecOut ro;
    ro.rec = ctx->get<uint4>("v2_rec", 4 * P);
    ro.irec = ctx->get<uint4>("v2_irec", 2 * P);
    uint4 *rec = ro.rec;
    vv.irec32 = reinterpret_cast<const uint32_t *>(ro.irec);
    vv.rec = ro.rec;

    uint64_t *blk_e = ctx->get<uint64_t>("v3_blk_e", gP);
    uint32_t *psz = ctx->get<uint32_t>("v3_psz", P);   // the big txns' per-pair entry counts (mark pass -> bigfill)
#ifdef ACC_PHASE_PROF
    const size_t ct_rows = (size_t)gP * WAVES;
    unsigned long long *ct_buf = prof_arm(ctx, "v2_ct_prof", HIP_SYMBOL(g_ct_prof), 8 * ct_rows, st);
#endif
    launch(ctx, "v2_count", k_v2_count, dim3(gP), dim3(BLOCK), 0, P, vv, (const uint32_t *)owner, ro, bigflag, blk_e);
#ifdef ACC_PHASE_PROF
    {
        const std::vector<unsigned long long> h = prof_read(ct_buf, 8 * ct_rows, st);
        double sum[8] = {}, mx[3] = {};
        size_t w = 0;
        for (size_t r = 0; r < ct_rows; ++r) {
            if (!(h[8 * r + 7] >> 32)) continue;
            ++w;
            for (int i = 0; i < 7; ++i) sum[i] += (double)h[8 * r + i];
            sum[7] += (double)(h[8 * r + 7] & 0xFFFFFFFFu);
            for (int i = 0; i < 3; ++i) mx[i] = std::max(mx[i], (double)h[8 * r + i]);
        }
        const double d = w ? (double)w : 1.0;
        fprintf(stderr, "[ct_phase] waves=%zu avg cycles: query %.0f r3count %.0f inline+write %.0f | max %.0f %.0f %.0f | "
                "per pair: bumped %.4f seg-with-bc %.4f posM-search %.4f r3-candidates %.3f run-records %.4f\n",
                w, sum[0] / d, sum[1] / d, sum[2] / d, mx[0], mx[1], mx[2], sum[3] / P, sum[4] / P, sum[5] / P, sum[6] / P,
                sum[7] / P);
    }
#endif
    const uint32_t raw_cap = ST_RAW;
    uint64_t *kd_off = ctx->get<uint64_t>("kd_off", (size_t)n + 1);
    uint64_t *arena_off = ctx->get<uint64_t>("arena_off", (size_t)n + 1);
    uint64_t *szA = ctx->get<uint64_t>("v3_szA", n), *szK = ctx->get<uint64_t>("v3_szK", n);
    uint64_t *eb = ctx->get<uint64_t>("v3_eb", n), *dB = ctx->get<uint64_t>("v3_dB", (size_t)n + 1);
    // the two list flags of a txn as one word: its halves are the big txns' and the run-record stream txns' counts, each
    // below 2^30, so the sum stays below the scan's 2^62
    if (n >= (1u << 30)) fail(ACC_E_CAP, "n_txn must be < 2^30 (list flags scanned as one word)");
    uint64_t *flagw = ctx->get<uint64_t>("v3_flagw", n), *fpos = ctx->get<uint64_t>("v3_fpos", n);
    launch(ctx, "v3_mark", k_v3_mark, dim3(grid_for((size_t)n * MK_G, BLOCK)), dim3(BLOCK), 0, n, key_off,
           (const uint32_t *)ro.irec, (const uint4 *)rec, psz, raw_cap, bigflag, szA, szK, tot + 2, eb, flagw);
    uint64_t *blk_pre = ctx->get<uint64_t>("v3_blk_pre", gP);
    {   // arena / key offsets, the count pass's per-block entry totals, the big txns' TxnId scratch bases, the places in
        // the two txn lists: one launch. tot[1] = stream txns with a run record << 32 | big txns
        const uint64_t *si[5] = { szA, szK, blk_e, eb, flagw };
        uint64_t *so[5] = { arena_off, kd_off, blk_pre, dB, fpos };
        uint64_t *stot[5] = { arena_off + n, kd_off + n, tot, dB + n, tot + 1 };
        const size_t sn[5] = { n, n, gP, n, n };
        scan_multi<uint64_t, OpAdd<uint64_t>>(ctx, 5, si, so, sn, true, stot);
    }
    // the big-txn list in txn order (k_v3_bigfill's per-txn ranges abut: a big txn writes its end where the next
    // txn's first pair starts, equal values when the next txn is big too), and the stream txns with a run record, for
    // the RUNS stream pass
    uint32_t *blist = ctx->get<uint32_t>("v3_blist", n), *rlist = ctx->get<uint32_t>("v3_rlist", n);
    launch(ctx, "v3_lists", k_v3_lists, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, (const uint64_t *)flagw,
           (const uint64_t *)fpos, blist, rlist);
    // ---- E (dependency entries), the two list lengths and the 9-16-key flag reach the host here
    ACC_HIP(hipMemcpyAsync(ctx->pinned, tot, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ctx->read_mark();
    // The lean stream pass needs nothing of that read-back: its grid follows from n, its inputs are the size scan's
    // offsets, bigflag and the records. Only the arena's size, P + E, is not known yet. So where the context holds an
    // arena already, a leading share of the pass (ACC_AHEAD_DIV) is enqueued here, behind the copy, and runs while the
    // host waits for the sizes and enqueues the side-stream kernels; it reads E from tot[0] itself and leaves without a
    // store when P + E is beyond what the buffer holds (the host sees the same E below, grows the buffer and runs the
    // whole pass in its old place). The rest of the pass follows in its old place, behind the side-stream launches.
    const uint64_t arena_cap = ctx->buf_cap("arena") / sizeof(int32_t);
    bool ahead = arena_cap != 0 && !(ctx->flags & ACC_OPT_KD_NO_STREAM_AHEAD);
#ifdef ACC_PHASE_PROF
    ahead = false;   // the tuning build reads each pass's counter rows back behind it: the old order
#endif
    uint64_t *u_off = ctx->get<uint64_t>("u_off", (size_t)n + 1);
    uint64_t *u_cnt = ctx->get<uint64_t>("u_cnt", n);
    uint32_t *dep_st = ctx->get<uint32_t>("v3_dep_stream", (size_t)n * ST_SLOT);   // stream txns' TxnIds, slot t * ST_SLOT
    uint32_t *const key_idx = ctx->get<uint32_t>("key_idx", P);
    // ---- stream pass: the stream txns' KeyDeps (a grid over every txn, 16 lanes per txn), TxnIds to scratch;
    // 256-thread workgroups co-schedule best with the 512-thread block tier
    constexpr int st_nt = 256;
    const uint32_t tt = (uint32_t)st_nt / ST_G;
    const uint32_t nblocks = (n + tt - 1) / tt;
    const uint32_t ntiles = nblocks * (uint32_t)(st_nt / 64);   // waves (phase-profile rows)
    V3Stream sp;
    sp.v = vv; sp.err = gstat + 5;
    sp.key_off = key_off; sp.bigflag = bigflag; sp.list = nullptr; sp.txn_of_rank = txn_of_rank;
    sp.rec = rec; sp.irec = ro.irec;
    sp.arena_off = arena_off; sp.kd_off = kd_off; sp.u_cnt_out = u_cnt; sp.arena = nullptr; sp.key_idx = key_idx;
    sp.dep_scr = dep_st; sp.t0 = 0; sp.n = n; sp.ntiles = ntiles;
    sp.e_dev = nullptr; sp.pairs = P; sp.arena_cap = arena_cap;
    // the lean pass over the txns [t0, t0 + cnt), t0 a multiple of the tile
    auto lean_pass = [&](uint32_t t0, uint32_t cnt) {
        V3Stream a = sp;
        a.t0 = t0; a.n = cnt;
        const uint32_t nb = (cnt + tt - 1) / tt;
        if (rbits <= 28) launch(ctx, "v3_stream", k_v3_stream<uint32_t, st_nt, ST_G, ST_N2, false, false>, dim3(nb), dim3(st_nt), 0, a);
        else launch(ctx, "v3_stream", k_v3_stream<uint64_t, st_nt, ST_G, ST_N2, false, false>, dim3(nb), dim3(st_nt), 0, a);
    };
    const uint32_t n_ahead = ahead ? n / ACC_AHEAD_DIV / tt * tt : 0u;
    if (ahead) {
        sp.arena = static_cast<int32_t *>(const_cast<void *>(ctx->buf_ptr("arena")));
        sp.e_dev = tot;
        lean_pass(0, n_ahead);
    }
    ctx->read_wait();
    const uint64_t E = ctx->pinned[0];
    const uint32_t nbig = (uint32_t)(ctx->pinned[1] & 0xFFFFFFFFu);
    const uint32_t nrun = (uint32_t)(ctx->pinned[1] >> 32);
    const bool any16 = ctx->pinned[2] != 0;
    if (E >= 0xFFFFFFFFull) fail(ACC_E_CAP, "more than 2^32-1 dependency entries in one batch");
    const bool redo = ahead && P + E > arena_cap;
    if (redo) {
        // the guard tripped: no wave of the pass stored anything. The stream is drained before the arena is replaced,
        // and every pointer to it is taken again below.
        ctx->sync();
        ahead = false;
    }
    ctx->stat("keydeps.stream_ahead", ahead ? 1 : 0);
    ctx->stat("keydeps.stream_ahead_redo", redo ? 1 : 0);
    uint64_t *vdep_off = nullptr;
    uint32_t *dep_scr = nullptr;
    uint64_t nfb = 0, efb = 0, nmed = 0, nbig2 = 0;
    ctx->stat("keydeps.huge_txns", 0);
    V2Out wo{};
    bool win_ok = false;
#ifdef ACC_PHASE_PROF
    unsigned long long *win_buf = nullptr, *sr_buf = nullptr;
    size_t sr_rows = 0;
#endif
    uint64_t *vcnt = nullptr;
    uint32_t *med_list = nullptr, *big_list = nullptr, *fb_list = nullptr;
    // persistent write-tier grids: min(work, the tier's default, the cap in flags bits 16..31 when set (testing))
    const unsigned tgm = (ctx->flags >> ACC_OPT_TIER_GRID_SHIFT) ? (ctx->flags >> ACC_OPT_TIER_GRID_SHIFT) : ~0u;
    auto tier_grid = [&](unsigned work, unsigned dflt) { return dim3(std::max(1u, std::min(std::min(work, dflt), tgm))); };
    // the sorting tiers: medium (<= MED_CAP raw entries), block (<= BIG_E), huge (<= HUGE_E, fed by the block tier)
    auto sort_tiers = [&](bool with_med) {
        if (with_med)
            launch(ctx, "v2_write_med", k_v2_write_big<MED_CAP, BLOCK>, tier_grid(nbig, 2048), dim3(BLOCK), 0,
                   (const uint32_t *)med_list, vv, (const uint64_t *)vcnt, wo);
        launch(ctx, "v2_write_big", k_v2_write_big<BIG_E, 512>, tier_grid(nbig, 1024), dim3(512), 0,
               (const uint32_t *)big_list, vv, (const uint64_t *)vcnt, wo);
        launch(ctx, "v2_write_huge", k_v2_write_big<HUGE_E, 1024>, tier_grid(nbig, 64), dim3(1024), 0,
               (const uint32_t *)wo.huge_list, vv, (const uint64_t *)vcnt, wo);
    };
    int32_t *const arena = ctx->get<int32_t>("arena", P + E);   // (ahead: it fits, the buffer the lean pass writes)
    sp.arena = arena; sp.e_dev = nullptr;
    uint32_t *const dep_txn = ctx->get<uint32_t>("dep_txn", std::max<uint64_t>(E, 1));
    // ---- big txns' arena / keys into place, TxnId offsets and compaction. With global-path txns (known only after
    // the tiers ran) this is redone once they are written, so the common case pays one host sync here.
    auto finish = [&]() {
        scan<uint64_t, OpAdd<uint64_t>>(ctx, u_cnt, u_off, n, true, u_off + n);
        const uint32_t *tmap = nullptr, *ne_cnt = nullptr;
        const uint64_t *uo = u_off;
        if (cb.opts.sparse) {
            uint32_t *flag = ctx->get<uint32_t>("v3_ne_flag", n), *pos = ctx->get<uint32_t>("v3_ne_pos", n);
            uint32_t *cnt = ctx->get<uint32_t>("v3_ne_cnt", 1), *ne_t = ctx->get<uint32_t>("v3_ne_t", n);
            uint64_t *ne_uoff = ctx->get<uint64_t>("v3_ne_uoff", (size_t)n + 1);
            launch(ctx, "v3_neflag", k_v3_neflag, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, (const uint64_t *)u_cnt, flag);
            scan<uint32_t, OpAdd<uint32_t>>(ctx, flag, pos, n, true, cnt);
            launch(ctx, "v3_nelist", k_v3_nelist, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, (const uint32_t *)flag,
                   (const uint32_t *)pos, (const uint32_t *)cnt, (const uint64_t *)u_off, ne_t, ne_uoff);
            tmap = ne_t; ne_cnt = cnt; uo = ne_uoff;
        }
        launch(ctx, "v3_ucompact", k_v3_ucompact, dim3((unsigned)((E + UC_CHUNK - 1) / UC_CHUNK) + 1), dim3(BLOCK), 0, n,
               uo, (const uint64_t *)arena_off, (const uint64_t *)kd_off, (const uint32_t *)bigflag, key_off,
               (const uint64_t *)vdep_off, (const uint32_t *)dep_st, (const uint32_t *)dep_scr,
               tmap, ne_cnt, dep_txn, (const uint64_t *)u_off, gstat + GSTAT_N);
        ACC_HIP(hipMemcpyAsync(ctx->pinned, gstat, (GSTAT_N + 6) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        ctx->sync();
    };
    // Side streams: aux[0] the big txns' tiers, aux[1] the RUNS stream pass. With the lean pass ahead they rest on the
    // read-back's event, not on the context stream's tail (fork would queue them behind the lean pass), and routing and
    // bigfill go to aux[0] too.
    const int nside = nrun ? 2 : nbig ? 1 : 0;
    if (ahead) ctx->fork_at_read(nside);
    // ---- big txns: v2 tiers, headers / key indices / entries into the final arrays, TxnIds into scratch
    if (nbig) {
        const unsigned gB = (nbig + WAVES - 1) / WAVES;
        vdep_off = ctx->get<uint64_t>("dep_off", P + 1);
        vcnt = ctx->get<uint64_t>("cnt", P);
        uint32_t *vcnz = ctx->get<uint32_t>("cnz", P + 1);
        dep_scr = ctx->get<uint32_t>("v2_dep_scratch", std::max<uint64_t>(E, 1));
        med_list = ctx->get<uint32_t>("v2_med_list", nbig);
        big_list = ctx->get<uint32_t>("v2_big_list", nbig);
        fb_list = ctx->get<uint32_t>("v2_fb_list", nbig);
        V3Big bg;
        bg.blist = blist; bg.key_off = key_off; bg.psz = psz; bg.dB = dB; bg.arena_off = arena_off; bg.kd_off = kd_off;
        bg.vdep_off = vdep_off; bg.vcnt = vcnt; bg.vcnz = vcnz; bg.u_cnt = u_cnt; bg.arena = arena; bg.key_idx = key_idx;
        const bool big_ok = rbits + 6 <= 31;
        win_ok = big_ok && !(ctx->flags & ACC_OPT_NO_WINDOW_TIER);   // (testing: the sorting tiers instead)
        if (ahead) ctx->launch_stream = ctx->aux[0];
        launch(ctx, "v3_route", k_v3_route, dim3(grid_for(nbig, BLOCK)), dim3(BLOCK), 0, nbig, (const uint32_t *)blist,
               key_off, (const uint64_t *)eb, (int)big_ok, (int)win_ok, med_list, big_list, fb_list,
               ctx->get<uint32_t>("v2_w8_list", nbig), ctx->get<uint32_t>("v2_w16_list", nbig), gstat);
        launch(ctx, "v3_bigfill", k_v3_bigfill, dim3(gB), dim3(BLOCK), 0, nbig, bg);
        if (ahead) {
            // The tier's first kernel is next in its queue behind bigfill; the stream passes become ready at the same
            // point but across queues, so the tier's blocks are placed first, as they were when the context stream
            // ran bigfill ahead of the fork (placed behind the stream passes' blocks the tier ran 0.66 against 0.56 ms).
            ctx->lane_mark();
            ctx->lane_wait();
            if (nrun) ACC_HIP(hipStreamWaitEvent(ctx->aux[1], ctx->lane_ev, 0));
        }
        wo.key_off = key_off; wo.dep_off = vdep_off; wo.arena_off = arena_off; wo.cnz = vcnz; wo.txn_of_rank = txn_of_rank;
        wo.arena = arena; wo.dep_scratch = dep_scr; wo.u_cnt = u_cnt; wo.gstat = gstat;
        wo.rec = rec; wo.irec32 = vv.irec32; wo.med_list = med_list; wo.big_list = big_list; wo.fb_list = fb_list;
        wo.huge_list = ctx->get<uint32_t>("v2_huge_list", nbig);
        // persistent grids over device-side list counts (routing happened after the last host sync); the tiers run on a
        // side stream, concurrently with the stream passes
        if (!ahead) ctx->fork(nside);
        ctx->launch_stream = ctx->aux[0];
        if (win_ok) {
#ifdef ACC_PHASE_PROF
            win_buf = prof_arm(ctx, "v2_win_prof", HIP_SYMBOL(g_win_prof), 10, ctx->aux[0]);
#endif
            // the window tier takes every big txn of <= 16 keys; the sorting tiers run after the next host sync, only
            // when it passed txns on or some txn has more keys (no launch without work)
            launch(ctx, "v2_write_win", k_v2_write_win<8>, tier_grid(nbig, 2048), dim3(BLOCK), 0,
                   (const uint32_t *)ctx->get<uint32_t>("v2_w8_list", nbig), (const uint64_t *)(gstat + 7), vv,
                   (const uint64_t *)vcnt, wo);
            // (> 8 keys is rare: a small persistent grid, launched only when the mark pass saw a big txn of 9-16 keys)
            if (any16)
                launch(ctx, "v2_write_win16", k_v2_write_win<16>, tier_grid(nbig, 256), dim3(BLOCK), 0,
                       (const uint32_t *)ctx->get<uint32_t>("v2_w16_list", nbig), (const uint64_t *)(gstat + 8), vv,
                       (const uint64_t *)vcnt, wo);
        } else if (big_ok) {
            sort_tiers(true);
        } else {
            // ranks beyond 25 bits: u64 records in the wave tier (k_v3_route sends everything else to the global path)
            launch(ctx, "v2_write_medium", k_v2_write_medium, tier_grid(gB, 2048), dim3(BLOCK), 0,
                   (const uint64_t *)gstat, (const uint32_t *)med_list, vv, (const uint64_t *)vcnt, wo);
        }
        ctx->launch_stream = nullptr;
    }
    {
        // ---- the stream passes (sp above)
#ifdef ACC_PHASE_PROF
        const size_t prof_rows = (size_t)ntiles;
        unsigned long long *prof_buf = prof_arm(ctx, "v3_prof", HIP_SYMBOL(g_st_prof), 8 * prof_rows, st);
#endif
        if (nrun) {
            // the stream txns with a run record on side stream 1, concurrently with the lean pass below (their gathers
            // kept out of the lean pass: registers and a wave-uniform loop in every wave that holds one; config 2: 25%
            // of the txns)
            if (!nbig && !ahead) ctx->fork(2);
            V3Stream sr = sp;
            sr.list = rlist; sr.n = nrun;
            const uint32_t rblocks = (nrun + tt - 1) / tt;
            ctx->launch_stream = ctx->aux[1];
#ifdef ACC_PHASE_PROF
            sr_rows = (size_t)rblocks * (st_nt / 64);
            sr_buf = prof_arm(ctx, "v3_sr_prof", HIP_SYMBOL(g_sr_prof), 8 * sr_rows, ctx->aux[1]);
#endif
            if (rbits <= 28) launch(ctx, "v3_stream_runs", k_v3_stream<uint32_t, st_nt, ST_G, ST_N2, true, true>, dim3(rblocks), dim3(st_nt), 0, sr);
            else launch(ctx, "v3_stream_runs", k_v3_stream<uint64_t, st_nt, ST_G, ST_N2, true, true>, dim3(rblocks), dim3(st_nt), 0, sr);
            ctx->launch_stream = nullptr;
        }
        // (ahead: the txns below n_ahead have been running since the size read-back was enqueued)
        lean_pass(ahead ? n_ahead : 0u, ahead ? n - n_ahead : n);
#ifdef ACC_PHASE_PROF
        {
            const std::vector<unsigned long long> h = prof_read(prof_buf, 8 * prof_rows, st);
            double sum[6] = {}, mx[6] = {};
            size_t w = 0;
            for (size_t r = 0; r < prof_rows; ++r) {
                if (!h[8 * r + 7]) continue;
                ++w;
                for (int i = 0; i < 6; ++i) { sum[i] += (double)h[8 * r + i]; mx[i] = std::max(mx[i], (double)h[8 * r + i]); }
            }
            const double d = w ? (double)w : 1.0;
            fprintf(stderr, "[st_phase] waves=%zu avg cycles: setup %.0f records %.0f gather %.0f sort %.0f emit-lds %.0f lookback+copy %.0f | max: %.0f %.0f %.0f %.0f %.0f %.0f\n",
                    w, sum[0] / d, sum[1] / d, sum[2] / d, sum[3] / d, sum[4] / d, sum[5] / d, mx[0], mx[1], mx[2], mx[3], mx[4], mx[5]);
        }
#endif
    }
    if (nside) ctx->join(nside);
#ifdef ACC_PHASE_PROF
    if (nbig && win_ok) {
        const std::vector<unsigned long long> h = prof_read(win_buf, 10, st);
        const double nt = h[6] ? (double)h[6] : 1.0;
        fprintf(stderr, "[win_phase] txns=%llu avg cycles per txn (thread 0 of each block): lowend %.0f gather %.0f "
                "union %.0f sort|prefix|below %.0f span-writes %.0f list-wait %.0f | avg E %.1f span words %.1f below %.1f\n",
                h[6], h[0] / nt, h[1] / nt, h[2] / nt, h[3] / nt, h[4] / nt, h[9] / nt, h[7] / nt,
                (double)(h[8] >> 32) / nt, (double)(h[8] & 0xFFFFFFFFull) / nt);
    }
#endif
#ifdef ACC_PHASE_PROF
    if (sr_buf) {
        const std::vector<unsigned long long> h = prof_read(sr_buf, 8 * sr_rows, st);
        double sum[6] = {};
        size_t w = 0;
        for (size_t r = 0; r < sr_rows; ++r) {
            if (!h[8 * r + 7]) continue;
            ++w;
            for (int i = 0; i < 6; ++i) sum[i] += (double)h[8 * r + i];
        }
        const double d = w ? (double)w : 1.0;
        fprintf(stderr, "[sr_phase] waves=%zu avg cycles: setup %.0f records %.0f gather %.0f sort %.0f emit-lds %.0f lookback+copy %.0f\n",
                w, sum[0] / d, sum[1] / d, sum[2] / d, sum[3] / d, sum[4] / d, sum[5] / d);
    }
#endif
    finish();
    if (ctx->pinned[5]) fail(ACC_E_STATE, "internal: stream gather count differs from the count pass");
    if (ctx->pinned[2]) fail(ACC_E_STATE, "internal: v2 gather count differs from the count pass");
    if (nbig && win_ok && (ctx->pinned[0] || ctx->pinned[1])) {
        // txns the window tier could not take (> 16 keys, or too many entries below its span): the sorting tiers now,
        // on the context stream, then the copies / compaction again
        sort_tiers(ctx->pinned[0] != 0);
        finish();
        if (ctx->pinned[2]) fail(ACC_E_STATE, "internal: v2 gather count differs from the count pass");
    }
    if (nbig) {
        nmed = ctx->pinned[0]; nbig2 = ctx->pinned[1];
        nfb = ctx->pinned[3]; efb = ctx->pinned[4];
        ctx->stat("keydeps.huge_txns", ctx->pinned[6]);
        ctx->stat("keydeps.window_txns", ctx->pinned[7] + ctx->pinned[8]);
    }
    if (nfb) {
        global_fallback(ctx, cb, vv, wo, nfb, efb);
        finish();
    }
    ctx->stat("keydeps.stream_txns", n - nbig);
    ctx->stat("keydeps.stream_run_txns", nrun);
    ctx->stat("keydeps.big_path_txns", nbig);
    ctx->stat("keydeps.medium_txns", nmed);
    ctx->stat("keydeps.big_txns", nbig2);
    ctx->stat("keydeps.fallback_txns", nfb);
    ctx->stat("keydeps.fallback_entries", efb);
    ctx->stat("keydeps.bumped_committed", nbc);
    *view = acc_keydeps_view{ n, ctx->pinned[GSTAT_N], ctx->pinned[GSTAT_N + 1], ctx->pinned[GSTAT_N + 2], E, arena_off,
                              arena, kd_off, key_idx, u_off, dep_txn };
    ctx->kd_view = *view;
    ctx->kd_valid = true;
}

// KeyDeps of a built batch: the exact replay (keydeps_replay.hip) when executeAt ties exist, where the FAST
// bisection's pick is order-dependent, or under ACC_OPT_FORCE_REPLAY; else the run-based path.
void keydeps_of(acc_ctx *ctx, CfkBuild &cb, acc_keydeps_view *view)
{
    if (!cb.cfk) {
        *view = ctx->kd_view;   // the empty result build_cfk left
    } else if (cb.ties || (ctx->flags & ACC_OPT_FORCE_REPLAY)) {
        ctx->lane_join();   // the build's side lane (its list is not used here; its buffers are, by later stages)
        need_pair_pos(ctx, cb);
        keydeps_replay(ctx, cb, view);
    } else {
        keydeps_runs(ctx, cb, view);
    }
}

void keydeps_batch(acc_ctx *ctx, const acc_batch_in *in, acc_keydeps_view *view)
{
    if (!in || !view) fail(ACC_E_ARG, "null argument");
    CfkBuild cb = build_cfk(ctx, in, CfkOpts{});
    keydeps_of(ctx, cb, view);
}

// ---------------------------------------------------------------- CFK snapshot for the other scans (recovery.hip)

uint32_t cfk_nseg(acc_ctx *ctx, const CfkBuild &cb)
{
    ACC_HIP(hipMemcpyAsync(ctx->pinned, cb.seg_incl + cb.P - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    return (uint32_t)(ctx->pinned[0] & 0xFFFFFFFFu);   // seg_incl = inclusive count of segment starts
}

CfkBuild cfk_snapshot(acc_ctx *ctx, const acc_batch_in *in)
{
    CfkOpts opts;
    opts.seg_keys = true;
    CfkBuild cb = build_cfk(ctx, in, opts);
    ctx->lane_join();   // the build's side lane: the snapshot's readers use the context stream only
    ctx->kd_valid = false;
    if (cb.cfk) cb.nseg = cfk_nseg(ctx, cb);
    return cb;
}

}  // namespace acc
