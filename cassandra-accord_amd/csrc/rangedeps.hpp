// rangedeps.hpp — what the RangeDeps translation units share (rangedeps.hip: prepare, stored-range dictionary and the
// driver; rangedeps_stab.hip: the queries and the stabbing pass; rangedeps_build.hip: the per-txn build and the
// compaction): the constants, the records the kernels take by value (QRec, View, Out), the record of one batch's
// pipeline (RdBuild) with its stage entry points. (The read-back of device scalars, ReadBack, is ctx.hpp's.)
#pragma once

#include "dict.hpp"

namespace acc {

namespace rd {

constexpr int RD_TS = 16;         // chunks of BLOCK txns per workgroup in the per-txn passes with global counters
constexpr int NCLS = 33;          // width classes 0..32 (4^32 = 2^64 covers every u64 width)
#ifndef ACC_RD_TILE
#define ACC_RD_TILE 256
#endif
constexpr int TILE = ACC_RD_TILE;   // entries per LDS tile in the stabbing pass (LDS per block sets the occupancy)
constexpr uint32_t BLOCK_E = 8192;  // workgroup tier (LDS)

__device__ __forceinline__ uint32_t width_class(uint64_t s, uint64_t e)
{
    const uint64_t w = e - s;                 // >= 1 after validation
    const uint32_t bits = w <= 1 ? 0u : 64u - (uint32_t)__builtin_clzll(w - 1);   // ceil(log2 w)
    return (bits + 1) >> 1;                   // w <= 4^class
}

__device__ __forceinline__ uint64_t class_width(uint32_t c) { return c >= 32 ? ~0ull : (1ull << (2 * c)); }

// query q: a key of a key txn (q < P) or a range of a range txn (q >= P); [lo, hi] its bounds
struct QRec {
    uint64_t lo, hi;
    uint32_t lim, tpos;
    uint32_t flags;   // witness mask | is-range << 8
    uint32_t q;
};

// what the stabbing kernels read and write (rangedeps_stab.hip)
struct View {
    uint32_t Q;
    int end_inclusive;
    const QRec *srec;             // queries sorted by low bound
    const uint64_t *cs_s, *cs_e;  // entries by (class, start)
    const uint2 *cs_info;         // (range id, TxnId position)
    const uint8_t *cs_kind;
    const uint32_t *class_off;    // [NCLS + 1]
    const uint32_t *win;          // per block: b0[NCLS], b1[NCLS] (k_rd_stab_win)
    const uint64_t *blo, *bhi;    // per block: lowest low bound, highest high bound of its queries
    uint64_t *cursor;             // global output cursor
    uint64_t cap;                 // capacity of ent
    uint64_t *ent;                // (range id << 32 | TxnId position) per emitted pair
    ulonglong2 *q_out;            // per query (original index): (first entry, entries), one 16-B store per query
};

// what the per-txn build and compaction kernels read and write (rangedeps_build.hip)
struct Out {
    uint32_t n, P;
    const uint32_t *key_off, *rng_off;
    const ulonglong2 *q_out;      // (first entry, entries) per query
    const uint64_t *ent;
    const uint32_t *txn_of_tpos;  // null: batch in TxnId order (tpos = batch index)
    const uint64_t *raw_off;      // [n + 1] raw entries per txn (scratch placement)
    uint32_t *s_arena, *s_rid, *s_dep;   // scratch at 2 raw_off / raw_off / raw_off
    uint32_t *rd_cnt, *u_cnt;
    uint64_t *a_cnt;
    const uint32_t *list;         // txns of the tier (build kernels)
    const uint64_t *glb_off;      // scratch offsets of the global tier (u64 elements)
    uint64_t *gscratch;
    // compaction
    const uint64_t *arena_off, *rd_off, *u_off;
    int32_t *arena;
    uint32_t *range_id, *dep_txn;
};

}  // namespace rd

// One batch's RangeDeps pipeline: rangedeps_batch sets the sizes, each stage fills its part in turn and only reads the
// parts before it. Device pointers are owned by the context and valid until its next compute call.
struct RdBuild {
    uint32_t n = 0, Q = 0;            // txns; queries = P + R
    uint32_t npos = 0;                // TxnId positions the entries name (0: n, the batch's own; rcmd.hip: the store's table)
    size_t P = 0, R = 0;              // key pairs, ranges
    int end_inclusive = 0;
    // ---- rd_prepare
    // staged inputs
    const uint32_t *key_off = nullptr, *rng_off = nullptr;
    const uint64_t *tm = nullptr, *tl = nullptr, *em = nullptr, *el = nullptr;
    const int32_t *tn = nullptr, *en = nullptr;
    const uint8_t *status = nullptr;
    const uint64_t *key_code = nullptr, *rs = nullptr, *re = nullptr;
    Dictionary dict;                  // the batch's own, or the KeyDeps half's (SharedDict)
    const uint32_t *owner = nullptr;  // [P] txn of every key pair
    uint4 *tinfo = nullptr;           // [n] {lim, tpos, witness mask, is range} (k_rd_txncols)
    uint32_t *txn_of_tpos = nullptr;  // [n] inverse of tpos
    uint64_t mask_s = 0, mask_e = 0, mask_lo = 0;   // OR-masks of range starts, ends and query low bounds (bit compaction)
    uint32_t *rowner = nullptr;       // [R] txn of every range
    uint32_t *eflag = nullptr;        // [R] 1: an entry (range of a non-erased range command)
    uint32_t *eidx = nullptr;         // [R + 1] exclusive scan of eflag
    uint32_t NE = 0;                  // entries
    // ---- rd_range_dict
    uint64_t *dict_s = nullptr, *dict_e = nullptr;   // [n_dict] stored ranges in Range::compare order (index = range id)
    uint32_t *dincl = nullptr;        // [NE + 1] inclusive scan of the dictionary flags; dincl[NE] = n_dict
    uint64_t *cs_s = nullptr, *cs_e = nullptr;       // [NE] entries by (class, start)
    uint2 *cs_info = nullptr;
    uint8_t *cs_kind = nullptr;
    uint32_t *class_off = nullptr;    // [NCLS + 1]
    // ---- rd_stab_queries
    rd::View v{};
    uint64_t E = 0;                   // raw (range id, TxnId position) pairs in v.ent
    uint32_t stab_passes = 0;         // 2: the first pass outgrew its capacity; 0: no queries
    // ---- rd_build_txns
    uint64_t *arena_off = nullptr, *rd_off = nullptr, *u_off = nullptr;   // [n + 1], allocated by rangedeps_batch
    rd::Out o{};
    uint32_t tier_txns[16] = {};      // txns per tier (k_rd_tsize)
    uint64_t block_txns = 0;          // txns of the LDS workgroup tiers
    uint64_t tot_arena = 0, tot_rd = 0, tot_u = 0;
    uint32_t n_dict = 0;
};

void rd_prepare(acc_ctx *ctx, const acc_range_batch_in *in, const SharedDict *shared, RdBuild &b);   // rangedeps.hip
void rd_range_dict(acc_ctx *ctx, RdBuild &b);                                                        // rangedeps.hip
void rd_stab_queries(acc_ctx *ctx, RdBuild &b);                                                      // rangedeps_stab.hip
void rd_build_txns(acc_ctx *ctx, RdBuild &b);                                                        // rangedeps_build.hip

}  // namespace acc
