// rcmd_partial.hpp — what rcmd.hip (the range-command store, its updates, prunes and queries) and rcmd_partial.hip
// (acc_rcmd_partial_rangedeps: the stab result with RedundantBefore.collectDeps' range deps) share: the store record,
// the union index it caches for the partial call, the staged queries, and the front end and tail of a query call.
#pragma once

#include "cfkredundant.hpp"
#include "rangedeps.hpp"

// The union index of acc_rcmd_partial_rangedeps (rcmd_partial.hip): the store's id table and dictionary merged with the
// bounds and the ranges of the RedundantBefore map's intervals whose bound is above TxnId.NONE, and the stabbing index's
// (range id, TxnId position) column renamed into both. Built lazily by the first partial call after the table or the
// map changed (valid == false); the arrays belong to the store.
struct acc_rcmd_union {
    bool valid = false;
    uint64_t builds = 0;              // index builds over the store's life (rcmd.union_builds)
    uint32_t live = 0;                // intervals with a bound above NONE (0: the partial call is acc_rcmd_rangedeps)
    uint32_t n_ids = 0, n_dict = 0;
    uint64_t *im = nullptr, *il = nullptr;      // [n_ids] the ids in compareTo order
    int32_t *in = nullptr;
    uint32_t *id_row = nullptr;                 // [n_ids] table row, or 0xFFFFFFFF
    uint64_t *dict_s = nullptr, *dict_e = nullptr;   // [n_dict] the union dictionary in Range::compare order
    uint2 *cs_info = nullptr;                   // [NE] the index's (range id, TxnId position) in union ids
    uint32_t *rowpos = nullptr;                 // [n + 1] union position of every row; rowpos[n] = n_ids
    uint32_t *ipos = nullptr, *irid = nullptr;  // [nv] per interval: union TxnId position and range id (NONE: no dep)
    uint32_t *ishare = nullptr;                 // [nv] 1: a non-erased row equal to the bound holds exactly Range(m)
    uint32_t *arange = nullptr;                 // [arange_n] 0, 1, ..: id_row of a store without a bound above NONE
    uint32_t arange_n = 0;
    size_t cap[12] = {};                        // bytes of the arrays above, in declaration order
};

struct acc_rcmd {
    int device = 0;
    uint32_t end_inclusive = 0;
    uint32_t n = 0;        // commands (table rows)
    uint32_t R = 0;        // ranges of the table
    uint32_t NE = 0;       // index entries = ranges of the non-erased commands
    uint32_t n_dict = 0;   // distinct stored ranges
    // the table
    uint64_t *tm = nullptr, *tl = nullptr;
    int32_t *tn = nullptr;
    uint8_t *flags = nullptr;
    uint32_t *rng_off = nullptr;
    uint64_t *rs = nullptr, *re = nullptr;
    // the state of each command (flags holds HAS_DEPS beside ERASED) and its deps, dep_off[n] = ND
    uint64_t ND = 0;
    uint64_t *em = nullptr, *el = nullptr;
    int32_t *en = nullptr;
    uint8_t *status = nullptr;
    uint32_t *dep_off = nullptr;
    uint64_t *dm = nullptr, *dl = nullptr;
    int32_t *dn = nullptr;
    uint64_t *ds = nullptr, *de = nullptr;
    uint8_t *dk = nullptr;
    // the index (rd_range_dict's arrays; class_off lies NCLS + 1 words into cls)
    uint64_t *dict_s = nullptr, *dict_e = nullptr;
    uint32_t *dincl = nullptr;
    uint64_t *cs_s = nullptr, *cs_e = nullptr;
    uint2 *cs_info = nullptr;
    uint8_t *cs_kind = nullptr;
    uint32_t *cls = nullptr;
    // byte sizes of the arrays above in declaration order (adopted from the context: they differ from the counts)
    size_t bytes[26] = {};
    // acc_rcmd_redundant_before: the store's RedundantBefore map (key code -> shardAppliedOrInvalidatedBefore), created
    // by the first accepted call
    acc_maxconflicts *rb = nullptr;
    // acc_rcmd_partial_rangedeps: invalidated by every call that rewrites the table or merges into the map
    acc_rcmd_union u;
};

namespace acc {

namespace rc {

struct Queries {
    uint32_t nq, P, R;
    const uint64_t *tm, *tl, *xm, *xl;
    const int32_t *tn, *xn;
    const uint32_t *key_off, *rng_off;
    const uint64_t *key, *rs, *re;
};

}  // namespace rc

// ---- rcmd.hip: the front end and the tail of acc_rcmd_rangedeps, as acc_rcmd_partial_rangedeps runs them
// mem, the bound type and the sizes; the build record of the queries (ctx->rd_valid cleared)
RdBuild rcmd_begin_rangedeps(acc_ctx *ctx, const acc_rcmd *store, const acc_cfk_mixed_queries *in);
// the queries staged, k_rc_qprep run over the store's table and its errors raised: b.tinfo, b.rowner, owner, b.mask_lo
rc::Queries rcmd_prep_rangedeps(acc_ctx *ctx, const acc_rcmd *store, const acc_cfk_mixed_queries *in, RdBuild &b, uint32_t *&owner);
void rcmd_bind_store_index(RdBuild &b, const acc_rcmd *store, const rc::Queries &Q, const uint32_t *owner);
// the stats acc_rcmd_rangedeps leaves: stabbed == false for a call that stabbed nothing
void rcmd_rangedeps_stats(acc_ctx *ctx, const acc_rcmd *store, const RdBuild &b, bool stabbed);
void rcmd_publish_view(acc_ctx *ctx, const RdBuild &b, acc_rangedeps_view *view);
void rcmd_rangedeps(acc_ctx *ctx, acc_rcmd *store, const acc_cfk_mixed_queries *q, acc_rangedeps_view *view);

// ---- rcmd_partial.hip
void rcmd_union_free(acc_rcmd *store);

}  // namespace acc
