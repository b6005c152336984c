// cfkredundant.hpp — the device passes behind acc_cfk_redundant_before (cfkredundant.hip), called by the store's host
// code in cfk.hip: the RedundantBefore map's max-merge, the prune of the key-major state, and the deps pre-pass of
// acc_cfk_apply_deps under a non-empty map. The range-command store (rcmd.hip, acc_rcmd_redundant_before) keeps its map
// through the same two steps (rb_stage_ranges, rb_merge_staged) and moves its deps with the same segmented copy.
#pragma once

#include "cfkquery.hpp"
#include "conflicts.hpp"

namespace acc {

// what one prune pass found and wrote (sizes of the new state; advanced == 0: nothing was rewritten)
struct RbPruned {
    uint64_t advanced = 0;   // stored keys whose bound rose
    uint32_t nk = 0;
    uint64_t ne = 0, nm = 0;
};

// One call's input on the device
struct RbInput {
    uint32_t n = 0;
    const uint64_t *rs = nullptr, *re = nullptr;    // the ranges
    const uint64_t *bm = nullptr, *bl = nullptr;    // their bounds
    const int32_t *bn = nullptr;
};

// Stages the input and validates its ranges (sorted, non-overlapping, start < end): ACC_E_ARG before anything changes.
RbInput rb_stage_ranges(acc_ctx *ctx, const acc_cfk_redundant_in *in);

// Merges a staged input into the map (pointwise Timestamp max).
void rb_merge_staged(acc_ctx *ctx, acc_maxconflicts *rb, const RbInput &in);

// rb_stage_ranges, RB_old of every stored key, rb_merge_staged: validates the ranges, keeps RB_old of every stored key, then merges the input into
// the map (pointwise Timestamp max). s / nk: the store's key-major state (nk == 0: no key to look up).
void rb_merge_map(acc_ctx *ctx, acc_maxconflicts *rb, const acc_cfk_redundant_in *in, const CfkResident &s);

// Prunes the key-major state s (ne entries, nm missing ids) against the map as merged by rb_merge_map: the new state in
// the context's cd_o* buffers (view), unless no key advanced.
RbPruned rb_prune(acc_ctx *ctx, const acc_maxconflicts *rb, const CfkResident &s, uint64_t ne, uint64_t nm,
                  acc_cfk_snap_view *view);

// The updates with every (update, key) pair's deps below RB(key) removed, as DEVICE arrays (out); returns the deps
// removed. Malformed dep offsets or unsorted deps leave *out = the staged input, which acc_cfk_apply then rejects.
uint64_t rb_trim_deps(acc_ctx *ctx, const acc_maxconflicts *rb, const acc_cfk_updates *up, acc_cfk_updates *out);

namespace rb {
// Columns that move together: up to four u64, two i32 and one u8 column, element i of each to element i's destination.
struct Cols {
    const uint64_t *s64[4];
    uint64_t *d64[4];
    const int32_t *s32[2];
    int32_t *d32[2];
    const uint8_t *s8;
    uint8_t *d8;
    int n64, n32;
};
}  // namespace rb

// Segmented copy of c's columns: destination elements [doff[s], doff[s + 1]) come from source elements sstart[s] + 0, 1,
// ...; doff[0] = 0, doff[ns] = *n_dev, non-decreasing. n_cap: a host-side upper bound of *n_dev (sizes the launch).
void rb_segcopy(acc_ctx *ctx, const char *name, const rb::Cols &c, uint64_t n_cap, const uint32_t *n_dev, uint32_t ns,
                const uint32_t *doff, const uint32_t *sstart);

}  // namespace acc
