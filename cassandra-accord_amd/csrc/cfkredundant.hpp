// cfkredundant.hpp — the device passes behind acc_cfk_redundant_before (cfkredundant.hip), called by the store's host
// code in cfk.hip: the RedundantBefore map's max-merge, the prune of the key-major state, and the deps pre-pass of
// acc_cfk_apply_deps under a non-empty map.
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

// Validates the ranges (ACC_E_ARG before anything changes), keeps RB_old of every stored key, then merges the input into
// the map (pointwise Timestamp max). s / nk: the store's key-major state (nk == 0: no key to look up).
void rb_merge_map(acc_ctx *ctx, acc_maxconflicts *rb, const acc_cfk_redundant_in *in, const CfkResident &s);

// Prunes the key-major state s (ne entries, nm missing ids) against the map as merged by rb_merge_map: the new state in
// the context's cd_o* buffers (view), unless no key advanced.
RbPruned rb_prune(acc_ctx *ctx, const acc_maxconflicts *rb, const CfkResident &s, uint64_t ne, uint64_t nm,
                  acc_cfk_snap_view *view);

// The updates with every (update, key) pair's deps below RB(key) removed, as DEVICE arrays (out); returns the deps
// removed. Malformed dep offsets or unsorted deps leave *out = the staged input, which acc_cfk_apply then rejects.
uint64_t rb_trim_deps(acc_ctx *ctx, const acc_maxconflicts *rb, const acc_cfk_updates *up, acc_cfk_updates *out);

}  // namespace acc
