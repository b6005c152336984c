// conflicts.hpp — what other translation units read of the device-resident ReducingRangeMap<Timestamp> of conflicts.hip
// (acc_maxconflicts): the interval list, a point lookup, and the max-merge of a batch of updates. cfkredundant.hip keeps a
// CommandsForKey store's RedundantBefore (reduced to shardRedundantBefore) in one.
#pragma once

#include "dict.hpp"
#include "search.hpp"

struct acc_maxconflicts {
    int device = 0;
    uint32_t end_inclusive = 1;
    uint64_t nv = 0, cap = 0;                         // intervals, allocated capacity
    uint64_t *st = nullptr, *en = nullptr;            // [cap] closed interval bounds
    uint64_t *vm = nullptr, *vl = nullptr;            // [cap] values (msb, lsb)
    int32_t *vn = nullptr;                            // [cap] values (node)
    uint64_t *bm = nullptr, *bl = nullptr;            // [cap / MC_BLK + 1] block maxima
    int32_t *bn = nullptr;
};

namespace acc {
namespace mc {

struct Map {
    const uint64_t *st, *en, *vm, *vl, *bm, *bl;
    const int32_t *vn, *bn;
    uint64_t nv;
    int ei;
};

// the value at key code k: the one interval with st <= k <= en, or Timestamp.NONE where the map holds nothing
__device__ __forceinline__ Ts point(const Map &mp, uint64_t k)
{
    const uint64_t i = lower_bound(mp.en, 0, mp.nv, k);
    if (i >= mp.nv || mp.st[i] > k) return Ts{ 0, 0, 0 };
    return Ts{ mp.vm[i], mp.vl[i], mp.vn[i] };
}

}  // namespace mc

inline mc::Map mc_map(const acc_maxconflicts *M)
{
    return mc::Map{ M->st, M->en, M->vm, M->vl, M->bm, M->bl, M->vn, M->bn, M->nv, (int)M->end_inclusive };
}

acc_maxconflicts *mc_new(int device, uint32_t end_inclusive);
void mc_free(acc_maxconflicts *m);
void mc_update(acc_ctx *ctx, acc_maxconflicts *m, const acc_conflicts_in *u);

}  // namespace acc
