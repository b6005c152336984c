// cfkquery.hpp — what cfkquery.hip reads of a resident CommandsForKey store (acc_cfk, cfk.hip): the key-major state
// acc_cfk_apply_deps maintains (the recovery scan also its missing[] lists) and the sorted TxnId columns of the
// txn-major view, as device pointers, in place.
#pragma once

#include "ctx.hpp"

namespace acc {

struct CfkResident {
    uint32_t n_txn = 0;     // the view's txns (TxnId order)
    bool deps = false;      // the store holds the key-major state
    // key-major: key k holds entries [ent_off[k], ent_off[k + 1]) in TxnId order
    uint32_t nk = 0;
    const uint64_t *key = nullptr;
    const uint32_t *ent_off = nullptr;
    const uint64_t *em = nullptr, *el = nullptr, *xm = nullptr, *xl = nullptr;   // TxnId / executeAt msb, lsb
    const int32_t *en = nullptr, *xn = nullptr;
    const uint8_t *st = nullptr;
    // entry e's missing[]: TxnIds [miss_off[e], miss_off[e + 1]) of the missing columns, sorted (acc_cfk_map_reduce_full)
    const uint32_t *miss_off = nullptr;
    const uint64_t *mm = nullptr, *ml = nullptr;
    const int32_t *mn = nullptr;
    // txn-major view: sorted TxnIds [n_txn]
    const uint64_t *tm = nullptr, *tl = nullptr;
    const int32_t *tn = nullptr;
};

CfkResident cfk_resident(const acc_cfk *cfk);   // cfk.hip

}  // namespace acc
