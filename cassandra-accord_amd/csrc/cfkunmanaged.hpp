// cfkunmanaged.hpp — the Unmanaged pending records of a resident CommandsForKey store (cfkunmanaged.hip), called by the
// store's host code in cfk.hip: the pending table the store owns, the two halves of acc_cfk_register_unmanaged (the
// evaluation with the merged key-major state, then the append once the store has adopted that state) and the record
// pass of acc_cfk_notify_unmanaged.
#pragma once

#include "cfkquery.hpp"
#include "conflicts.hpp"

namespace acc {
namespace um {

// The pending table: DEVICE arrays the store owns, records in registration order. Record r waits on key[r] until
// `until` (pending 0: the commit of its deps up to that TxnId; 1: the application of everything executing before that
// executeAt); a COMMIT record keeps the waiter's dep list for the key, deps [dep_off[r], dep_off[r + 1]).
struct Table {
    uint32_t n_rec = 0;
    uint64_t n_dep = 0;
    size_t cap_rec = 0, cap_dep = 0;
    uint64_t *key = nullptr, *um = nullptr, *ul = nullptr, *tm = nullptr, *tl = nullptr, *xm = nullptr, *xl = nullptr;
    int32_t *un = nullptr, *tn = nullptr, *xn = nullptr;
    uint8_t *pending = nullptr;
    uint32_t *dep_off = nullptr;
    uint64_t *dm = nullptr, *dl = nullptr;
    int32_t *dn = nullptr;
};

void table_free(Table &t);

// one call's waiters on the device (acc_cfk_unmanaged_in, staged)
struct In {
    uint32_t nw;
    uint64_t NP, ND;
    const uint64_t *tm, *tl, *xm, *xl;
    const int32_t *tn, *xn;
    const uint32_t *key_off;
    const uint64_t *key;
    const uint32_t *dep_off;
    const uint64_t *dm, *dl;
    const int32_t *dn;
};

// what one evaluation found; its per-pair arrays stay in the context's um_* buffers for register_append
struct Registered {
    uint64_t n_pairs = 0, n_inserted = 0;
    uint64_t ready = 0, pending_commit = 0, pending_apply = 0;
    uint32_t n_new_rec = 0;
    uint64_t n_new_dep = 0;
    In in{};
    acc_cfk_snap_view view{};   // the merged key-major state in the context's cd_o* buffers (n_inserted != 0)
};

// Validates and evaluates every (waiter, key) pair against the state s (ne entries, nm missing ids) and the map rb
// (null: no bound anywhere), fills *out, grows the table's capacity for the new records, and, when a dep is missing,
// writes the state with the TRANSITIVELY_KNOWN entries merged in. Neither the store nor the table's content changes.
Registered register_eval(acc_ctx *ctx, const acc_maxconflicts *rb, const CfkResident &s, uint64_t ne, uint64_t nm, Table &t,
                         const acc_cfk_unmanaged_in *in, acc_cfk_unmanaged_out *out);

// Appends the not-ready pairs of the last register_eval on this context as records.
void register_append(acc_ctx *ctx, Table &t, const Registered &r);

// The COMMIT and APPLY steps over the records of the asked keys (akey: DEVICE, sorted unique, the rows of min_unc /
// next; null: the rows are the store's keys and every record is asked), the events, and the stable compaction.
void notify(acc_ctx *ctx, const acc_maxconflicts *rb, const CfkResident &s, Table &t, const uint64_t *akey, uint32_t n_asked,
            const uint32_t *min_unc, const uint32_t *next, acc_cfk_unmanaged_events *out);

}  // namespace um
}  // namespace acc
