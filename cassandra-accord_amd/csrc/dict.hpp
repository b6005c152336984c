// dict.hpp — shared front end of the deps paths (dictionary.hip): input validation and the dense order-rank
// dictionary of every TxnId and executeAt of a batch (Timestamp.compareTo, primitives/Timestamp.java:208-217).
#pragma once

#include "prims.hpp"
#include "ts.hpp"
#include <functional>

namespace acc {

struct Dictionary {
    uint32_t *rank = nullptr;         // [2n]: rank[t] = TxnId of t, rank[n + t] = executeAt of t
    uint32_t *txn_of_rank = nullptr;  // [2n]: txn index of each TxnId rank
    int rbits = 0;                    // bits of the largest rank
    bool batch_sorted = false;        // txns given in TxnId order
    bool fast = false;                // sorted-batch dictionary taken
    bool ties_pending = false;        // its executeAt-tie check (g[6]) is still to be read by the caller
    uint64_t hg[8] = {};              // prep words: ts word masks [0..2], key mask [3], errors [4], unsorted [5],
                                      // OR of the key counts [6], executeAts that differ from their TxnId [7]
    uint64_t nbc = 0;                 // prep: keys of the bumped committed txns (ts.hpp) = entries of the bumped committed list
    bool fast_ok = false;             // prep: the sorted-batch dictionary applies
    // the sorted-batch dictionary's sorted bumped executeAts (valid while fast): txn of the k-th smallest = bsrc[sb_vals[k]]
    uint32_t nb = 0;
    const uint32_t *sb_vals = nullptr, *bsrc = nullptr;
};

// Dense order ranks of n composite keys of nw (1..3) u64 words, most significant first, compared unsigned after
// (word & and_mask[k]) ^ xor_mask[k] (null masks: identity). rank[i] in [0, count); first[r] = smallest index of rank r
// (want_first). count is left on device (count_dev) for the caller's next sync. Buffers named "<tag>.*".
struct DenseRank {
    uint32_t *rank = nullptr;
    uint32_t *first = nullptr;
    const uint32_t *perm = nullptr;   // the stable sorted order of the n keys (nullptr: identity, every key equal)
    uint64_t *count_dev = nullptr;
    uint64_t count = 0;
};
DenseRank dense_rank(acc_ctx *ctx, const char *tag, size_t n, int nw, const uint64_t *const *words, const uint64_t *and_mask,
                     const uint64_t *xor_mask, bool want_first);

// key_off/key_code: the key-domain part (P pairs); owner[P] receives the txn of every pair; g[8] scratch words.
// the prep / dictionary flag words: g[0..7], then the prep pass's slotted partials (PREP_SLOTS rows of PREP_ROW words, nine
// of them used), zeroed by one fill
constexpr uint32_t PREP_SLOTS = 64, PREP_ROW = 16;
constexpr size_t PREP_G_WORDS = 8 + (size_t)PREP_SLOTS * PREP_ROW;
// prep_dictionary = prep_batch (the prep pass and its host sync: validation, the masks, sortedness, out.fast_ok, out.nbc;
// allocates the rank arrays) + build_dictionary (the ranks; enqueued on ctx->cur(): a caller that has work independent
// of the ranks runs the sorted-batch dictionary on the side lane beside it, which needs out.fast_ok and defer_ties).
void prep_batch(acc_ctx *ctx, uint32_t n, size_t P, const uint64_t *tm, const uint64_t *tl, const int32_t *tn,
                const uint64_t *em, const uint64_t *el, const int32_t *en, const uint8_t *status, const uint32_t *key_off,
                const uint64_t *key_code, uint32_t *owner, uint64_t *g, Dictionary &out);
void build_dictionary(acc_ctx *ctx, uint32_t n, const uint64_t *tm, const uint64_t *tl, const int32_t *tn,
                      const uint64_t *em, const uint64_t *el, const int32_t *en, uint64_t *g, Dictionary &out, bool defer_ties);
void prep_dictionary(acc_ctx *ctx, uint32_t n, size_t P, const uint64_t *tm, const uint64_t *tl, const int32_t *tn,
                     const uint64_t *em, const uint64_t *el, const int32_t *en, const uint8_t *status,
                     const uint32_t *key_off, const uint64_t *key_code, uint32_t *owner, uint64_t *g, Dictionary &out,
                     bool defer_ties = false);
void redo_general_dictionary(acc_ctx *ctx, uint32_t n, const uint64_t *tm, const uint64_t *tl, const int32_t *tn,
                             const uint64_t *em, const uint64_t *el, const int32_t *en, uint64_t *g, Dictionary &d);

// The validation error bits of the prep pass and the dictionary (g[4] / hg[4]); check_errors throws the first one set.
enum : uint32_t {
    ERR_BAD_STATUS = 1u << 0,
    ERR_BAD_KIND = 1u << 1,
    ERR_LOCAL_ONLY = 1u << 2,
    ERR_KEYS_UNSORTED = 1u << 3,
    ERR_DUP_TXNID = 1u << 4,
    ERR_KEY_OFF = 1u << 5,
    ERR_KEY_TOTAL = 1u << 6,   // key_off[n] != n_pairs
};
void check_errors(uint64_t errs);

// The dictionary of a batch computed by one half of PartialDeps, handed to the other (acc_partial_deps_batch): valid
// when the KeyDeps half ran prep_dictionary (the batch has key pairs).
struct SharedDict {
    bool valid = false;
    Dictionary dict;
    const uint32_t *owner = nullptr;   // [P] txn of every key pair
    // called by keydeps_mixed once the dictionary is final (its kernels enqueued on the context stream): starts the
    // RangeDeps half concurrently with the rest of the KeyDeps half
    std::function<void(const SharedDict &)> ready;
};

}  // namespace acc
