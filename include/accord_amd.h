/*
 * accord_amd.h — C ABI of the MI355X-native Accord dependency-calculation path.
 *
 * This is the drop-in boundary a JVM shim (JNI for Java 11, FFM for Java >= 22) binds; see
 * INTEGRATION.md for the binding stubs. Plain pointers and sizes only: no C++, no torch types.
 *
 * Reference interfaces replaced (paths relative to accord-core/src/main/java/accord/):
 *
 *   acc_keydeps_batch      PreAccept.calculatePartialDeps            messages/PreAccept.java:245-265
 *                          -> SafeCommandStore.mapReduceActive        local/SafeCommandStore.java:279
 *                          -> InMemorySafeStore.mapReduceActive       impl/InMemoryCommandStore.java:863-870
 *                          -> CommandsForKey.mapReduceActive          local/CommandsForKey.java:614-650
 *                          -> KeyDeps.Builder / AbstractBuilder.build utils/RelationMultiMap.java:88-260
 *                          evaluated for every txn of a batch against one CommandsForKey snapshot
 *                          (batch semantics: SURVEY.md §8 "Batch semantics").
 *   acc_keydeps_merge      KeyDeps.merge(List, getter, getter)       primitives/KeyDeps.java:115-135
 *                          (LinearMerger fold of linearUnion,         utils/RelationMultiMap.java:284-406,561-816)
 *                          batched over many coordinated txns (Deps.merge primitives/Deps.java:256-260).
 *   acc_rangedeps_batch    the range-command part of InMemorySafeStore.mapReduceActive impl/InMemoryCommandStore.java:863-870
 *                          -> mapReduceRangesInternal                 impl/InMemoryCommandStore.java:883-1016
 *                          -> RangeDeps.Builder                       primitives/RangeDeps.java:873-891
 *                          for every txn of a mixed key/range batch (PreAccept.calculatePartialDeps
 *                          messages/PreAccept.java:245-265; SearchableRangeList stabbing core/utils/SearchableRangeList.java:89-116).
 *   acc_shard_pack /       per-node reduce of per-CommandStore PartialDeps across GPUs (PreAccept.reduce
 *   acc_shard_merge        messages/PreAccept.java:141-156, CommandStores.mapReduce local/CommandStores.java:575-592):
 *                          fragments to the txn's home GPU (all-to-all(v) by the host over RCCL), then KeyDeps.with
 *                          folded in shard order = the batched KeyDeps.merge below.
 *   acc_partial_deps_batch both halves of PartialDeps of a mixed batch in one call (KeyDeps + RangeDeps through
 *                          PartialDeps.Builder primitives/PartialDeps.java:31-45), one shared dictionary pass.
 *   acc_map_reduce_full    the recovery scans of BeginRecovery        messages/BeginRecovery.java:334-378
 *                          -> SafeCommandStore.mapReduceFull          local/SafeCommandStore.java:285
 *                          -> InMemorySafeStore.mapReduceFull         impl/InMemoryCommandStore.java:874-881 (key part)
 *                          -> CommandsForKey.mapReduceFull            local/CommandsForKey.java:553-612
 *                          -> Deps.Builder                            primitives/Deps.java:46-96
 *                          for a batch of recovery queries against one CommandsForKey snapshot.
 *   acc_map_reduce_full_ranges  the range-command half of the same scans  impl/InMemoryCommandStore.java:883-1016
 *   acc_latest_deps_merge  LatestDeps.mergeProposal / mergeCommit     primitives/LatestDeps.java:306-326
 *                          (Recover.java:295-355): the interval fold of the replies, then KeyDeps/RangeDeps.slice of
 *                          every selected deps object to its interval and the batched Deps.merge of the slices.
 *   acc_deps_from_json /   Json.DEPS_ADAPTER read / write             accord-maelstrom/.../maelstrom/Json.java:316-398
 *   acc_deps_to_json       (the in-tree Deps wire format) parsed / written on device, with the KeyDeps / RangeDeps Builder.
 *   acc_cfk_*              CommandsForKey.update for batches of commands   local/CommandsForKey.java:652-706
 *                          against a CFK store kept in HBM (SafeCommandStore.updateCommandsForKey :217-240).
 *   acc_cfk_map_reduce_full  the same recovery scans (BeginRecovery.java:330-380 -> CommandsForKey.mapReduceFull
 *                          local/CommandsForKey.java:553-612) read from the resident CFK store's segments in place.
 *   acc_rcmd_*             the rangeCommands map of a CommandStore kept in HBM: InMemorySafeStore.update
 *                          impl/InMemoryCommandStore.java:739-762 (RangeCommand.update = ranges.with(add), :524-539) for
 *                          batches of commands, and the range-command half of mapReduceActive (:863-870, :883-960) for
 *                          new txns only, read from the store's resident stabbing index.
 *   acc_rcmd_map_reduce_full  the range-command half of the recovery scans (mapReduceRangesInternal :883-960 with every
 *                          TestStartedAt / TestDep / TestStatus) read from the same store and the state its updates
 *                          carry (acc_rcmd_update_cmds).
 *   acc_rcmd_redundant_before  CommandStore.markShardDurable (local/CommandStore.java:520-528 ->
 *                          impl/InMemoryCommandStore.java:346-370) on the same store: the prune of its range half.
 *   acc_levelise           execution-order restatement of Commands.updateWaitingOn local/Commands.java:776-830
 *                          (deterministic wavefront schedule).
 *
 * Array-level seams mirrored: KeyDeps.SerializerSupport.create(Keys, TxnId[], int[])
 * (primitives/KeyDeps.java:55-73): every per-txn result is emitted as the exact Java `keysToTxnIds`
 * int[] plus the key subset and the TxnId array (as batch indices).
 *
 * Error model (utils/Invariants.java:98-205): IllegalArgumentException -> ACC_E_ARG,
 * IllegalStateException / AssertionError -> ACC_E_STATE. Device failures have their own codes.
 * acc_last_error(ctx) returns the message of the last failing call on that context.
 *
 * Threading (local/SafeCommandStore.java:50-55): one acc_ctx per host thread / CommandStore shard;
 * calls on one ctx are not re-entrant; distinct contexts run on independent HIP streams.
 */
#ifndef ACCORD_AMD_H
#define ACCORD_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A Ranges: sorted, deoverlapped Range (start, end) key codes of one bound type (primitives/Ranges.java). */
typedef struct acc_rlist {
    const uint64_t *start;
    const uint64_t *end;
    uint32_t n;
    uint32_t reserved;
} acc_rlist;

/* ---- error codes ---- */
#define ACC_OK          0
#define ACC_E_ARG      (-1)   /* IllegalArgumentException class */
#define ACC_E_STATE    (-2)   /* IllegalStateException / invariant violation */
#define ACC_E_NOMEM    (-3)   /* device allocation failed */
#define ACC_E_DEVICE   (-4)   /* HIP runtime error */
#define ACC_E_CAP      (-5)   /* caller buffer too small; required sizes were written */

/* ---- InternalStatus ordinals (local/CommandsForKey.java:194-203) ---- */
#define ACC_ST_TRANSITIVELY_KNOWN   0
#define ACC_ST_HISTORICAL           1
#define ACC_ST_PREACCEPTED          2
#define ACC_ST_ACCEPTED             3
#define ACC_ST_COMMITTED            4
#define ACC_ST_STABLE               5
#define ACC_ST_APPLIED              6
#define ACC_ST_INVALID_OR_TRUNCATED 7

/* ---- Txn.Kind ordinals (primitives/Txn.java:53-113); kind = (lsb >> 1) & 7 (TxnId.java:149-152) ---- */
#define ACC_KIND_READ                 0
#define ACC_KIND_WRITE                1
#define ACC_KIND_EPHEMERAL_READ       2
#define ACC_KIND_SYNC_POINT           3
#define ACC_KIND_EXCLUSIVE_SYNC_POINT 4
#define ACC_KIND_LOCAL_ONLY           5

/* ---- memory placement of caller arrays ---- */
#define ACC_MEM_HOST   0
#define ACC_MEM_DEVICE 1

/* ---- context options ---- */
#define ACC_OPT_TIMING 0x1u   /* record per-kernel HIP events (bench / profiling) */
#define ACC_OPT_FORCE_REPLAY 0x2u  /* always take the exact FAST-bisection replay path (testing) */
#define ACC_OPT_NO_WINDOW_TIER 0x4u  /* KeyDeps: the sorting build tiers instead of the window tier (testing) */
#define ACC_OPT_RD_WIDE_SORT 0x8u    /* RangeDeps: 64-bit sort keys in the lane-group build tiers (testing) */
/* flags bits 16..31 (testing): persistent KeyDeps write-tier grids, the window tier and the sorting tiers, are capped at
 * this many blocks (0: the defaults). It rides in flags because the layout of acc_opts is fixed. */
#define ACC_OPT_TIER_GRID_SHIFT 16
#define ACC_OPT_TIER_GRID(n) ((uint32_t)(n) << ACC_OPT_TIER_GRID_SHIFT)
#define ACC_OPT_PD_SERIAL 0x10u      /* acc_partial_deps_batch: both halves in order on this context (one buffer set:
                                        less device memory, no overlap) */
#define ACC_OPT_KD_NO_STREAM_AHEAD 0x20u /* KeyDeps: the lean stream pass behind the size read-back, with the other write
                                            kernels, never ahead of it (testing) */

/* levelise walk (acc_opts.lv_tier); AUTO picks the whole-graph LDS walk up to 65,535 txns, the windowed walk beyond */
#define ACC_LV_AUTO     0u
#define ACC_LV_LDS_WALK 1u
#define ACC_LV_WINDOWED 2u
#define ACC_LV_WAVES    3u

typedef struct acc_ctx acc_ctx;

/* Context options, fixed at acc_create (the library reads no environment): flags plus the knobs the tests use to force
 * a code path; zero everywhere = the defaults. */
typedef struct acc_opts {
    uint32_t flags;           /* ACC_OPT_* */
    uint32_t wave_grid_max;   /* wave-per-item launches (chunk scans of acc_cfk_keydeps and of the recovery scans) are
                                 issued in slices of at most this many blocks (0: 2^23; clamped to 1..2^23) */
    uint32_t cfk_hot;         /* acc_cfk_apply: keys with more than this many sorted elements take the closed form
                                 of the replay (0: 64) */
    uint32_t lv_tier;         /* ACC_LV_* */
    uint32_t lv_chunk;        /* the LDS walk's dependency chunk cap in entries (0: as large as the LDS allows) */
    uint32_t cfq_wave_cap;    /* acc_cfk_keydeps: queries with at most this many emitted entries build their KeyDeps in
                                 one wave's LDS, larger ones through the sorting tier (0: 1024; clamped to 1..1024) */
} acc_opts;

/* Timestamp / TxnId as three SoA columns: Timestamp.msb, Timestamp.lsb, Node.Id.id
 * (primitives/Timestamp.java:77-79). Order = Timestamp.compareTo (:208-217), identity = equals (:244-249). */
typedef struct acc_ts_cols {
    const uint64_t *msb;
    const uint64_t *lsb;
    const int32_t  *node;
} acc_ts_cols;

/* One batch = one CommandsForKey snapshot of one CommandStore. Every txn of the batch is both an
 * entry of the CFK of each of its keys and a query T evaluated with startedBefore = T.executeAt and
 * testKind = T.kind().witnesses(); p1 = (executeAt.equals(txnId) ? null : txnId). */
typedef struct acc_batch_in {
    uint32_t    n_txn;        /* N */
    uint32_t    mem;          /* ACC_MEM_HOST or ACC_MEM_DEVICE for every pointer below */
    uint64_t    n_pairs;      /* P = key_off[N]; must be < 2^32 */
    acc_ts_cols txn_id;       /* [N] TxnIds, pairwise distinct under Timestamp.equals */
    acc_ts_cols execute_at;   /* [N] executeAt (== txnId for PREACCEPTED-style entries) */
    const uint8_t  *status;   /* [N] InternalStatus ordinal */
    const uint32_t *key_off;  /* [N+1] CSR offsets into key_code */
    const uint64_t *key_code; /* [P] order-preserving key codes, sorted unique within each txn (Keys) */
} acc_batch_in;

/* Result view of the last acc_keydeps_batch on a context. Pointers are DEVICE pointers owned by
 * the context and valid until the next compute call on it. For txn t:
 *   arena[arena_off[t] .. arena_off[t+1])  = Java KeyDeps.keysToTxnIds (int[]) of t's PartialDeps
 *   key_idx[kd_off[t] .. kd_off[t+1])      = KeyDeps.keys as indices into t's input keys
 *   dep_txn[u_off[t] .. u_off[t+1])        = KeyDeps.txnIds as batch indices, ascending TxnId order */
typedef struct acc_keydeps_view {
    uint32_t n_txn;
    uint64_t total_arena, total_keys, total_deps, total_edges; /* Σ(Kd+E), ΣKd, ΣU, ΣE */
    const uint64_t *arena_off;
    const int32_t  *arena;
    const uint64_t *kd_off;
    const uint32_t *key_idx;
    const uint64_t *u_off;
    const uint32_t *dep_txn;
    const uint64_t *kd_key;   /* [total_keys] KeyDeps.keys as key codes (acc_keydeps_mixed; null after acc_keydeps_batch) */
} acc_keydeps_view;

/* Caller-owned output buffers (two-call sizing: capacities in elements; a call with null offset
 * arrays, or with a capacity below the requirement, returns ACC_E_CAP after writing the required
 * totals to need_*, and touches nothing else). */
typedef struct acc_keydeps_out {
    uint32_t  mem;            /* ACC_MEM_HOST or ACC_MEM_DEVICE */
    uint64_t  cap_arena, cap_keys, cap_deps;
    uint64_t  need_arena, need_keys, need_deps;  /* written */
    uint64_t *arena_off;      /* [N+1] */
    int32_t  *arena;          /* [cap_arena] */
    uint64_t *kd_off;         /* [N+1] */
    uint32_t *key_idx;        /* [cap_keys] */
    uint64_t *u_off;          /* [N+1] */
    uint32_t *dep_txn;        /* [cap_deps] */
    uint64_t *kd_key;         /* optional [cap_keys]: key codes, copied when non-null and the result has them */
} acc_keydeps_out;

/* ---- context ---- */
int         acc_create(int device, const acc_opts *opts, acc_ctx **out_ctx);
void        acc_destroy(acc_ctx *ctx);
const char *acc_last_error(const acc_ctx *ctx);
int         acc_sync(acc_ctx *ctx);
/* HIP stream (hipStream_t) the context launches on, as an opaque handle. */
void       *acc_stream(acc_ctx *ctx);
const char *acc_version(void);

/* ---- KeyDeps batch: CommandsForKey conflict scan + KeyDeps.Builder for all txns of a batch ---- */
int acc_keydeps_batch(acc_ctx *ctx, const acc_batch_in *in, acc_keydeps_view *out_view);
int acc_keydeps_copy_out(acc_ctx *ctx, acc_keydeps_out *out);

/* ---- RangeDeps batch: range-command stabbing + RangeDeps.Builder for all txns of a mixed batch ----
 * Txns whose TxnId domain bit (lsb & 1, TxnId.java:124-157) is Range are range commands/queries with Ranges
 * rng_start/rng_end[rng_off[t] .. rng_off[t+1]) (sorted and deoverlapped, start < end); key-domain txns list keys
 * in key_off/key_code exactly as acc_batch_in and no ranges. A range txn whose status is INVALID_OR_TRUNCATED is
 * an erased range command (saveStatus >= Erased, InMemoryCommandStore.java:892-893) and contributes no deps. */
typedef struct acc_range_batch_in {
    uint32_t    n_txn;
    uint32_t    mem;           /* ACC_MEM_HOST or ACC_MEM_DEVICE for every pointer below */
    uint64_t    n_pairs;       /* P = key_off[N] */
    uint64_t    n_ranges;      /* R = rng_off[N]; P + R < 2^32 */
    acc_ts_cols txn_id;
    acc_ts_cols execute_at;
    const uint8_t  *status;
    const uint32_t *key_off;   /* [N+1] */
    const uint64_t *key_code;  /* [P] */
    const uint32_t *rng_off;   /* [N+1] */
    const uint64_t *rng_start; /* [R] order-preserving codes of Range.start() */
    const uint64_t *rng_end;   /* [R] order-preserving codes of Range.end() */
    uint32_t    end_inclusive; /* 1: Range.EndInclusive (s, e]; 0: Range.StartInclusive [s, e) (Range.java:40-138) */
    uint32_t    reserved;
} acc_range_batch_in;

/* Result of the last acc_rangedeps_batch (device pointers owned by the context). Ranges are ids into the
 * dictionary of distinct stored ranges (the ranges of non-erased range commands) sorted by Range::compare
 * (start, then end; Range.java:309-317). For txn t:
 *   arena[arena_off[t] .. arena_off[t+1])      = Java RangeDeps.rangesToTxnIds (int[])
 *   range_id[rd_off[t] .. rd_off[t+1])        = RangeDeps.ranges as dictionary ids (ascending)
 *   dep_txn[u_off[t] .. u_off[t+1])           = RangeDeps.txnIds as batch indices, ascending TxnId order */
typedef struct acc_rangedeps_view {
    uint32_t n_txn;
    uint32_t n_ranges;                  /* dictionary size */
    uint64_t total_arena, total_ranges, total_deps, total_edges;
    const uint64_t *rng_start, *rng_end;   /* [n_ranges] dictionary */
    const uint64_t *arena_off;  const int32_t  *arena;
    const uint64_t *rd_off;     const uint32_t *range_id;
    const uint64_t *u_off;      const uint32_t *dep_txn;
} acc_rangedeps_view;

typedef struct acc_rangedeps_out {
    uint32_t  mem;
    uint64_t  cap_arena, cap_ranges, cap_deps, cap_dict;
    uint64_t  need_arena, need_ranges, need_deps, need_dict;   /* written */
    uint64_t *rng_start, *rng_end;      /* [cap_dict] */
    uint64_t *arena_off;  int32_t  *arena;     /* [N+1], [cap_arena] */
    uint64_t *rd_off;     uint32_t *range_id;  /* [N+1], [cap_ranges] */
    uint64_t *u_off;      uint32_t *dep_txn;   /* [N+1], [cap_deps] */
} acc_rangedeps_out;

int acc_rangedeps_batch(acc_ctx *ctx, const acc_range_batch_in *in, acc_rangedeps_view *out_view);

/* KeyDeps of every txn of a mixed key/range batch (the same input as acc_rangedeps_batch). Key txns: exactly
 * acc_keydeps_batch. A range-domain txn is no CommandsForKey member (SafeCommandStore.updateCommandsForKey registers
 * key txns only, local/SafeCommandStore.java:217-240); as a query it runs CommandsForKey.mapReduceActive on every CFK
 * whose key lies in its ranges with the Range bound inclusivity (InMemoryCommandStore.mapReduceForKey,
 * impl/InMemoryCommandStore.java:274-289). Replaces the key part of PreAccept.calculatePartialDeps for range txns
 * (messages/PreAccept.java:245-265). The view is acc_keydeps_view with kd_key filled for every txn; for a range txn,
 * key_idx indexes the list of CFK keys its ranges cover (range order). Copy out with acc_keydeps_copy_out. */
int acc_keydeps_mixed(acc_ctx *ctx, const acc_range_batch_in *in, acc_keydeps_view *out_view);
int acc_rangedeps_copy_out(acc_ctx *ctx, acc_rangedeps_out *out);
/* The whole PartialDeps of every txn of a mixed batch in one call (PreAccept.calculatePartialDeps,
 * messages/PreAccept.java:245-265, routing each emitted (key | range, TxnId) through PartialDeps.Builder,
 * primitives/PartialDeps.java:31-45 / Deps.AbstractBuilder.add primitives/Deps.java:56-71): the KeyDeps half of
 * acc_keydeps_mixed and the RangeDeps half of acc_rangedeps_batch, sharing one dictionary pass (and its validation) and
 * the staged inputs. Both views stay valid until the next compute call; acc_keydeps_copy_out / acc_rangedeps_copy_out
 * copy them. The RangeDeps half runs concurrently on a child context created on first use (own stream and its own
 * grow-only device buffers, held until acc_destroy of ctx; environment ACC_PD_SERIAL=1 keeps both halves on ctx). */
int acc_partial_deps_batch(acc_ctx *ctx, const acc_range_batch_in *in, acc_keydeps_view *key_view,
                           acc_rangedeps_view *range_view);

/* ---- Deps.merge over many replies per txn ----
 * Input: R = n_groups groups (one coordinated txn each); group g owns replies
 * [grp_off[g], grp_off[g+1]); reply r is a KeyDeps in Java layout over integer ids:
 *   keys:   key_code[key_off[r] .. key_off[r+1])          (sorted unique)
 *   txnIds: txn_rank[val_off[r] .. val_off[r+1])          (sorted unique u32 order ranks of TxnIds)
 *   keysToTxnIds: k2v[k2v_off[r] .. k2v_off[r+1])         (Java int[] verbatim)
 * Output per group: the KeyDeps.merge result (== canonical union, KeyDepsTest.java:275-283) in the
 * same three-array layout, device-resident in the context. */
typedef struct acc_merge_in {
    uint32_t mem;
    uint32_t n_groups;
    uint64_t n_replies;
    const uint64_t *grp_off;   /* [n_groups+1] into replies */
    const uint64_t *key_off;   /* [n_replies+1] */
    const uint64_t *key_code;  /* [key_off[n_replies]] */
    const uint64_t *val_off;   /* [n_replies+1] */
    const uint32_t *txn_rank;  /* [val_off[n_replies]] */
    const uint64_t *k2v_off;   /* [n_replies+1] */
    const int32_t  *k2v;       /* [k2v_off[n_replies]] */
} acc_merge_in;

typedef struct acc_merge_view {
    uint32_t n_groups;
    uint64_t total_keys, total_vals, total_k2v, total_in_entries;
    const uint64_t *key_off;  const uint64_t *key_code;
    const uint64_t *val_off;  const uint32_t *txn_rank;
    const uint64_t *k2v_off;  const int32_t  *k2v;
} acc_merge_view;

int acc_keydeps_merge(acc_ctx *ctx, const acc_merge_in *in, acc_merge_view *out_view);

/* Caller-owned copy of the last merge result (two-call sizing as acc_keydeps_out). */
typedef struct acc_merge_out {
    uint32_t  mem;
    uint64_t  cap_keys, cap_vals, cap_k2v;
    uint64_t  need_keys, need_vals, need_k2v;   /* written */
    uint64_t *key_off;  uint64_t *key_code;     /* [n_groups+1], [cap_keys] */
    uint64_t *val_off;  uint32_t *txn_rank;     /* [n_groups+1], [cap_vals] */
    uint64_t *k2v_off;  int32_t  *k2v;          /* [n_groups+1], [cap_k2v] */
} acc_merge_out;

int acc_merge_copy_out(acc_ctx *ctx, acc_merge_out *out);

/* ---- Deps.merge over raw deps objects ----
 * Deps.merge(List, getter) (primitives/Deps.java:256-260) = KeyDeps.merge (primitives/KeyDeps.java:115-135) and
 * RangeDeps.merge (primitives/RangeDeps.java:101-134) of the replies of each coordinated txn (group g owns replies
 * [grp_off[g], grp_off[g+1])), folded left to right by a LinearMerger (utils/RelationMultiMap.java:284-406), empty
 * replies skipped. Each reply half is given as the arrays KeyDeps/RangeDeps.SerializerSupport expose
 * (primitives/KeyDeps.java:55-73, primitives/RangeDeps.java:55-73): keys (or ranges), the TxnId[] as raw columns and the
 * Java keysToTxnIds / rangesToTxnIds int[] verbatim. TxnIds are ranked on device (Timestamp.compareTo / equals); an
 * equals-tie whose raw bits differ (flags outside IDENTITY_LSB) keeps the instance the Java fold keeps
 * (SortedArrays.linearUnion utils/SortedArrays.java:152-281, RelationMultiMap.linearUnion :561-816). */
typedef struct acc_rmm_in {
    const uint64_t *key_off;   /* [n_replies+1]; null: the half is absent (every result is NONE) */
    const uint64_t *key_a;     /* KeyDeps: key codes; RangeDeps: Range.start codes */
    const uint64_t *key_b;     /* RangeDeps: Range.end codes (Range::compare = (start, end), Range.java:310-317); KeyDeps: null */
    const uint64_t *val_off;   /* [n_replies+1] */
    acc_ts_cols     txn;       /* TxnId[] of every reply, raw */
    const uint64_t *k2v_off;   /* [n_replies+1] */
    const int32_t  *k2v;       /* keysToTxnIds / rangesToTxnIds int[] of every reply */
} acc_rmm_in;

typedef struct acc_deps_merge_in {
    uint32_t mem;              /* ACC_MEM_HOST or ACC_MEM_DEVICE for every pointer */
    uint32_t n_groups;
    uint64_t n_replies;
    const uint64_t *grp_off;   /* [n_groups+1] */
    acc_rmm_in key_deps;
    acc_rmm_in range_deps;
} acc_deps_merge_in;

/* A merged half per group g (device pointers owned by the context, valid until its next compute call):
 * keys/ranges key_a[key_off[g]..key_off[g+1]) (+ key_b), TxnIds txn_*[val_off[g]..], ints k2v[k2v_off[g]..].
 * txn_src = an input slot (index into the half's TxnId columns) holding the kept instance's raw bits. */
typedef struct acc_rmm_view {
    uint64_t total_keys, total_vals, total_k2v;
    const uint64_t *key_off;  const uint64_t *key_a;  const uint64_t *key_b;
    const uint64_t *val_off;  const uint64_t *txn_msb; const uint64_t *txn_lsb; const int32_t *txn_node;
    const uint32_t *txn_src;
    const uint64_t *k2v_off;  const int32_t  *k2v;
} acc_rmm_view;

typedef struct acc_deps_merge_view {
    uint32_t n_groups;
    uint64_t total_in_entries;          /* keysToTxnIds + rangesToTxnIds entries over every reply */
    acc_rmm_view key_deps, range_deps;
} acc_deps_merge_view;

int acc_deps_merge(acc_ctx *ctx, const acc_deps_merge_in *in, acc_deps_merge_view *out_view);

/* Copy any acc_rmm_view of this context into caller buffers (two-call sizing: null offset arrays or a capacity below
 * the need -> ACC_E_CAP after writing need_*). key_b / txn_src are copied when both the view and the caller have them. */
typedef struct acc_rmm_out {
    uint32_t  mem;
    uint64_t  cap_keys, cap_vals, cap_k2v;
    uint64_t  need_keys, need_vals, need_k2v;   /* written */
    uint64_t *key_off;  uint64_t *key_a;  uint64_t *key_b;        /* [n_groups+1], [cap_keys] x2 */
    uint64_t *val_off;  uint64_t *txn_msb; uint64_t *txn_lsb; int32_t *txn_node; uint32_t *txn_src;   /* [cap_vals] */
    uint64_t *k2v_off;  int32_t  *k2v;                            /* [cap_k2v] */
} acc_rmm_out;

int acc_rmm_copy_out(acc_ctx *ctx, uint32_t n_groups, const acc_rmm_view *view, acc_rmm_out *out);

/* ---- RelationMultiMap helpers over a batch of built deps objects (one KeyDeps or RangeDeps per group) ----
 * The arrays of KeyDeps/RangeDeps.SerializerSupport (primitives/KeyDeps.java:55-73, primitives/RangeDeps.java:55-73);
 * the TxnIds themselves are not needed (val_off gives their count per group). key_b null = KeyDeps (key codes),
 * non-null = RangeDeps (Range start/end codes sorted by Range::compare). */
typedef struct acc_rmm_batch {
    uint32_t mem;              /* ACC_MEM_HOST or ACC_MEM_DEVICE for every pointer (and for acc_ranges_in) */
    uint32_t n_groups;
    const uint64_t *key_off;   /* [n_groups+1] */
    const uint64_t *key_a;     /* key codes | Range.start codes */
    const uint64_t *key_b;     /* null | Range.end codes */
    const uint64_t *val_off;   /* [n_groups+1] TxnIds per group */
    const uint64_t *k2v_off;   /* [n_groups+1] */
    const int32_t  *k2v;       /* keysToTxnIds / rangesToTxnIds int[] per group */
} acc_rmm_batch;

/* Per-group int[] result (device pointers owned by the context): ints[off[g] .. off[g+1]). */
typedef struct acc_csr_view {
    uint32_t n_groups;
    uint64_t total;
    const uint64_t *off;
    const int32_t  *ints;
} acc_csr_view;

/* RelationMultiMap.invert (utils/RelationMultiMap.java:907-938) of every group: KeyDeps.txnIdsToKeys
 * (primitives/KeyDeps.java:350-362) / RangeDeps txnIdsToRanges: per group the Java int[] of nv end offsets (from nv)
 * followed by the key indices of each TxnId in ascending key order. */
int acc_rmm_invert(acc_ctx *ctx, const acc_rmm_batch *in, acc_csr_view *out_view);

/* Ranges per group (sorted, deoverlapped; Ranges.ofSortedAndDeoverlapped): [off[g], off[g+1]) of start/end. */
typedef struct acc_ranges_in {
    const uint64_t *off;       /* [n_groups+1] */
    const uint64_t *start;
    const uint64_t *end;
    uint32_t end_inclusive;    /* Range.EndInclusive (s, e] = 1; StartInclusive [s, e) = 0 (Range.java:40-138) */
    uint32_t reserved;
} acc_ranges_in;

/* Slice result per group: the selected key indices (into the group's keys, ascending), the kept TxnId indices (into
 * the group's txnIds, ascending) and the new keysToTxnIds int[] over the kept TxnIds. */
typedef struct acc_slice_view {
    uint32_t n_groups;
    uint64_t total_keys, total_vals, total_k2v;
    const uint64_t *key_off;  const uint32_t *key_idx;
    const uint64_t *val_off;  const uint32_t *val_idx;
    const uint64_t *k2v_off;  const int32_t  *k2v;
} acc_slice_view;

/* KeyDeps.slice(Ranges) (primitives/KeyDeps.java:189-236: keys contained in the ranges) / RangeDeps.slice(Ranges)
 * (primitives/RangeDeps.java:545-565: ranges intersecting them) with trimUnusedValues
 * (utils/RelationMultiMap.java:491-532), each group against its own select Ranges; the reference's short cuts are kept
 * (empty input, nothing selected, everything selected = `return this` without trimming). */
int acc_rmm_slice(acc_ctx *ctx, const acc_rmm_batch *in, const acc_ranges_in *select, acc_slice_view *out_view);

/* RelationMultiMap.remove (utils/RelationMultiMap.java:843-905) = KeyDeps.without (primitives/KeyDeps.java:255-259) /
 * RangeDeps.without (primitives/RangeDeps.java:584-588) of every group, with the predicate of the recovery callers
 * (`without(earlierCommittedWitness::contains)`, messages/BeginRecovery.java:180-183, coordinate/Recover.java:322):
 * remove(t) = Deps.contains(t) = KeyDeps.contains || RangeDeps.contains (primitives/Deps.java:107-110), each an
 * Arrays.binarySearch over that deps object's sorted TxnIds (Timestamp.compareTo == 0). The group's TxnId set(s) to
 * test against: set_a and set_b (either may be absent: off null), each sorted ascending by Timestamp.compareTo
 * without duplicates per group (ACC_E_ARG otherwise). The input half's TxnIds are `txn` ([val_off[n_groups]] raw).
 * Result per group, exactly as the Java returns:
 *   ACC_WITHOUT_FROM — `return from` (isEmpty(): no entries; or nothing removed): the input object itself;
 *   ACC_WITHOUT_NONE — `return none` (every TxnId removed): KeyDeps.NONE / RangeDeps.NONE, no keys;
 *   ACC_WITHOUT_NEW  — rebuilt: every key kept (keys whose lists emptied stay, :877-891), the kept TxnIds in order,
 *                      the new keysToTxnIds int[].
 * The view is an acc_slice_view over the input (key_idx: kept key indices, val_idx: kept TxnId indices, k2v: the
 * group's int[]; FROM groups list everything with the input int[] verbatim) plus the kind per group. */
#define ACC_WITHOUT_FROM 0
#define ACC_WITHOUT_NONE 1
#define ACC_WITHOUT_NEW  2

typedef struct acc_txn_sets {
    const uint64_t *off;       /* [n_groups+1]; null: every set is empty */
    acc_ts_cols     txn;       /* sorted unique TxnIds of every group's set */
} acc_txn_sets;

typedef struct acc_without_view {
    acc_slice_view sl;
    const uint8_t *kind;       /* [n_groups] ACC_WITHOUT_* */
    uint64_t n_from, n_none, n_new;
} acc_without_view;

int acc_rmm_without(acc_ctx *ctx, const acc_rmm_batch *in, const acc_ts_cols *txn, const acc_txn_sets *set_a,
                    const acc_txn_sets *set_b, acc_without_view *out_view);

/* The recovery reply reduce of the deps the recovery coordinator folds (coordinate/Recover.java:320-322; pairwise as
 * BeginRecovery.RecoverOk.reduce, messages/BeginRecovery.java:180-183): per recovered txn (group),
 *   earlierCommittedWitness  = Deps.merge(replies' earlierCommittedWitness)           -> committed_view,
 *   earlierAcceptedNoWitness = Deps.merge(replies' earlierAcceptedNoWitness)
 *                                .without(earlierCommittedWitness::contains)            -> accepted_merged + accepted_*.
 * Both merges as acc_deps_merge (same input layout; the replies in the order the Java folds them); the without runs on
 * the merged accepted halves with each group's merged committed key and range TxnIds as the two sets. accepted_key /
 * accepted_range index into accepted_merged's halves (val_idx into its TxnIds, key_idx into its keys / ranges).
 * Views are device pointers owned by the context, valid until its next compute call. */
typedef struct acc_recovery_deps_view {
    acc_deps_merge_view committed;        /* earlierCommittedWitness per group */
    acc_deps_merge_view accepted_merged;  /* Deps.merge of earlierAcceptedNoWitness per group (before the without) */
    acc_without_view accepted_key;        /* KeyDeps.without over accepted_merged.key_deps */
    acc_without_view accepted_range;      /* RangeDeps.without over accepted_merged.range_deps */
} acc_recovery_deps_view;

int acc_recovery_deps_reduce(acc_ctx *ctx, const acc_deps_merge_in *committed_witness,
                             const acc_deps_merge_in *accepted_no_witness, acc_recovery_deps_view *out_view);

/* Stabbing queries over built RangeDeps (SearchableRangeList.forEach, utils/SearchableRangeList.java:89-116;
 * RangeDeps.forEach / computeTxnIds, primitives/RangeDeps.java:152-412, 629-643): query q against group grp[q]:
 * a key (q_end null: Range.contains with the bound type) or a range [q_start, q_end) (compareIntersecting == 0). */
typedef struct acc_stab_in {
    uint32_t mem;
    uint32_t n_queries;
    const uint32_t *grp;       /* [n_queries] */
    const uint64_t *q_start;   /* [n_queries] key codes | range starts */
    const uint64_t *q_end;     /* [n_queries] range ends, or null for key queries */
    uint32_t end_inclusive;
    uint32_t want_txns;        /* also produce computeTxnIds (sorted unique TxnId indices) */
} acc_stab_in;

typedef struct acc_stab_view {
    uint32_t n_queries;
    uint64_t total_ranges, total_txns;
    const uint64_t *range_off; const uint32_t *range_idx;   /* ascending range indices per query */
    const uint64_t *txn_off;   const uint32_t *txn_idx;     /* want_txns: ascending TxnId indices per query */
} acc_stab_view;

int acc_rangedeps_stab(acc_ctx *ctx, const acc_rmm_batch *range_deps, const acc_stab_in *queries, acc_stab_view *out_view);

/* Copy `bytes` from a device pointer of a result view into caller memory (mem = ACC_MEM_HOST / ACC_MEM_DEVICE), on the
 * context stream, synchronously: lets a host without HIP bindings read any view. */
int acc_copy_out(acc_ctx *ctx, void *dst, const void *src_device, size_t bytes, uint32_t mem);

/* ---- Key-range CommandStore shards across GPUs (PreAccept.reduce) ----
 * acc_shard_pack: the last acc_keydeps_batch result of this shard (the same `in`) as fragments for the txns' home
 * ranks (home(t) = t mod world, t the global index). A fragment = header (t, nk, nv, no) + nk key codes + nv TxnIds (batch indices) +
 * no Java keysToTxnIds ints; only txns with a non-empty shard KeyDeps send one (PartialDeps.with skips empties).
 * Streams are destination-major: destination d owns elements [x_off[d], x_off[d+1]) of each stream. The caller
 * supplies the four stream buffers (two-call sizing: with a capacity below the need, ACC_E_CAP after writing the
 * four host offset arrays, whose last entries are the totals) and four HOST offset arrays of world+1 entries. */
typedef struct acc_frag_streams {
    uint32_t  world;
    uint32_t  mem;                                   /* placement of hdr/keys/vals/k2v */
    uint64_t  cap_frag, cap_keys, cap_vals, cap_k2v; /* capacities: fragments (hdr = 4 u32 each), elements */
    uint32_t *hdr;
    uint64_t *keys;
    uint32_t *vals;
    int32_t  *k2v;
    uint64_t *frag_off, *key_off, *val_off, *k2v_off;   /* host [world+1], written */
    const uint32_t *txn_global; /* optional [N], placement of the batch: global index of each batch txn (a store's
                                   batch holds only the txns touching its keys, in TxnId order); null = identity */
} acc_frag_streams;

int acc_shard_pack(acc_ctx *ctx, const acc_batch_in *in, acc_frag_streams *out);

/* acc_shard_merge: what this rank received, the four streams concatenated in source-rank (= shard) order, with the
 * per-source element counts (host arrays of `world` entries). Result: the merged KeyDeps of every home txn
 * t = rank + g * world (group g), in the acc_merge_view layout (txn ranks = batch indices). */
typedef struct acc_frag_recv {
    uint32_t mem;              /* placement of hdr/keys/vals/k2v */
    uint32_t world, rank, n_txn;
    const uint64_t *n_frag, *n_keys, *n_vals, *n_k2v;   /* host [world] */
    const uint32_t *hdr;
    const uint64_t *keys;
    const uint32_t *vals;
    const int32_t  *k2v;
} acc_frag_recv;

int acc_shard_merge(acc_ctx *ctx, const acc_frag_recv *in, acc_merge_view *out_view);

/* ---- The exchange between CommandStores on different GPUs, behind the ABI ----
 * acc_comm: a communicator of `world` ranks (one GPU and one acc_ctx each). Two transports:
 *   RCCL (acc_comm_init_rccl): rank 0 makes an id with acc_comm_unique_id and the host distributes the 128 bytes
 *     (any channel); device buffers move point to point over xGMI;
 *   host (acc_comm_init_host): the caller's all-to-all(v) of host bytes (e.g. a JVM node's own messaging): fn gets
 *     send[] with send_bytes[d] bytes for rank d (concatenated in rank order) and fills recv[] with recv_bytes[s]
 *     bytes from each rank s; returns 0 on success.
 * acc_shard_reduce: PreAccept.reduce of the store KeyDeps (messages/PreAccept.java:141-156, PartialDeps.with) for the
 * last acc_keydeps_batch on ctx over `in` (the same batch): acc_shard_pack, one exchange of the element counts, one
 * all-to-all(v) of the four fragment streams, acc_shard_merge; every rank calls it (collective). txn_global / n_global
 * as acc_frag_streams.txn_global and the global txn count; the result is acc_shard_merge's view. Every txn_global entry
 * must be below n_global (the placement is increasing, so its last entry is checked): ACC_E_ARG otherwise, here and in
 * acc_partial_deps_reduce, before anything is sent. */
#define ACC_COMM_ID_BYTES 128
typedef struct acc_comm acc_comm;
typedef int (*acc_alltoallv_fn)(void *user, const void *send, const uint64_t *send_bytes, void *recv,
                                const uint64_t *recv_bytes);
int  acc_comm_unique_id(uint8_t *id_out);   /* [ACC_COMM_ID_BYTES]; ACC_E_DEVICE without RCCL */
int  acc_comm_init_rccl(acc_ctx *ctx, uint32_t world, uint32_t rank, const uint8_t *id, acc_comm **out);
int  acc_comm_init_host(acc_ctx *ctx, uint32_t world, uint32_t rank, acc_alltoallv_fn fn, void *user, acc_comm **out);
void acc_comm_destroy(acc_comm *comm);
int  acc_shard_reduce(acc_ctx *ctx, acc_comm *comm, const acc_batch_in *in, const uint32_t *txn_global, uint32_t n_global,
                      acc_merge_view *out_view);
/* PartialDeps.covering (primitives/PartialDeps.java:31-58, 80-86). A store's txns all carry the store's Ranges as
 * covering (PreAccept.calculatePartialDeps: new PartialDeps.Builder(ranges), messages/PreAccept.java:245-265); the
 * reduced PartialDeps of a home txn carries the fold that.covering.with(this.covering) over the stores that replied
 * for it (every store whose batch holds the txn), in store order. Per home txn: cov_id into a table of the distinct
 * coverings (device memory owned by the context, valid until the next reduce) and the mask of the stores that replied.
 * Both calls check the PartialDeps constructor's invariants covering.containsAll(keyDeps.keys) and
 * rangeDeps.isCoveredBy(covering) for every txn (PartialDeps.java:52-58) -> ACC_E_STATE. */
typedef struct acc_covering_view {
    uint32_t n_groups;             /* home txns, as the reduce's key view */
    uint32_t n_coverings;          /* distinct coverings in the table */
    const uint32_t *cov_id;        /* [n_groups] */
    const uint64_t *cov_off;       /* [n_coverings+1] into cov_start / cov_end */
    const uint64_t *cov_start;
    const uint64_t *cov_end;
    const uint64_t *store_mask;    /* [n_groups] bit s: store (rank) s replied for the txn */
    uint64_t total_ranges;
} acc_covering_view;

/* The store's `covering` (sorted, deoverlapped; the batch's bound type) for the last acc_partial_deps_batch on ctx over
 * `in` (the same batch): the invariant checks of every txn's PartialDeps(covering, keyDeps, rangeDeps). */
int  acc_partial_deps_covering(acc_ctx *ctx, const acc_range_batch_in *in, const acc_rlist *covering);

/* acc_partial_deps_reduce: PreAccept.reduce of a store's whole PartialDeps (messages/PreAccept.java:141-156;
 * PartialDeps.with = KeyDeps.with + RangeDeps.with, primitives/PartialDeps.java:80-86) for the last
 * acc_partial_deps_batch on ctx over `in` (the same mixed batch): the KeyDeps fragments (as acc_shard_reduce) and the
 * RangeDeps fragments (ranges as (start, end) codes, TxnIds raw, rangesToTxnIds) of both halves in ONE size exchange
 * and ONE grouped all-to-all(v); on the home rank the KeyDeps.with fold (key_view, as acc_shard_reduce) and the
 * RangeDeps.with fold in store order (RangeDeps.java:567-582; the range half of range_view, raw TxnIds; its key half is
 * absent). A range command is stored sliced to each store's ranges (impl/InMemoryCommandStore.java:739-761), so the
 * result depends on the store split exactly as the reference's does. With `covering` (this store's Ranges; null: no
 * covering), the same exchange carries the store's txns and covering, and covering_view receives every home txn's
 * PartialDeps.covering (above). Collective over comm. */
int  acc_partial_deps_reduce(acc_ctx *ctx, acc_comm *comm, const acc_range_batch_in *in, const uint32_t *txn_global,
                             uint32_t n_global, const acc_rlist *covering, acc_merge_view *key_view,
                             acc_deps_merge_view *range_view, acc_covering_view *covering_view);

/* ---- Recovery scans: CommandsForKey.mapReduceFull over a batch of queries (SURVEY.md §8(f) N3 = A7) ----
 * The snapshot is an acc_batch_in (one CommandsForKey per key, as for acc_keydeps_batch) plus, per input pair j
 * (txn t, key k), the entry's TxnInfoWithMissing.missing (local/CommandsForKey.java:385-410): the TxnIds of that CFK
 * the txn's deps do not include, as batch indices sorted by TxnId, missing_txn[missing_off[j] .. missing_off[j+1]).
 * Every query q is one (testTxnId, keys) call of SafeCommandStore.mapReduceFull with the call-wide tests:
 *   started_at  TestStartedAt ordinal: 0 STARTED_BEFORE (txnId < testTxnId), 1 STARTED_AFTER (from the binarySearch
 *               insert position, testTxnId itself included when it is on the key), 2 ANY
 *   test_dep    TestDep ordinal: 0 WITH, 1 WITHOUT (testTxnId absent / present in missing), 2 ANY_DEPS; WITH and
 *               WITHOUT also need InternalStatus.hasInfo and executeAt > testTxnId; WITH skips keys where testTxnId
 *               is no CFK member
 *   test_status TestStatus ordinal: 0 ANY_STATUS (not TRANSITIVELY_KNOWN), 1 IS_PROPOSED (ACCEPTED, COMMITTED),
 *               2 IS_STABLE (STABLE, APPLIED)
 *   test_kinds  Kinds as a mask over Kind ordinals, or -1 for testTxnId.kind().witnessedBy() (Txn.java:247-262)
 *   flags       ACC_FULL_EXECUTES_AFTER: the map keeps only executeAt > testTxnId (BeginRecovery.java:339-341)
 * The result per query is the Deps.Builder KeyDeps of every (key, txnId) the map visited, in the acc_keydeps_view
 * layout (key_idx into the query's keys, dep_txn = batch indices); the boolean recovery predicates
 * (hasAcceptedOrCommittedStartedAfterWithoutWitnessing, hasStableExecutesAfterWithoutWitnessing) are
 * u_off[q+1] > u_off[q]. acc_keydeps_copy_out copies it. The range commands' half of the same call is
 * acc_map_reduce_full_ranges below. */
#define ACC_STARTED_BEFORE 0
#define ACC_STARTED_AFTER  1
#define ACC_STARTED_ANY    2
#define ACC_DEP_WITH       0
#define ACC_DEP_WITHOUT    1
#define ACC_DEP_ANY        2
#define ACC_STATUS_ANY         0
#define ACC_STATUS_IS_PROPOSED 1
#define ACC_STATUS_IS_STABLE   2
#define ACC_FULL_EXECUTES_AFTER 1u

typedef struct acc_recovery_in {
    uint32_t    n_query;
    uint32_t    mem;            /* placement of the query arrays and of missing_off / missing_txn */
    acc_ts_cols test_txn;       /* [n_query] testTxnId of each query (any TxnId, batch member or not) */
    const uint32_t *key_off;    /* [n_query+1] */
    const uint64_t *key_code;   /* keys of each query, sorted unique (Keys) */
    const uint32_t *missing_off;/* [n_pairs+1] of the snapshot */
    const uint32_t *missing_txn;/* [n_missing] batch indices */
    uint64_t    n_missing;
    uint8_t     started_at, test_dep, test_status, flags;
    int32_t     test_kinds;
} acc_recovery_in;

int acc_map_reduce_full(acc_ctx *ctx, const acc_batch_in *snapshot, const acc_recovery_in *q, acc_keydeps_view *out_view);

/* ---- Recovery scans, range-command half: InMemorySafeStore.mapReduceRangesInternal
 * (impl/InMemoryCommandStore.java:883-1016), the second half of SafeCommandStore.mapReduceFull (:874-881) ----
 * The store's range commands are a table of n_cmd entries sorted by TxnId (non-decreasing): the rangeCommands map (a
 * TreeMap by TxnId) and, flagged ACC_RCMD_HISTORICAL, the historicalRangeCommands map (a TxnId may be in both). Entry c:
 *   txn_id, execute_at  Command.executeAt() (executeAtOrTxnId where it is null; a historical entry: its TxnId)
 *   status              Status ordinal (local/Status.java:47-86: NotDefined 0 .. Accepted 3, PreCommitted 4,
 *                       Committed 5, Stable 6, PreApplied 7, Applied 8, Truncated 9, Invalidated 10)
 *   flags               ACC_RCMD_ERASED: saveStatus >= Erased, never visited (:891-893); ACC_RCMD_HAS_DEPS:
 *                       known().deps.hasProposedOrDecidedDeps() (Status.java:601-612); ACC_RCMD_HISTORICAL (:962-1004):
 *                       visited only when test_status = ANY_STATUS and test_dep = ANY_DEPS, with executeAt = TxnId
 *   ranges              [rng_off[c], rng_off[c+1]): sorted, non-overlapping, start < end, bound type end_inclusive
 *   deps                its PartialDeps flattened to (TxnId, participant) pairs sorted by TxnId: dep_txn[dep_off[c] ..
 *                       dep_off[c+1]), a KeyDeps entry with dep_is_key = 1 and its key in dep_start, a RangeDeps entry
 *                       with its range [dep_start, dep_end). The WITH / WITHOUT test is Deps.intersects(testTxnId,
 *                       the entry's ranges) (primitives/Deps.java:112-115, KeyDeps.java:266-285, RangeDeps.java:468-495)
 * Query q = one (testTxnId, keysOrRanges.slice(slice)) call: participants [part_off[q], part_off[q+1]), keys
 * (part_is_range[q] = 0: part_start sorted unique) or ranges (1: part_start / part_end sorted, non-overlapping). The
 * call-wide tests are those of acc_recovery_in (started_at, test_dep, test_status, test_kinds, flags).
 * Result per query: the RangeDeps of every (range of the command, TxnId) the map visited, built by Deps.Builder, as an
 * acc_rangedeps_view with query q in place of txn q: the range dictionary is the distinct ranges of the table, dep_txn
 * the first table index holding that TxnId. The boolean recovery predicates are u_off[q+1] > u_off[q]. Copy out with
 * acc_rangedeps_copy_out; the view is valid until the next compute call. */
#define ACC_RCMD_ERASED     1u
#define ACC_RCMD_HAS_DEPS   2u
#define ACC_RCMD_HISTORICAL 4u

typedef struct acc_range_cmds_in {
    uint32_t    n_cmd;
    uint32_t    mem;             /* placement of every array below */
    uint32_t    end_inclusive;   /* 1: Range.EndInclusive (s, e]; 0: Range.StartInclusive [s, e) */
    acc_ts_cols txn_id, execute_at;
    const uint8_t  *status, *flags;
    const uint32_t *rng_off;     /* [n_cmd+1] */
    const uint64_t *rng_start, *rng_end;
    const uint32_t *dep_off;     /* [n_cmd+1] */
    acc_ts_cols     dep_txn;
    const uint64_t *dep_start, *dep_end;
    const uint8_t  *dep_is_key;
} acc_range_cmds_in;

typedef struct acc_recovery_ranges_in {
    uint32_t    n_query;
    uint32_t    mem;
    acc_ts_cols test_txn;        /* [n_query] */
    const uint8_t  *part_is_range;   /* [n_query] */
    const uint32_t *part_off;        /* [n_query+1] */
    const uint64_t *part_start, *part_end;
    uint8_t     started_at, test_dep, test_status, flags;
    int32_t     test_kinds;
} acc_recovery_ranges_in;

int acc_map_reduce_full_ranges(acc_ctx *ctx, const acc_range_cmds_in *cmds, const acc_recovery_ranges_in *q,
                               acc_rangedeps_view *out_view);

/* ---- Recovery merge of LatestDeps replies ----
 * Group g = one recovering txn with replies [grp_off[g], grp_off[g+1]), each a LatestDeps (primitives/LatestDeps.java):
 * reply r owns intervals [iv_off[r], iv_off[r+1]) = RoutingKey ranges [iv_start, iv_end) ascending and disjoint (gaps =
 * null entries), each with a KnownDeps ordinal (local/Status.java:539-578: DepsUnknown 0, DepsProposed 1,
 * DepsCommitted 2, DepsErased 3, DepsKnown 4, NoDeps 5), a Ballot and its coordinatedDeps / localDeps as ids of deps
 * objects (-1 = null). Ids stand for Java object identity: MergeBuilder.tryMergeEqual compares deps by reference
 * (LatestDeps.java:420-435), so equal ids must mean the same object. Deps object d = key_deps / range_deps reply slot d
 * in the acc_rmm_in layout of Deps.merge (n_deps slots). The interval descriptors are host arrays; the deps arrays are in
 * deps_mem. mode ACC_LATEST_PROPOSAL = mergeProposal (:350-358), ACC_LATEST_COMMIT = mergeCommit(txn_id[g],
 * execute_at[g]) (:360-369), which also yields sufficientFor. Ranges are end_inclusive (s, e] or [s, e). */
#define ACC_LATEST_PROPOSAL 0u
#define ACC_LATEST_COMMIT   1u
typedef struct acc_latest_in {
    uint32_t n_groups;
    uint32_t mode;
    const uint32_t *grp_off;          /* [n_groups+1] */
    const uint32_t *iv_off;           /* [n_replies+1] */
    const uint64_t *iv_start, *iv_end;
    const uint8_t  *known;
    acc_ts_cols     ballot;
    const int32_t  *coord_deps;       /* coordinatedDeps id per interval, -1 = null */
    const int32_t  *local_deps;       /* localDeps id per interval, -1 = null */
    acc_ts_cols     txn_id, execute_at;   /* [n_groups], ACC_LATEST_COMMIT only */
    uint32_t        end_inclusive;
    uint32_t        deps_mem;
    uint32_t        n_deps;
    acc_rmm_in      key_deps, range_deps;
} acc_latest_in;

/* deps: per group the merged Deps (device views as acc_deps_merge, copied with acc_rmm_copy_out); sufficientFor per group
 * (mergeCommit): ranges sufficient_start/end[sufficient_off[g] .. sufficient_off[g+1]), HOST pointers owned by the
 * context, valid until its next call. */
typedef struct acc_latest_view {
    acc_deps_merge_view deps;
    uint64_t        total_sufficient;
    const uint64_t *sufficient_off;
    const uint64_t *sufficient_start, *sufficient_end;
} acc_latest_view;

int acc_latest_deps_merge(acc_ctx *ctx, const acc_latest_in *in, acc_latest_view *out_view);

/* ---- Deps wire format: Maelstrom JSON <-> device ----
 * acc_deps_from_json: a batch of JSON documents, each one Deps as Json.DEPS_ADAPTER writes it
 * (accord-maelstrom/.../Json.java:316-398: {"keyDeps":[[datum,[msb,lsb,node]],...],"rangeDeps":[[start,end,[msb,lsb,node]],...]})
 * concatenated in bytes[doc_off[d] .. doc_off[d+1]), parsed on device and built per document (KeyDeps / RangeDeps
 * Builder, Json.java:356-392) into the per-document Deps of `deps` (acc_rmm_view halves; copy with acc_rmm_copy_out).
 * Keys are datums (mael/Datum.java); their codes in `deps` are dense ranks of every datum of the batch in
 * Datum.compareTo order (hash first, COMPARE_BY_HASH), with the dictionary rank -> (Datum.Kind ordinal, null, value,
 * hash). Every Datum.Kind: LONG and DOUBLE as Gson reads a number (nextLong, else nextDouble; the decimal conversion
 * is Double.parseDouble, exactly rounded for up to 19 significant digits -- more give ACC_E_ARG), HASH, and STRING (ASCII text, JSON
 * escapes resolved; two different texts with one hash and equal first 16 characters give ACC_E_ARG). DOUBLE egress is
 * Double.toString (shortest round-trip digits, JDK >= 19), STRING egress Gson's HTML-safe escaping.
 * acc_deps_to_json: the inverse for any acc_rmm_view pair of this context whose key codes index such a dictionary
 * (e.g. a Deps.merge of ingested replies): Gson's compact DEPS_ADAPTER text per group, two-call sizing on need_bytes. */
typedef struct acc_json_in {
    uint32_t mem;
    uint32_t n_docs;
    const uint8_t  *bytes;
    const uint64_t *doc_off;   /* [n_docs+1] */
} acc_json_in;

typedef struct acc_json_deps_view {
    uint32_t n_docs;
    acc_deps_merge_view deps;
    uint64_t n_dict;
    const uint8_t  *dict_kind;   /* Datum.Kind ordinal: STRING 0, LONG 1, DOUBLE 2, HASH 3 */
    const uint8_t  *dict_null;   /* value == null (the +Inf sentinel) */
    const uint64_t *dict_value;  /* LONG: the long; HASH: the hash as u32; DOUBLE: Double.doubleToLongBits;
                                    STRING: byte offset of its text in dict_str */
    const int32_t  *dict_hash;   /* Datum.hash(value) */
    const uint32_t *dict_len;    /* STRING: text length in bytes (ASCII); else 0 */
    const uint8_t  *dict_str;    /* the STRING texts */
} acc_json_deps_view;

int acc_deps_from_json(acc_ctx *ctx, const acc_json_in *in, acc_json_deps_view *out_view);

typedef struct acc_json_out_in {
    uint32_t n_groups;
    acc_rmm_view key_deps, range_deps;      /* device views (key_off null = absent half) */
    uint64_t n_dict;
    const uint8_t  *dict_kind, *dict_null;  /* device */
    const uint64_t *dict_value;
    const uint32_t *dict_len;               /* device; STRING datums need both (as acc_json_deps_view) */
    const uint8_t  *dict_str;
} acc_json_out_in;

typedef struct acc_json_out {
    uint32_t  mem;
    uint64_t  cap_bytes;
    uint64_t  need_bytes;      /* written */
    uint8_t  *bytes;           /* [cap_bytes] */
    uint64_t *doc_off;         /* [n_groups+1] */
} acc_json_out;

int acc_deps_to_json(acc_ctx *ctx, const acc_json_out_in *in, acc_json_out *out);

/* ---- A device-resident CommandsForKey store, updated incrementally ----
 * acc_cfk_update applies CommandsForKey.update(prev, next) (local/CommandsForKey.java:652-706) for every key of every
 * command of `delta`, as SafeCommandStore.updateCommandsForKey does (local/SafeCommandStore.java:217-240; key-domain,
 * globally visible kinds only, others are ignored): an absent TxnId is inserted (executeAt = txnId unless the status
 * carries info), a present one is updated in place and registered on any new keys; a status lower than the stored one
 * is the reference's stale-status IllegalStateException (ACC_E_STATE), an equal status without info changes nothing.
 * The store stays in HBM between calls; acc_cfk_view describes it as an acc_batch_in of DEVICE pointers (txns in TxnId
 * order, keys ascending per txn) that acc_keydeps_batch / acc_map_reduce_full / acc_shard_pack take as they are. The
 * view is valid until the next acc_cfk_update on that store. One store is used by one context at a time. */
typedef struct acc_cfk acc_cfk;
int  acc_cfk_create(acc_ctx *ctx, acc_cfk **out);
void acc_cfk_destroy(acc_cfk *cfk);
int  acc_cfk_update(acc_ctx *ctx, acc_cfk *cfk, const acc_batch_in *delta);
int  acc_cfk_view(acc_ctx *ctx, acc_cfk *cfk, acc_batch_in *out);

/* ---- CommandsForKey.update with each command's deps (local/CommandsForKey.java:657-1149) ----
 * The missing[] and TRANSITIVELY_KNOWN half of CommandsForKey maintenance, on a key-major snapshot: key k (sorted unique
 * codes) holds its TxnInfos [ent_off[k], ent_off[k+1]) in TxnId order (TxnId, executeAt, InternalStatus) and each
 * TxnInfo its TxnInfoWithMissing.missing [miss_off[e], miss_off[e+1]) (sorted raw TxnIds). A batch of command updates
 * is applied in array order to every key each lists, as SafeCommandStore.updateCommandsForKey calls
 * CommandsForKey.update(prev, next) (local/SafeCommandStore.java:217-240): status = the new InternalStatus (0xFF: the
 * save status maps to none, no change), flags bit 0 = acceptedOrCommitted changed since the previous update (the
 * reference returns the CFK unchanged for an equal status otherwise), flags bit 1 = next.status() == AcceptedInvalidate
 * (Commands.acceptInvalidate may move an Accepted command to AcceptedInvalidateWithDefinition = PREACCEPTED: no stale
 * status check, the CFK stays unchanged, CommandsForKey.java:681-688), execute_at = Command.executeAt(), and per
 * (update, key) pair the command's partialDeps().keyDeps.txnIds(key) [dep_off[j], dep_off[j+1]) sorted. Deps the CFK
 * lacks become TRANSITIVELY_KNOWN entries; TxnIds it holds (uncommitted, witnessed) that a dep list lacks go to that
 * TxnInfo's missing[]; committing removes a TxnId from every missing[]. A status going back is ACC_E_STATE (the
 * reference's IllegalStateException) unless flags bit 1 is set. RedundantBefore is empty. The result (keys without entries dropped) is
 * device-resident until the next compute call, and its missing[] is what acc_map_reduce_full's WITH / WITHOUT tests
 * read. */
typedef struct acc_cfk_snap {
    uint32_t mem, n_keys;
    uint64_t n_entries, n_missing;
    const uint64_t *key;         /* [n_keys] */
    const uint32_t *ent_off;     /* [n_keys+1] */
    acc_ts_cols txn_id, execute_at;
    const uint8_t *status;       /* [n_entries] InternalStatus ordinals */
    const uint32_t *miss_off;    /* [n_entries+1] */
    acc_ts_cols missing;         /* [n_missing] */
} acc_cfk_snap;

typedef struct acc_cfk_updates {
    uint32_t mem, n_upd;
    uint64_t n_pairs, n_deps;
    acc_ts_cols txn_id, execute_at;
    const uint8_t *status, *flags;
    const uint32_t *key_off;     /* [n_upd+1] */
    const uint64_t *key;         /* [n_pairs] sorted unique per update */
    const uint32_t *dep_off;     /* [n_pairs+1] */
    acc_ts_cols deps;            /* [n_deps] */
} acc_cfk_updates;

typedef struct acc_cfk_snap_view {
    uint32_t n_keys;
    uint64_t n_entries, n_missing;
    const uint64_t *key;
    const uint32_t *ent_off;
    acc_ts_cols txn_id, execute_at;
    const uint8_t *status;
    const uint32_t *miss_off;
    acc_ts_cols missing;
} acc_cfk_snap_view;

int  acc_cfk_apply(acc_ctx *ctx, const acc_cfk_snap *snap, const acc_cfk_updates *updates, acc_cfk_snap_view *out_view);

/* The key-major CommandsForKey state as the txn-major snapshot acc_map_reduce_full scans, without leaving HBM (the
 * recovery scan of SafeCommandStore.mapReduceFull reads the store's CFKs, local/CommandsForKey.java:553-612): each
 * distinct TxnId of snap is one batch txn (TxnId order) whose keys are the keys holding it, with the executeAt and
 * InternalStatus its TxnInfos carry — equal on every key, as a store's CFKs all see the command's one status, else
 * ACC_E_STATE — and each (txn, key) pair's TxnInfoWithMissing.missing becomes batch indices (a missing TxnId that is no
 * entry of the store: ACC_E_STATE). snap may be an acc_cfk_apply result (mem = ACC_MEM_DEVICE). The output is DEVICE
 * memory owned by the context, valid until the next acc_cfk_snap_to_batch; acc_map_reduce_full reads it in place
 * (its acc_recovery_in with mem = ACC_MEM_DEVICE and this missing_off / missing_txn). */
typedef struct acc_cfk_batch_view {
    acc_batch_in    batch;        /* mem = ACC_MEM_DEVICE */
    const uint32_t *missing_off;  /* [batch.n_pairs+1] */
    const uint32_t *missing_txn;  /* [n_missing] batch indices, sorted per pair */
    uint64_t        n_missing;
} acc_cfk_batch_view;

int  acc_cfk_snap_to_batch(acc_ctx *ctx, const acc_cfk_snap *snap, acc_cfk_batch_view *out_view);

/* One CommandsForKey store for the update with deps and every scan (the reference keeps one
 * CommandsForKey per key that CommandsForKey.update writes and mapReduceActive / mapReduceFull read,
 * local/CommandsForKey.java:614-706, 1085-1149): acc_cfk_apply_deps applies a batch of updates with deps to the acc_cfk
 * store itself — acc_cfk_apply over the store's key-major state, then the store's txn-major view and its per-pair
 * missing[] as txn indices rebuilt from the result — so acc_cfk_view (acc_keydeps_batch, acc_shard_pack), acc_cfk_missing
 * (acc_map_reduce_full: its batch and acc_recovery_in's missing_off / missing_txn with mem = ACC_MEM_DEVICE) and
 * acc_cfk_state (the key-major state in the acc_cfk_apply layout, DEVICE memory) read one state in place, valid until
 * the next update of the store. A rejected batch (ACC_E_STATE / ACC_E_ARG) leaves the store unchanged. A store keeps
 * missing[] from its first acc_cfk_apply_deps on; acc_cfk_update (status-only, no missing[]) is then ACC_E_STATE, and
 * acc_cfk_apply_deps on a store holding acc_cfk_update state is ACC_E_STATE. The store adopts the call's result
 * arrays from the context (no copies) and hands its previous arrays to the context for its next results. Keys with
 * many updates in one batch (more than ACC_CFK_HOT, default 64, snapshot + update elements) are computed by the
 * data-parallel closed form of the replay (acc_cfk_apply too); results are the same. */
int  acc_cfk_apply_deps(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_updates *updates);
int  acc_cfk_state(acc_ctx *ctx, acc_cfk *cfk, acc_cfk_snap *out);
int  acc_cfk_missing(acc_ctx *ctx, acc_cfk *cfk, acc_cfk_batch_view *out);

/* RedundantBefore on the resident store: the prune that keeps it a steady-state store. A CommandStore advances its
 * RedundantBefore as sync points apply (local/RedundantBefore.java: a ReducingRangeMap of Entries merged with max), and
 * every CommandsForKey follows on its next access (SafeCommandStore.maybeTruncate, local/SafeCommandStore.java:158-164 ->
 * CommandsForKey.withRedundantBefore, local/CommandsForKey.java:1654-1684). An Entry is modelled by its
 * shardRedundantBefore alone: the store owns one map RB, key code -> TxnId, all zero (TxnId.NONE) where nothing is set.
 * acc_cfk_redundant_before first replaces RB by the pointwise Timestamp.compareTo maximum of RB and the input
 * (RedundantBefore.merge: a lower bound is absorbed, never an error); range j covers the key codes (s, e] with
 * end_inclusive = 1, [s, e) with 0, and holds bound[j]. Then every stored key k with RB_new(k) > RB_old(k) = b is
 * pruned: pos = the lower bound of b among the key's TxnIds (insertPos(0, b); an entry whose TxnId compares equal to b
 * stays), the entries [0, pos) are dropped, and if pos != 0 every surviving entry's missing[] loses its prefix below b
 * (Arrays.binarySearch(missing, b); an id equal to b stays). A key whose bound did not rise is unchanged even if it
 * holds entries below its bound (the newRedundantBefore.equals(redundantBefore) early return: update inserts entries
 * without looking at the bound, and they stay until the bound next rises). A key left without entries leaves the state
 * (the "keys without entries dropped" convention of acc_cfk_apply). The txn-major view (acc_cfk_view) and the per-pair
 * missing[] indices (acc_cfk_missing) are rebuilt from the result exactly as acc_cfk_apply_deps rebuilds them, and the
 * new arrays adopted the same way: a TxnId dropped from all its keys leaves the view, and later dep_txn indices refer to
 * the new view. If no stored key's bound rises, no array is rewritten and every view stays valid.
 * Under a non-empty map acc_cfk_apply_deps ignores, per (update, key) pair, the deps below RB(key)
 * (deps.find(redundantBefore.shardRedundantBefore()), :1088-1089): they create no TRANSITIVELY_KNOWN entries and play
 * no part in the missing merge. The scans (acc_cfk_keydeps*, acc_cfk_map_reduce_full) do not consult the bound, as in
 * the reference (:553-650): they read the pruned state.
 * Errors, store and map unchanged: ranges unsorted, overlapping (rng_end[j-1] > rng_start[j]) or with start >= end,
 * end_inclusive > 1, end_inclusive differing from an earlier call's: ACC_E_ARG; a non-empty status-only store
 * (acc_cfk_update): ACC_E_STATE. An empty store records the map, and keys that appear later honour it (maybeTruncate on
 * a fresh CFK). n_ranges == 0 is a no-op.
 * Stats: cfk.redundant_keys_advanced, cfk.redundant_entries_dropped, cfk.redundant_missing_dropped; cfk.deps_trimmed
 * (set by acc_cfk_apply_deps); cfk.redundant_prune_us / cfk.redundant_view_us (stream time of the prune passes and of
 * the view rebuild).
 * RedundantBefore.collectDeps (:418-421: the (range, bound) range deps added to PreAccept results) is
 * acc_rcmd_partial_rangedeps, read from the range-command store's copy of the map. Out of scope: the
 * locally-redundant, bootstrap and stale fields of an Entry, and registerHistorical. (The range-command store is
 * pruned by its own call, acc_rcmd_redundant_before below.)
 * acc_cfk_redundant_view describes the map: closed intervals over the key codes, ascending and disjoint (adjacent
 * intervals with equal bounds are one), with the bound of each. */
typedef struct acc_cfk_redundant_in {
    uint32_t mem, n_ranges;          /* ACC_MEM_HOST or ACC_MEM_DEVICE for every pointer */
    uint32_t end_inclusive;          /* the store's Range bound type, as acc_cfk_mixed_queries */
    const uint64_t *rng_start, *rng_end;   /* [n_ranges] sorted, non-overlapping, start < end */
    acc_ts_cols bound;               /* [n_ranges] shardRedundantBefore (a TxnId) of each range */
} acc_cfk_redundant_in;
int  acc_cfk_redundant_before(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_redundant_in *in);

typedef struct acc_cfk_redundant_map {   /* DEVICE pointers, valid until the next acc_cfk_redundant_before */
    uint64_t n;  uint32_t end_inclusive;
    const uint64_t *st, *en;         /* closed intervals over the key codes, ascending, disjoint */
    acc_ts_cols bound;
} acc_cfk_redundant_map;
int  acc_cfk_redundant_view(acc_ctx *ctx, acc_cfk *cfk, acc_cfk_redundant_map *out);

/* PreAccept.calculatePartialDeps' key half for a batch of queries against a resident store: query q runs
 * CommandsForKey.mapReduceActive (local/CommandsForKey.java:614-650) on the CFK of each of its keys with
 * startedBefore = execute_at[q], testKind = txn_id[q].kind().witnesses(), and txn_id[q] itself never emitted.
 * The store (one that acc_cfk_apply_deps maintains, or an empty one) is read in place: its key-major segments are
 * scanned where they lie, nothing of it is re-sorted and the deps of stored txns are not recomputed, so the work is
 * the queries' (query, key) pairs plus the segment prefixes (entries with TxnId < executeAt) they read.
 * Per (query, key) pair, with S = the query's executeAt: end = the first entry with TxnId >= S (Timestamp.compareTo);
 * M = the largest executeAt among the entries below end that are COMMITTED / STABLE / APPLIED Writes with executeAt < S
 * (the closed form of the FAST bisection of committed[] and the walk down to a Write; none: nothing is pruned); every
 * entry below end is emitted whose kind the query's kind witnesses, whose status is neither TRANSITIVELY_KNOWN nor
 * INVALID_OR_TRUNCATED, that is not a committed-class entry with executeAt < M, and whose TxnId is not
 * Timestamp.equals to the query's. A key without a CFK contributes nothing.
 * Tie rule: the closed form and the reference's bisection can differ only when two or more committed-class entries of
 * one key have an executeAt compare-equal to S (the bisection may land on either); the reference never holds such a
 * state (executeAt is unique per command). A pair that sees two or more fails the call with ACC_E_STATE.
 * The result is an acc_keydeps_view with n_txn = n_query in the acc_keydeps_batch layout per query: key_idx into the
 * query's own keys (keys with at least one dep), kd_key their codes, dep_txn = KeyDeps.txnIds as indices into the
 * store's acc_cfk_view txn order, ascending. It is the context's last KeyDeps result (acc_keydeps_copy_out copies it),
 * valid until the next compute call on the context. The store is not modified. Errors: a range-domain or
 * invalid-kind TxnId, offsets that do not start at 0 / decrease / end off n_pairs, unsorted or duplicate keys of a
 * query: ACC_E_ARG; a LocalOnly TxnId (Kind.witnesses() throws) or a non-empty status-only store (acc_cfk_update):
 * ACC_E_STATE. An empty store, n_query == 0 and queries without keys give empty results. */
typedef struct acc_cfk_queries {
    uint32_t    n_query, mem;      /* ACC_MEM_HOST or ACC_MEM_DEVICE for every pointer */
    uint64_t    n_pairs;           /* key_off[n_query] */
    acc_ts_cols txn_id;            /* [n_query] any TxnId, store member or not */
    acc_ts_cols execute_at;        /* [n_query]; execute_at.msb == NULL: executeAt = txnId for every query */
    const uint32_t *key_off;       /* [n_query+1] */
    const uint64_t *key_code;      /* [n_pairs] sorted unique per query (Keys) */
} acc_cfk_queries;
int  acc_cfk_keydeps(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_queries *q, acc_keydeps_view *out_view);

/* acc_cfk_keydeps for queries of both domains: the Range case of InMemoryCommandStore.mapReduceForKey
 * (impl/InMemoryCommandStore.java:274-289) next to its Key case. A key-domain query (TxnId domain bit 0) lists keys
 * and is answered exactly as by acc_cfk_keydeps. A range-domain query (domain bit 1: sync points, range reads) lists
 * ranges and runs the same per-(query, key) scan — prefix below S = executeAt, M, the emit switch, the Timestamp.equals
 * self-exclusion, the tie rule — on every CFK of commandsForKey.subMap(start, startInclusive, end, endInclusive) of each
 * of its ranges: the store keys k with s < k <= e (end_inclusive = 1) or s <= k < e (0), range by range in order; the
 * ranges of a query do not overlap, so its covered keys ascend strictly. A range txn is no CFK member, and a range that
 * covers no store key contributes nothing. The store's keys are sorted, so the keys a range covers are one run of them
 * and their entries one span of the entry columns: only those are read, the store is not re-sorted or modified.
 * Result as acc_cfk_keydeps; for a range-domain query key_idx indexes the list of its covered CFK keys in range order
 * (the acc_keydeps_mixed convention) and kd_key holds their codes.
 * lane_seg: covered keys whose whole segment holds at most lane_seg entries (1..256) are scanned one lane per key,
 * consecutive lanes on consecutive keys, instead of one wave per (query, key); ACC_CFQ_LANE_NONE: never; 0: the library
 * default. Results do not depend on it.
 * Errors on top of acc_cfk_keydeps': a range-domain query that lists keys, a key-domain query that lists ranges, a
 * range with start >= end, ranges of a query out of order or overlapping (rng_end[j-1] > rng_start[j]; touching ranges
 * are allowed), rng_off not starting at 0 / decreasing / ending off n_ranges, end_inclusive > 1, lane_seg above 256 and
 * not ACC_CFQ_LANE_NONE: ACC_E_ARG; more than 2^32 - 2 (query, key) pairs after expansion: ACC_E_CAP. */
#define ACC_CFQ_LANE_NONE 0xFFFFFFFFu
typedef struct acc_cfk_mixed_queries {
    uint32_t    n_query, mem;          /* ACC_MEM_HOST or ACC_MEM_DEVICE for every pointer */
    uint64_t    n_pairs;               /* key_off[n_query] */
    uint64_t    n_ranges;              /* rng_off[n_query] */
    acc_ts_cols txn_id;                /* [n_query]; domain bit (lsb & 1) picks keys or ranges */
    acc_ts_cols execute_at;            /* msb == NULL: executeAt = txnId for every query */
    const uint32_t *key_off;           /* [n_query+1] */
    const uint64_t *key_code;          /* [n_pairs] sorted unique per key-domain query */
    const uint32_t *rng_off;           /* [n_query+1] */
    const uint64_t *rng_start, *rng_end; /* [n_ranges] per range-domain query: sorted, non-overlapping, start < end */
    uint32_t    end_inclusive;         /* 1: (s, e]; 0: [s, e) — the store's Range bound type */
    uint32_t    lane_seg;              /* see above; 0: the library default */
} acc_cfk_mixed_queries;
int  acc_cfk_keydeps_mixed(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_mixed_queries *q, acc_keydeps_view *out_view);

/* The recovery scans on the resident store: acc_map_reduce_full's questions (BeginRecovery's four,
 * messages/BeginRecovery.java:330-380 -> SafeCommandStore.mapReduceFull -> CommandsForKey.mapReduceFull,
 * local/CommandsForKey.java:553-612) asked of the live CommandsForKey of the recovered txn's keys and of nothing else,
 * as the reference does: the key-major segments and each entry's missing[] (raw TxnIds, sorted) are read in place; the
 * store is not re-ranked, re-sorted or rebuilt, and the per-pair missing[] indices of acc_cfk_missing are not read.
 * Per (query, key) pair over the key's segment, with X = test_txn[q] and every comparison Timestamp.compareTo:
 * pos = the lower bound of X among the segment's TxnIds (Arrays.binarySearch's index or insert point, :561-562),
 * isKnown = the entry at pos compares equal to X; a pair with !isKnown and test_dep = WITH contributes nothing (:563-564).
 * The window is [segment start, pos) for STARTED_BEFORE, [pos, segment end) for STARTED_AFTER (X's own entry included
 * when it is a member) and the whole segment for ANY (:566-575). An entry of the window is visited iff its kind
 * ((lsb >> 1) & 7) is in the Kinds mask (:580), it passes the status test (:581-596: IS_PROPOSED = ACCEPTED or
 * COMMITTED; IS_STABLE = STABLE <= s < INVALID_OR_TRUNCATED; ANY_STATUS = not TRANSITIVELY_KNOWN), for WITH / WITHOUT
 * its status hasInfo (ACCEPTED..APPLIED), its executeAt > X and (X is absent from its missing[]) == (test_dep == WITH)
 * (:597-605; a binary search of X in the entry's missing[]), and with ACC_FULL_EXECUTES_AFTER its executeAt > X
 * (BeginRecovery.java:339-341).
 * A key-domain query (TxnId domain bit 0) lists keys; a key without a CFK contributes nothing. A range-domain query
 * (domain bit 1) lists ranges and runs the same scan on every store key each range covers, bounds by end_inclusive,
 * range by range: mapReduceForKey's Range case (impl/InMemoryCommandStore.java:274-289), which mapReduceFull (:874-881)
 * uses exactly as mapReduceActive does. There is no special case for it: a range-domain X is a member of a key only if
 * a stored TxnId compares equal to it.
 * Result per query: the Deps.Builder KeyDeps of every visited (key, TxnId) in the acc_keydeps_view layout of
 * acc_cfk_keydeps / acc_cfk_keydeps_mixed: key_idx into the query's own keys (its covered keys in range order for a
 * range-domain query), kd_key their codes, dep_txn = indices into the store's acc_cfk_view txn order, ascending. It is
 * the context's last KeyDeps result (acc_keydeps_copy_out copies it). The boolean predicates
 * (hasAcceptedOrCommittedStartedAfterWithoutWitnessing, hasStableExecutesAfterWithoutWitnessing) are
 * u_off[q+1] > u_off[q]. The store is not modified. The one-wave / sorting build tiers split at acc_opts.cfq_wave_cap.
 * Errors: the participant validation of acc_cfk_keydeps_mixed (domain / participant mismatch, offsets, unsorted or
 * duplicate keys, bad ranges, end_inclusive > 1: ACC_E_ARG; 2^32 - 1 or more pairs after expansion: ACC_E_CAP);
 * started_at, test_dep or test_status > 2, unknown flags bits, test_kinds > 0x3F: ACC_E_ARG; with test_kinds == -1 a
 * LocalOnly X (Kind.witnessedBy() throws): ACC_E_STATE, an invalid kind ordinal: ACC_E_ARG (with a Kinds mask X's kind
 * is not read, as in acc_map_reduce_full); a non-empty status-only store (acc_cfk_update): ACC_E_STATE. An empty
 * store, n_query == 0 and queries without participants give empty results; a failed call leaves the context usable.
 * The range-command half of the same questions is acc_rcmd_map_reduce_full below, which takes this query struct and
 * answers from the resident range-command store (acc_rcmd); acc_map_reduce_full_ranges answers them over a table the
 * caller passes whole. */
typedef struct acc_cfk_recovery_in {
    uint32_t    n_query, mem;            /* ACC_MEM_HOST or ACC_MEM_DEVICE for every pointer */
    uint64_t    n_pairs, n_ranges;       /* key_off[n_query], rng_off[n_query] */
    acc_ts_cols test_txn;                /* [n_query] testTxnId: any TxnId, store member or not */
    const uint32_t *key_off;  const uint64_t *key_code;              /* key-domain queries: sorted unique keys */
    const uint32_t *rng_off;  const uint64_t *rng_start, *rng_end;   /* range-domain queries */
    uint32_t    end_inclusive;           /* the store's Range bound type, as acc_cfk_mixed_queries */
    uint8_t     started_at, test_dep, test_status, flags;   /* exactly acc_recovery_in's */
    int32_t     test_kinds;              /* Kinds mask, or -1: testTxnId.kind().witnessedBy() */
} acc_cfk_recovery_in;
int  acc_cfk_map_reduce_full(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_recovery_in *q, acc_keydeps_view *out_view);

/* ---- Execution releases from the resident CommandsForKey store ----
 * acc_cfk_notify reads the key-major state (acc_cfk_state: status, executeAt, missing[] of every TxnInfo) and answers,
 * for every asked key, what CommandsForKey.notify (local/CommandsForKey.java:1501-1635, behind notifyAndUpdatePending,
 * :1163-1215) tells Commands.removeWaitingOnKeyAndMaybeExecute (local/Commands.java:859-876): the derived fields of the
 * CommandsForKey constructor (:422-470) and the events of the full-range scan notify(AnyGloballyVisible, 0,
 * committed.length). APPLIED and INVALID_OR_TRUNCATED entries pass the scan's counters (:1524-1526), so a scan from index
 * 0 equals a scan from `next`; every window notifyAndUpdatePending asks for starts at next.executeAt or Timestamp.NONE,
 * so each reference call's events are a prefix, in committed[] order, of the events given here (ev_pos cuts it); `kinds`
 * filters only the COMMITTED branch. The store is not modified.
 * Per key, over its entries in TxnId order (Timestamp.compareTo throughout): an entry is uncommitted below COMMITTED
 * (ordinals 0..3), committed-class when COMMITTED, STABLE or APPLIED; INVALID_OR_TRUNCATED is neither.
 *   min_uncommitted  the first uncommitted entry;
 *   next             the COMMITTED or STABLE entry with the least executeAt, ties to the lower TxnId (strict >, :442-445);
 *   next_write       the same among Writes; each of the two is null when min_uncommitted < its executeAt (:451-458);
 *   committed[]      the committed-class entries sorted by executeAt, ties in TxnId order (a stable sort).
 * For a STABLE entry T of kind k with executeAt X: c[W], c[R], c[S] count the COMMITTED and STABLE entries before T in
 * committed[] by class (Write; Read; SyncPoint or ExclusiveSyncPoint), u[.] the uncommitted entries with TxnId < X by
 * the same classes (TRANSITIVELY_KNOWN and HISTORICAL ones by their kind: the closed form of the uncommittedIndex
 * backfill, :1540-1570). expect = (c+u)[W] for a Read, plus (c+u)[R] for a Write, plus (c+u)[S] for a sync point.
 * missingCount = |missing(T)|, less the ids below min_uncommitted when both exist (:1596-1603). T is released iff
 * expect == missingCount: an ACC_NOTIFY_RELEASE event. Every COMMITTED entry gives an ACC_NOTIFY_WAITING_TO_EXECUTE
 * event (the progress-log call, :1528-1537); a STABLE entry that is held gives none.
 * Input: key_code sorted unique (NULL: every key of the store, n_keys ignored); a key without a CFK gives an empty row.
 * Output (DEVICE pointers, valid until the context's next compute call): per row min_uncommitted / next / next_write as
 * entry indices into the acc_cfk_state entry columns (ACC_NOTIFY_NONE: null) and ev_off; per event, in TxnId order
 * within the row, ev_entry (acc_cfk_state entry), ev_txn (index into the acc_cfk_view txn order, the dep_txn convention
 * of acc_cfk_keydeps), ev_kind and ev_pos (the entry's index in committed[], applied entries included); per view txn
 * rel_keys = the number of asked keys that release it, to compare with its set WaitingOn key bits.
 * tier: the bumped (executeAt != TxnId) committed-class entries of a key are ranked by a lane, a wave or the store-wide
 * sort by their number; a non-zero tier forces one (where the key fits it, else the sort). Results do not depend on it.
 * Errors: mem, an unknown tier, unsorted or duplicate keys: ACC_E_ARG; a LocalOnly or EphemeralRead entry in an asked
 * key (the reference's illegalState), a non-empty status-only store (acc_cfk_update): ACC_E_STATE. An empty store and
 * n_keys == 0 give empty results; a failed call leaves the context usable. Stats: cfk.notify_keys, cfk.notify_candidates
 * (COMMITTED or STABLE entries of the asked keys), cfk.notify_releases, cfk.notify_sorted, cfk.notify_us.
 * Out of scope: the progress-log side of notifyWaitingOnCommit (min_uncommitted is given for the caller to do it); the
 * range-command half of WaitingOn and the WaitingOn key bits themselves (acc_waiting_* below takes these releases).
 * (Unmanaged pending records: acc_cfk_register_unmanaged / acc_cfk_notify_unmanaged below.) */
#define ACC_NOTIFY_WAITING_TO_EXECUTE 0
#define ACC_NOTIFY_RELEASE            1
#define ACC_NOTIFY_NONE               0xFFFFFFFFu
#define ACC_NOTIFY_TIER_LANE          1
#define ACC_NOTIFY_TIER_WAVE          2
#define ACC_NOTIFY_TIER_SORT          3
typedef struct acc_cfk_notify_in {
    uint32_t mem, n_keys;
    const uint64_t *key_code;   /* sorted unique; NULL: every key of the store */
    uint32_t tier;              /* 0: library default; other values force one kernel tier (tests) */
} acc_cfk_notify_in;
typedef struct acc_cfk_notify_view {
    uint32_t n_keys, n_txn;
    uint64_t n_events;
    const uint32_t *min_uncommitted, *next, *next_write;   /* [n_keys] */
    const uint64_t *ev_off;                                /* [n_keys + 1] */
    const uint32_t *ev_entry, *ev_txn, *ev_pos;            /* [n_events] */
    const uint8_t  *ev_kind;                               /* [n_events] */
    const uint32_t *rel_keys;                              /* [n_txn] */
} acc_cfk_notify_view;
int  acc_cfk_notify(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_notify_in *in, acc_cfk_notify_view *out);

/* ---- Unmanaged pending records of the resident CommandsForKey store ----
 * Commands that wait on keys without being CommandsForKey members: range-domain txns (range reads, every sync point) and
 * key-domain EphemeralRead / LocalOnly. When one becomes Stable, SafeCommandStore.updateCommandsForKey
 * (local/SafeCommandStore.java:246-268) calls CommandsForKey.registerUnmanaged (local/CommandsForKey.java:1406-1498) on
 * every key it waits on, and from then on notifyAndUpdatePending (:1206-1214) runs notifyUnmanaged (:1270-1316) after
 * each update. The store keeps the records (Unmanaged, :140-184) in a pending table in DEVICE memory, freed by
 * acc_cfk_destroy: per record the key code (records name their key by code and survive the key leaving the state),
 * pending (ACC_UNM_COMMIT / ACC_UNM_APPLY), waiting_until, the waiter's TxnId and executeAt (raw bits) and, for a COMMIT
 * record, the waiter's dep list for that key (an APPLY record is never re-evaluated and keeps none). Records stay in
 * registration order (call order, then pair order); compaction is stable and a record that moves from COMMIT to APPLY
 * keeps its slot: every threshold test is a per-record predicate, so nothing needs the Unmanaged.compareTo order.
 * acc_cfk_unmanaged_view describes the table (DEVICE pointers, valid until the store's next acc_cfk_register_unmanaged
 * or acc_cfk_notify_unmanaged). acc_cfk_redundant_before carries the table unchanged (the reference's "TODO filter
 * pending unmanageds", :1682).
 *
 * acc_cfk_register_unmanaged: `in` is acc_cfk_updates without status / flags: per waiter TxnId, executeAt and keys
 * (sorted unique), per (waiter, key) pair partialDeps().keyDeps.txnIds(key) (sorted unique). Every pair is evaluated
 * against the store as it stands before the call (:1415-1498; outcomes do not depend on pair order: a dep another pair
 * inserts as TRANSITIVELY_KNOWN counts as uncommitted absent or present). Deps below RB(key), the store's
 * RedundantBefore map, are skipped (a dep equal to the bound stays); none left: ACC_UNM_READY. For each remaining dep:
 * absent from the key's entries: not ready, not waitingToApply, and the dep is missing; present below COMMITTED: not
 * ready, not waitingToApply; otherwise (INVALID_OR_TRUNCATED included), if the waiter's kind awaitsOnlyDeps
 * (ExclusiveSyncPoint, EphemeralRead; primitives/Txn.java:211-214) or the entry's executeAt is below the waiter's:
 * ready &= status >= APPLIED, executesAt = max(executesAt, entry.executeAt). Outcome: ready: ACC_UNM_READY (the shim's
 * removeWaitingOn; no record, nothing inserted); else waitingToApply: ACC_UNM_PENDING_APPLY with waiting_until =
 * executesAt; else ACC_UNM_PENDING_COMMIT with waiting_until = the pair's last dep. The distinct missing (key, TxnId) of
 * all not-ready pairs are merged into the key-major state as TxnInfo.create(id, TRANSITIVELY_KNOWN) (executeAt = TxnId,
 * empty missing[]; other entries' missing[] untouched, :1454-1471; a key without a CFK is created) and the txn-major
 * view is rebuilt as acc_cfk_apply_deps rebuilds it; with nothing missing no store array is rewritten and every view
 * stays valid. The view holds one status per TxnId: a missing dep that the store holds on another key with a status
 * other than TRANSITIVELY_KNOWN fails the call with ACC_E_STATE. Then the new records are appended.
 * `out` (DEVICE pointers, valid until the context's next compute call): per pair outcome and until (zeros for READY),
 * and n_inserted. For an awaitsOnlyDeps waiter the caller raises WaitingOn.executeAtLeast to `until` of each
 * PENDING_APPLY pair (:1476-1484).
 * tier: pairs with at most UM_LANE_MAX (16) deps at or above the bound are evaluated by one lane, longer ones by one
 * wave; a non-zero tier forces one for every pair. Results do not depend on it.
 * Errors leave the store and the table unchanged. ACC_E_ARG: mem; offsets not starting at 0, decreasing, or not ending
 * at the counts; keys of a waiter not sorted unique; deps of a pair not sorted unique; a kind ordinal above 5; a managed
 * waiter (key domain and a globally visible kind); the same waiter TxnId twice in one call; an unknown tier.
 * ACC_E_STATE: a non-empty status-only store (acc_cfk_update). ACC_E_CAP: the table's records or deps would reach
 * 2^32 - 1. n_waiters == 0 is a no-op. Registering a (waiter, key) at most once across calls is the caller's contract,
 * as in the reference.
 *
 * acc_cfk_notify_unmanaged: key_code sorted unique (NULL: every key that has a record). It first runs acc_cfk_notify on
 * those keys for min_uncommitted and next (and inherits its errors), then per record of an asked key applies :1206-1212
 * and :1270-1316 in closed form. COMMIT step: Tc = minUncommitted's TxnId (Timestamp.MAX when null); a COMMIT record with
 * waiting_until < Tc is re-evaluated by updatePending (:1333-1388): deps below the current RB(key) are skipped, the walk
 * stops at the key's last entry (deps beyond it are ignored), the test is awaitsOnlyDeps || executeAt <
 * waiterExecuteAt with no COMMITTED check; a dep that is absent while a later entry exists is the reference's
 * illegalState: ACC_E_STATE, table unchanged. The record is either released or becomes an APPLY record in its slot with
 * waiting_until = executesAt, its deps dropped. The step runs unconditionally (when nothing newly committed no record
 * qualifies: a COMMIT record's last dep is at or above an uncommitted entry). APPLY step, on the table after the COMMIT
 * step, only if minUncommitted == null || next != null: Ta = next's executeAt (MAX when next is null); APPLY records
 * with waiting_until < Ta are released. Both thresholds are exclusive.
 * Output (DEVICE pointers, valid until the context's next compute call): one event per affected record in table order:
 * ev_kind (ACC_UNM_EV_TO_APPLY / ACC_UNM_EV_RELEASE), ev_flags (bit 0: re-evaluated from COMMIT in this call), ev_key,
 * ev_txn, ev_until (the record's APPLY waiting_until, zeros if it never had one); n_events, and n_rec after the stable
 * compaction. RELEASE is removeWaitingOn(txnId, key); with bit 0 set, an awaitsOnlyDeps waiter and a non-zero ev_until
 * the caller also calls updateExecuteAtLeast(ev_until) (:1372-1381). A call that moves nothing leaves the table and
 * its view as they are.
 * Stats: cfk.unmanaged_pairs, _ready, _pending_commit, _pending_apply, _tk_inserted, _records, _register_us
 * (register); cfk.unmanaged_reevaluated, _released, _records, _notify_us (notify).
 * Out of scope: the progress-log side of notifyWaitingOnCommit; updatePendingAsync's load scheduling (the device always
 * has the command's deps in the record); registerHistorical; the range-command half of WaitingOn (acc_waiting_* below,
 * whose release pairs also take the `until` values given here). */
#define ACC_UNM_COMMIT          0
#define ACC_UNM_APPLY           1
#define ACC_UNM_READY           0
#define ACC_UNM_PENDING_COMMIT  1
#define ACC_UNM_PENDING_APPLY   2
#define ACC_UNM_TIER_LANE       1
#define ACC_UNM_TIER_WAVE       2
#define ACC_UNM_EV_TO_APPLY     0
#define ACC_UNM_EV_RELEASE      1
typedef struct acc_cfk_unmanaged_in {
    uint32_t mem, n_waiters;     /* ACC_MEM_HOST or ACC_MEM_DEVICE for every pointer */
    uint64_t n_pairs, n_deps;
    acc_ts_cols txn_id, execute_at;   /* [n_waiters] */
    const uint32_t *key_off;     /* [n_waiters+1] */
    const uint64_t *key;         /* [n_pairs] sorted unique per waiter */
    const uint32_t *dep_off;     /* [n_pairs+1] */
    acc_ts_cols deps;            /* [n_deps] sorted unique per pair */
    uint32_t tier;               /* 0: library default; ACC_UNM_TIER_LANE / _WAVE force one kernel tier (tests) */
} acc_cfk_unmanaged_in;
typedef struct acc_cfk_unmanaged_out {
    uint64_t n_pairs, n_inserted;
    const uint8_t *outcome;      /* [n_pairs] ACC_UNM_READY / _PENDING_COMMIT / _PENDING_APPLY */
    acc_ts_cols until;           /* [n_pairs] waiting_until; zeros for READY */
} acc_cfk_unmanaged_out;
typedef struct acc_cfk_unmanaged_table {   /* DEVICE pointers */
    uint32_t n_rec;
    uint64_t n_deps;
    const uint64_t *key;         /* [n_rec] */
    const uint8_t  *pending;     /* [n_rec] ACC_UNM_COMMIT / ACC_UNM_APPLY */
    acc_ts_cols until, txn_id, execute_at;
    const uint32_t *dep_off;     /* [n_rec+1] */
    acc_ts_cols deps;            /* [n_deps] */
} acc_cfk_unmanaged_table;
typedef struct acc_cfk_unmanaged_notify_in {
    uint32_t mem, n_keys;
    const uint64_t *key_code;    /* sorted unique; NULL: every key that has a record */
} acc_cfk_unmanaged_notify_in;
typedef struct acc_cfk_unmanaged_events {
    uint32_t n_events, n_rec;
    const uint8_t *ev_kind, *ev_flags;   /* [n_events] */
    const uint64_t *ev_key;
    acc_ts_cols ev_txn, ev_until;
} acc_cfk_unmanaged_events;
int  acc_cfk_register_unmanaged(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_unmanaged_in *in, acc_cfk_unmanaged_out *out);
int  acc_cfk_notify_unmanaged(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_unmanaged_notify_in *in, acc_cfk_unmanaged_events *out);
int  acc_cfk_unmanaged_view(acc_ctx *ctx, acc_cfk *cfk, acc_cfk_unmanaged_table *out);

/* ---- A device-resident range-command store and the RangeDeps of new txns ----
 * The other half of PreAccept.calculatePartialDeps beside acc_cfk_keydeps_mixed: the deps on the store's range commands
 * (InMemorySafeStore.mapReduceActive -> mapReduceRangesInternal, impl/InMemoryCommandStore.java:863-870, 883-960). The
 * reference keeps rangeCommands as a live TreeMap<TxnId, RangeCommand> that update() adds to (:739-762) and asks it about
 * the incoming txn only; acc_rcmd is that map in HBM, one per CommandStore, one Range bound type fixed at creation
 * (end_inclusive: 1 = (s, e], 0 = [s, e)). Per TxnId in Timestamp.compareTo order it holds the TxnId's raw bits (those of
 * its first update), an erased flag (saveStatus >= Erased) and its Ranges (sorted, non-overlapping), and beside the table
 * the stabbing index over the ranges of the non-erased commands: the dictionary of distinct stored ranges in
 * Range::compare order and the entries in (width class, start) order, as acc_rangedeps_batch builds them per call.
 *
 * acc_rcmd_update applies the updates in array order, as InMemorySafeStore.update does per command: update u is a
 * TxnId, flags[u] and the ranges [rng_off[u], rng_off[u+1]). A key-domain TxnId is ignored (txnId.domain() != Range ->
 * return; stat rcmd.skipped_key_domain). A non-erased update inserts the TxnId when absent (computeIfAbsent) and sets
 * ranges = ranges == null ? add : ranges.with(add) (RangeCommand.update :524-539; Ranges.with =
 * AbstractRanges.union(MERGE_OVERLAPPING), primitives/AbstractRanges.java:439-585 — what acc_ranges_with computes, replayed
 * step by step on the device: it has a superset short-cut and absorbs touching ranges only inside a group a strict overlap
 * opened, so [1,3) with [3,5) with [2,4) = {[1,3),[3,5)} while [1,3) with [2,4) with [3,5) = {[1,5)}; a TxnId listed
 * several times in one batch folds in array order). An update with ACC_RCMD_ERASED marks the TxnId erased, inserting a
 * row without ranges when absent; its listed ranges are ignored. An erased command is never visited (:891-892): its
 * ranges leave the table and the dictionary, and every later update of it changes nothing (stat rcmd.erased_ignored). A
 * command may hold no ranges. Two TxnIds that are Timestamp.equals are one command. Errors (ACC_E_ARG): an invalid kind
 * ordinal, a flags bit other than ACC_RCMD_ERASED, ranges of an update not sorted / overlapping / start >= end, rng_off
 * not starting at 0 / decreasing / not ending at n_ranges. A rejected batch leaves the store unchanged; n_upd == 0 is a
 * no-op. Each update rebuilds the index once from the resident table. One store is used by one context at a time.
 *
 * acc_rcmd_view describes the table: DEVICE pointers, valid until the next acc_rcmd_update of the store.
 *
 * acc_rcmd_rangedeps takes the query struct of acc_cfk_keydeps_mixed, so one query batch serves both halves
 * (end_inclusive must equal the store's: ACC_E_ARG; lane_seg is ignored). For query q with S = its executeAt
 * (execute_at.msb == NULL: S = TxnId) it visits every stored command C (:888-960 with ANY_STATUS / ANY_DEPS) that is not
 * erased, has C.txnId < S strictly (STARTED_BEFORE, :901-902), whose kind q.kind().witnesses() holds, and whose TxnId is
 * not Timestamp.equals to q's; each of C's ranges that contains one of q's keys (Range.contains with the bound type) or
 * intersects one of q's ranges (compareIntersecting == 0) is collected per Range (a TreeMap by Range::compare, each list
 * in TxnId order without consecutive duplicates) and built by RangeDeps.Builder. The result is an acc_rangedeps_view with
 * n_txn = n_query in the acc_rangedeps_batch layout: range_id are ids into the store's dictionary (rng_start / rng_end),
 * dep_txn indices into the acc_rcmd_view table order, ascending. It is the context's last RangeDeps result
 * (acc_rangedeps_copy_out copies it), valid until the next RangeDeps compute call on the context or the next update of
 * the store. The store is not modified. Errors as acc_cfk_keydeps_mixed: domain / participant mismatch, bad ranges or
 * offsets, unsorted keys, n_pairs + n_ranges >= 2^32 - 1: ACC_E_ARG; a LocalOnly query: ACC_E_STATE. An empty store,
 * n_query == 0 and queries without participants give empty results.
 * Not modelled: historicalRangeCommands, which the reference's mapReduceActive also visits (:962-1004);
 * acc_rangedeps_batch does not model them either. */
typedef struct acc_rcmd acc_rcmd;

typedef struct acc_rcmd_updates {
    uint32_t    n_upd, mem;            /* ACC_MEM_HOST or ACC_MEM_DEVICE for every pointer */
    uint64_t    n_ranges;              /* rng_off[n_upd] */
    acc_ts_cols txn_id;                /* [n_upd]; may repeat */
    const uint8_t  *flags;             /* [n_upd] 0 or ACC_RCMD_ERASED */
    const uint32_t *rng_off;           /* [n_upd+1] */
    const uint64_t *rng_start, *rng_end; /* [n_ranges] per update: sorted, non-overlapping, start < end */
} acc_rcmd_updates;

typedef struct acc_rcmd_table {
    uint32_t    n_cmd, end_inclusive;
    uint64_t    n_ranges;              /* rng_off[n_cmd] */
    uint32_t    n_dict, reserved;
    acc_ts_cols txn_id;                /* [n_cmd] TxnId order */
    const uint8_t  *flags;             /* [n_cmd] ACC_RCMD_ERASED (and ACC_RCMD_HAS_DEPS once acc_rcmd_update_cmds set it) */
    const uint32_t *rng_off;           /* [n_cmd+1] */
    const uint64_t *rng_start, *rng_end; /* [n_ranges] */
    const uint64_t *dict_start, *dict_end; /* [n_dict] distinct ranges of the non-erased commands, Range::compare order */
} acc_rcmd_table;

int  acc_rcmd_create(acc_ctx *ctx, uint32_t end_inclusive, acc_rcmd **out);
void acc_rcmd_destroy(acc_rcmd *store);
int  acc_rcmd_update(acc_ctx *ctx, acc_rcmd *store, const acc_rcmd_updates *updates);
int  acc_rcmd_view(acc_ctx *ctx, acc_rcmd *store, acc_rcmd_table *out);
int  acc_rcmd_rangedeps(acc_ctx *ctx, acc_rcmd *store, const acc_cfk_mixed_queries *q, acc_rangedeps_view *out_view);

/* The state of each stored range command, and the recovery scans read from it.
 * The reference's RangeCommand points at the live Command (RangeCommand.command, impl/InMemoryCommandStore.java:524-539),
 * whose status, executeAt and PartialDeps mapReduceRangesInternal's recovery predicates read (:889-933). The store keeps
 * them per command beside its Ranges: status (Status ordinal 0..10 as in acc_range_cmds_in), execute_at (raw bits), the
 * ACC_RCMD_HAS_DEPS bit in the flags column and the PartialDeps flattened as acc_range_cmds_in describes them: (TxnId,
 * key | range) pairs sorted by TxnId.
 *
 * acc_rcmd_update_cmds is acc_rcmd_update with these columns: the ranges fold exactly as there (same grouping by
 * Timestamp.equals, array-order replay of Ranges.with, erasure rule and skipping of key-domain TxnIds; one
 * implementation serves both), and per command (group of updates of one TxnId, in array order)
 *   status, execute_at  those of the group's last update (execute_at.msb == NULL: the TxnIds, executeAtOrTxnId);
 *   deps, HAS_DEPS      those of the group's last update without ACC_RCMD_KEEP_DEPS; if every update of the group
 *                       carries it the stored deps and bit stay (a newly inserted command: none). An update's deps are
 *                       [dep_off[u], dep_off[u+1]); those of a KEEP_DEPS or erasing update are validated and ignored;
 *   ACC_RCMD_ERASED     the update stores its own status and executeAt, drops the deps and clears HAS_DEPS; every
 *                       later update of an erased command changes nothing (rcmd.erased_ignored), its state included.
 * A row that plain acc_rcmd_update inserts has status 0 (NotDefined), executeAt = its raw TxnId, no deps and HAS_DEPS
 * clear; on an existing row acc_rcmd_update leaves the state as it is, except that erasing drops the deps and clears
 * HAS_DEPS (an erased row holds neither ranges nor deps). Flags allowed here: ACC_RCMD_ERASED, ACC_RCMD_HAS_DEPS,
 * ACC_RCMD_KEEP_DEPS; ACC_RCMD_HISTORICAL or any other bit: ACC_E_ARG. historicalRangeCommands stay unmodelled, as in
 * acc_rcmd_rangedeps. Errors beside acc_rcmd_update's (all ACC_E_ARG, checked before anything indexes through an
 * offset): status > 10; dep_off not starting at 0 / decreasing / not ending at n_deps; an update's dep TxnIds decreasing
 * by Timestamp.compareTo; a range entry with start >= end; dep_is_key > 1. 2^32 - 1 or more stored deps: ACC_E_CAP. A
 * rejected batch leaves the store unchanged. Every update rewrites the state columns with the table (rows shift when
 * TxnIds are inserted below them and their deps move with them).
 *
 * acc_rcmd_state_view: DEVICE pointers to the state columns in acc_rcmd_view table order, valid until the next update
 * of the store. flags is the table's flags column: ACC_RCMD_ERASED | ACC_RCMD_HAS_DEPS.
 *
 * acc_rcmd_map_reduce_full answers acc_map_reduce_full_ranges' questions from the resident store (no historical rows)
 * for the query struct of acc_cfk_map_reduce_full, so one query batch serves both halves (end_inclusive must equal the
 * store's: ACC_E_ARG). Per query X = test_txn[q] a stored command C is visited iff it is not erased; its TxnId is in the
 * TestStartedAt window (< X for STARTED_BEFORE, > X strictly for STARTED_AFTER, any for ANY: no self-exclusion, under
 * ANY a command Timestamp.equals to X is visited, :895-906); for STARTED_BEFORE and ANY with test_dep != ANY_DEPS its
 * executeAt >= X (:901-905; STARTED_AFTER does not test it); the status test holds (IS_PROPOSED: Accepted,
 * PreCommitted, Committed; IS_STABLE: Stable <= s < Truncated); its kind is in the Kinds mask (test_kinds == -1:
 * X.kind().witnessedBy()); for WITH / WITHOUT HAS_DEPS is set and Deps.intersects(X, C.ranges) == (test_dep == WITH);
 * with ACC_FULL_EXECUTES_AFTER executeAt > X. Each range of a visited C that contains one of X's keys or intersects one
 * of X's ranges is collected per Range. The stabbing index lists the (stored range, command) candidates of each
 * participant inside the TxnId window and the Kinds mask; only those are tested (stats rcr.queries, rcr.raw_entries,
 * rcr.kept_entries, rcr.dep_probes, rcr.wave_launches). Result: an acc_rangedeps_view in the layout of
 * acc_rcmd_rangedeps (range_id into the store's dictionary, dep_txn = table indices, ascending), the context's last
 * RangeDeps result. The boolean predicates are u_off[q+1] > u_off[q]. The store is not modified. Errors: the participant
 * validation of acc_rcmd_rangedeps (ACC_E_ARG); started_at, test_dep or test_status > 2, unknown flags bits, test_kinds
 * > 0x3F: ACC_E_ARG; with test_kinds == -1 a LocalOnly X: ACC_E_STATE, an invalid kind ordinal: ACC_E_ARG. An empty
 * store, n_query == 0 and queries without participants give empty results; a failed call leaves the context usable. */
#define ACC_RCMD_KEEP_DEPS  8u

typedef struct acc_rcmd_cmd_updates {
    uint32_t    n_upd, mem;            /* as acc_rcmd_updates */
    uint64_t    n_ranges;
    acc_ts_cols txn_id;
    const uint8_t  *flags;             /* [n_upd] ACC_RCMD_ERASED | ACC_RCMD_HAS_DEPS | ACC_RCMD_KEEP_DEPS */
    const uint32_t *rng_off;
    const uint64_t *rng_start, *rng_end;
    acc_ts_cols execute_at;            /* [n_upd]; msb == NULL: the TxnIds */
    const uint8_t  *status;            /* [n_upd] Status ordinals 0..10 */
    uint64_t    n_deps;                /* dep_off[n_upd] */
    const uint32_t *dep_off;           /* [n_upd+1] */
    acc_ts_cols     dep_txn;           /* [n_deps] sorted by TxnId per update */
    const uint64_t *dep_start, *dep_end;
    const uint8_t  *dep_is_key;
} acc_rcmd_cmd_updates;

typedef struct acc_rcmd_state {
    uint32_t    n_cmd, reserved;
    uint64_t    n_deps;                /* dep_off[n_cmd] */
    acc_ts_cols execute_at;            /* [n_cmd] table order */
    const uint8_t  *status;            /* [n_cmd] */
    const uint8_t  *flags;             /* [n_cmd] ACC_RCMD_ERASED | ACC_RCMD_HAS_DEPS */
    const uint32_t *dep_off;           /* [n_cmd+1] */
    acc_ts_cols     dep_txn;           /* [n_deps] */
    const uint64_t *dep_start, *dep_end;
    const uint8_t  *dep_is_key;
} acc_rcmd_state;

int  acc_rcmd_update_cmds(acc_ctx *ctx, acc_rcmd *store, const acc_rcmd_cmd_updates *updates);
int  acc_rcmd_state_view(acc_ctx *ctx, acc_rcmd *store, acc_rcmd_state *out);
int  acc_rcmd_map_reduce_full(acc_ctx *ctx, acc_rcmd *store, const acc_cfk_recovery_in *q, acc_rangedeps_view *out_view);

/* RedundantBefore on the resident range-command store: the prune that keeps the range half a steady-state store, as
 * acc_cfk_redundant_before keeps the key half. CommandStore.markShardDurable (local/CommandStore.java:520-528) merges a
 * sync point into RedundantBefore; InMemoryCommandStore.markShardDurable (impl/InMemoryCommandStore.java:346-370) then
 * cuts `ranges` out of every range command below syncId and removes those left empty; from then on
 * InMemorySafeStore.update (:757-760) registers only what RedundantBefore.removeShardRedundant
 * (local/RedundantBefore.java:214-223, 431-435) leaves of a range command's ranges.
 * Input and map structs are acc_cfk_redundant_before's. in->end_inclusive must equal the store's; range j is (s, e] or
 * [s, e) by that bound type and holds bound[j], the shardAppliedOrInvalidatedBefore TxnId. Bounds are per range so one
 * call can carry several sync points: one call is the reference's markShardDurable calls, one per distinct bound, in
 * any order (AbstractRanges.subtract cuts each range of the left side into its maximal pieces outside the right side
 * and never merges across them, so subtracting disjoint ranges one after the other, in any order, is subtracting their
 * union). In call order:
 *   1. validation; ACC_E_ARG, store and map unchanged: mem not host / device, end_inclusive > 1 or not the store's,
 *      ranges unsorted, overlapping (rng_end[j-1] > rng_start[j]) or with start >= end, null arguments. n_ranges == 0
 *      is a no-op.
 *   2. the store's map RB, key code -> TxnId (all TxnId.NONE at first), becomes the pointwise Timestamp.compareTo
 *      maximum of RB and the input (RedundantBefore.merge: a lower bound is absorbed, never an error). An empty store
 *      records the map.
 *   3. the prune, defined by the call's input (as in the reference), not by the merged map: for every non-erased
 *      command C, J(C) = { j : C.txnId < bound[j] } strictly by compareTo (a TxnId that compares equal to a bound
 *      stays; identity bits outside compareTo do not matter); C.ranges = C.ranges.subtract(the ranges of J(C)): each
 *      stored range cut into its maximal pieces outside them, in order, none empty, nothing merged. A non-erased
 *      command with non-empty J(C) whose ranges are now empty leaves the table, one that already held no ranges
 *      included (removeIf tests every command below syncId). Rows above a dropped row shift down with their raw TxnId
 *      bits, status, executeAt, HAS_DEPS and deps spans unchanged (a range command's own deps are not trimmed here).
 *      Erased rows are not touched: they hold no ranges and stay as the tombstones that make later updates of that
 *      TxnId no-ops.
 *   4. if any row was cut or dropped the index is rebuilt from the new table exactly as an update rebuilds it, the new
 *      arrays are adopted, and earlier views of the store (acc_rcmd_view, acc_rcmd_state_view, results) are invalid.
 *      If nothing was cut or dropped no array is rewritten and every view stays valid.
 * Registration under a non-empty map (acc_rcmd_update, acc_rcmd_update_cmds; only once some bound is above NONE): per
 * non-erasing update of a range-domain TxnId t, the ranges that enter the Ranges.with fold are
 * add.subtract(the map's intervals whose bound > t). Validation runs on the caller's ranges, before trimming. A command
 * whose every update trims to nothing is still inserted, with no ranges (computeIfAbsent runs regardless), and stays
 * until a later prune whose bound is above it. Erasing updates, key-domain TxnIds and the state columns behave as
 * without a map. The store's owned ranges (ranges().allBetween) stay unmodelled: the store takes what it is given.
 * The queries (acc_rcmd_rangedeps, acc_rcmd_map_reduce_full) do not consult the map: they read the pruned state, as
 * mapReduceRangesInternal does.
 * acc_rcmd_redundant_view describes the map as acc_cfk_redundant_view does (closed intervals over the key codes,
 * ascending and disjoint, adjacent equal bounds merged; DEVICE pointers valid until the next
 * acc_rcmd_redundant_before on the store); n == 0 on a store that was never marked.
 * Stats: rcmd.redundant_cmds_cut (commands whose ranges changed but that stayed), rcmd.redundant_cmds_dropped,
 * rcmd.redundant_ranges_before / rcmd.redundant_ranges_after (table ranges), rcmd.update_ranges_trimmed (input ranges
 * the registration pre-pass changed or removed; set by the update calls), rcmd.redundant_prune_us /
 * rcmd.redundant_index_us (stream time of the prune passes and of the index rebuild).
 * RedundantBefore.collectDeps, the (range, bound) deps PreAccept adds to its result (RedundantBefore.java:181-190,
 * 418-421), is acc_rcmd_partial_rangedeps below.
 * Out of scope: an Entry's locally-redundant, bootstrap and stale fields;
 * historicalRangeCommands and maxRedundant (InMemoryCommandStore.java:350-354, 366); removing the tombstones of erased
 * commands; the state of a dropped command: it is gone, a later acc_rcmd_update_cmds of that TxnId carries its own
 * state and a plain acc_rcmd_update re-inserts it NotDefined, as for any absent TxnId. */
int  acc_rcmd_redundant_before(acc_ctx *ctx, acc_rcmd *store, const acc_cfk_redundant_in *in);
int  acc_rcmd_redundant_view(acc_ctx *ctx, acc_rcmd *store, acc_cfk_redundant_map *out);

/* PreAccept's RangeDeps from the pruned store: the stab result with RedundantBefore.collectDeps' range deps.
 * PreAccept.calculatePartialDeps (messages/PreAccept.java:245-265) returns builder.build().with(redundant), where
 * redundant = RedundantBefore.collectDeps (local/RedundantBefore.java:181-190, 418-421) holds one (entry.range,
 * shardAppliedOrInvalidatedBefore) range dep for every RedundantBefore entry a participant of the txn touches
 * (ReducingRangeMap.foldl, utils/ReducingRangeMap.java:120-196): the dep on the sync point stands for every dep the
 * prune removed. acc_rcmd_partial_rangedeps is acc_rcmd_rangedeps with that second side, so that with
 * acc_cfk_keydeps(_mixed) it is the whole PartialDeps of calculatePartialDeps from resident state (collectDeps adds no
 * key dep).
 * The map is the store's own (acc_rcmd_redundant_view): an Entry is modelled by its shardAppliedOrInvalidatedBefore
 * alone, and since Builder.tryMergeEqual and slice (RedundantBefore.java:470-496) keep entry.range equal to the map
 * segment and merge touching entries that are otherwise equal, a maximal interval m = [st, en] of the view is exactly
 * one entry.range: Range(m) = (st - 1, en] on an EndInclusive store, [st, en + 1) otherwise. Epoch bounds are
 * unmodelled (outOfBounds is never true).
 * Per query q, I(q) = the intervals m with bound[m] > TxnId.NONE that a participant of q touches: a key k when
 * st <= k <= en, a range when it intersects Range(m) as a set of keys (touching ends do not intersect); each interval
 * once per query. Nothing else filters: no STARTED_BEFORE test against executeAt (the reference carries a TODO there,
 * PreAccept.java:261), no witnesses() test, no exclusion of the query's own TxnId, and whatever the domain of the bound
 * TxnId the pair is a range dep (Deps.AbstractBuilder.add routes by the range's domain, primitives/Deps.java:56-71).
 * The result of q is Stab(q).with(Redundant(q)) (RangeDeps.with, primitives/RangeDeps.java:567-581, a linearUnion):
 * Stab(q) what acc_rcmd_rangedeps returns, Redundant(q) the RangeDeps of {(Range(m), bound[m]) : m in I(q)}; ranges by
 * Range::compare, TxnIds by compareTo, each range's list the union of both sides, a (range, TxnId) pair of both sides
 * (the sync point stored as a range command whose range equals the interval) once.
 * rd is the context's last RangeDeps result in the acc_rcmd_rangedeps layout over two union tables: its dictionary
 * (rd.rng_start / rng_end) is the store's dictionary merged with Range(m) of every interval with bound > NONE, equal
 * ranges once; dep_txn index ids, the table's TxnIds (erased rows included) merged with the distinct bounds > NONE,
 * Timestamp.equals ids once; id_row[i] is the acc_rcmd_view row of id i or 0xFFFFFFFF for a bound no row equals. Raw
 * bits of an id: the stored row's where a row equals it (linearUnion keeps the left instance, the builder's), else the
 * bound's as acc_rcmd_redundant_view reports them for the lowest interval holding it. (In a query whose stab result
 * lacks that command the reference would carry the bound's own instance; the two differ only in bits outside
 * Timestamp.equals, and that per-query difference is not modelled.)
 * acc_rangedeps_copy_out copies rd, dictionary included; ids and id_row are read with acc_copy_out. Everything is valid
 * until the next RangeDeps compute call on the context or the next update or prune of the store. The store is not
 * modified. Validation, errors and the rangedeps.* stats are acc_rcmd_rangedeps's, by the same code in the same order.
 * With no bound above NONE (a store never marked, or only NONE bounds) the call is acc_rcmd_rangedeps: a store never
 * marked launches its kernels and no others, rd is bit-identical, ids are the table's columns and id_row[i] = i. (A map
 * of NONE bounds only is found to be one by the index build of the first call after it changed.) An empty store with a
 * non-empty map still returns the redundant deps.
 * The union tables, the per-interval ids and the stabbing index's (range id, TxnId position) column renamed into them
 * are cached in the store: built by the first call after an acc_rcmd_update*, or an acc_rcmd_redundant_before with
 * ranges, and reused until the next one (updates and prunes themselves do no work for it).
 * Stats: rcmd.partial_intervals (the sum of |I(q)|), rcmd.partial_pairs_shared (pairs of both sides),
 * rcmd.union_builds (index builds over the store's life), rcmd.union_ids, rcmd.union_ranges.
 * Out of scope: PartialDeps.covering; a variant reading the CommandsForKey store's map (ReplicaStore keeps the two
 * maps equal). */
typedef struct acc_rcmd_partial_view {
    acc_rangedeps_view rd;   /* n_txn = n_query; rd.rng_start / rng_end [rd.n_ranges]: the union dictionary; range_id
                                index it, dep_txn index ids, arena holds positions in the query's own dep_txn list */
    uint32_t    n_ids, n_cmd;
    acc_ts_cols ids;         /* [n_ids] DEVICE */
    const uint32_t *id_row;  /* [n_ids] DEVICE */
} acc_rcmd_partial_view;
int  acc_rcmd_partial_rangedeps(acc_ctx *ctx, acc_rcmd *store, const acc_cfk_mixed_queries *q, acc_rcmd_partial_view *out);

/* ---- MaxConflicts and the PreAccept executeAt proposal (local/MaxConflicts.java:31-96,
 * local/CommandStore.java:280-290 updateMaxConflicts, :320-345 preaccept) ----
 * A CommandStore's MaxConflicts is the pointwise max of every (keysOrRanges, executeAt) update it received
 * (MaxConflicts.merge(map, create(keysOrRanges, executeAt)), a ReducingRangeMap folded with Timestamp::max; a key k
 * enters as its asRange(), which holds exactly k), so MaxConflicts.get(q) is the max executeAt over the updates whose
 * keys / ranges intersect q's keys / ranges (Range.contains for a key, compareIntersecting for two ranges).
 * Input: the updates (Command.executeAt() and keys or ranges each; updateMaxConflicts skips an update whose executeAt
 * does not exceed the previous one, which the max already absorbs). Output per query (a PreAccept of txn_id over its
 * sliced keys or ranges): max = minNonConflicting = MaxConflicts.get(keys) (all zero = Timestamp.NONE when nothing
 * intersects) and fast_path = txnId.compareTo(minNonConflicting) >= 0 (preaccept then returns txnId when
 * permitFastPath and the epoch check hold, the caller's part; otherwise time.uniqueNow(minNonConflicting)). Among
 * compare-equal timestamps with different raw flag bits, which instance is returned is unspecified. */
typedef struct acc_conflicts_in {
    uint32_t mem, n_upd, end_inclusive;
    uint64_t n_keys, n_ranges;
    acc_ts_cols execute_at;      /* [n_upd] */
    const uint32_t *key_off;     /* [n_upd+1] */
    const uint64_t *key;         /* [n_keys] sorted unique per update */
    const uint32_t *rng_off;     /* [n_upd+1] */
    const uint64_t *rng_start, *rng_end;   /* [n_ranges] sorted, non-overlapping per update */
} acc_conflicts_in;

typedef struct acc_preaccept_in {
    uint32_t mem, n_query;
    uint64_t n_parts;
    acc_ts_cols txn_id;          /* [n_query] */
    const uint8_t *is_range;     /* [n_query] 0: keys, 1: ranges */
    const uint32_t *part_off;    /* [n_query+1] */
    const uint64_t *part_start, *part_end;
} acc_preaccept_in;

typedef struct acc_preaccept_out {
    uint32_t mem;
    uint64_t *max_msb, *max_lsb;
    int32_t  *max_node;
    uint8_t  *fast_path;         /* all [n_query], caller-owned */
} acc_preaccept_out;

int  acc_max_conflicts(acc_ctx *ctx, const acc_conflicts_in *updates, const acc_preaccept_in *queries,
                       acc_preaccept_out *out);

/* A CommandStore's MaxConflicts kept on the device across calls (the store's one map, CommandStore.maxConflicts,
 * local/CommandStore.java:270-290): disjoint intervals over the key codes with a Timestamp each (ReducingRangeMap).
 * acc_maxconflicts_update merges a batch of commands' (keysOrRanges, executeAt) into it (MaxConflicts.update =
 * ReducingIntervalMap.merge with Timestamp::max; a batch equals its commands applied one by one in any order);
 * acc_maxconflicts_get answers PreAccept queries as acc_max_conflicts does, in O(log map) per key or range (the
 * acc_max_conflicts form rebuilds the map from the store's whole update history on every call). end_inclusive fixes
 * the map's Range bound type; updates must carry the same. Not thread-safe; one context at a time. */
typedef struct acc_maxconflicts acc_maxconflicts;
int  acc_maxconflicts_create(acc_ctx *ctx, uint32_t end_inclusive, acc_maxconflicts **out);
void acc_maxconflicts_destroy(acc_maxconflicts *map);
int  acc_maxconflicts_update(acc_ctx *ctx, acc_maxconflicts *map, const acc_conflicts_in *updates);
int  acc_maxconflicts_get(acc_ctx *ctx, acc_maxconflicts *map, const acc_preaccept_in *queries, acc_preaccept_out *out);
/* intervals currently held (ReducingRangeMap.size) */
uint64_t acc_maxconflicts_size(const acc_maxconflicts *map);

/* ---- Execution readiness from a resident WaitingOn store ----
 * acc_waiting is Command.WaitingOn (local/Command.java:1294-1610) of every registered Stable command, kept in DEVICE
 * memory and advanced as local/Commands.java advances it: initialiseWaitingOn (:735-753), updateWaitingOn (:755-830),
 * updateDependencyAndMaybeExecute (:832-857) and removeWaitingOnKeyAndMaybeExecute (:859-876), read against the state
 * an acc_rcmd store holds per command (acc_rcmd_state: status, executeAt). One call per batch returns the commands
 * whose maybeExecute (:656-733) would now pass: it takes the rel pairs acc_cfk_notify / acc_cfk_notify_unmanaged report
 * and the `until` values the unmanaged calls hand the caller for WaitingOn.executeAtLeast.
 *
 * The store: one record per registered command W in TxnId order (Timestamp.compareTo): txn_id and execute_at (raw
 * bits); flags: ACC_WT_AWAITS_ONLY_DEPS when W's kind is ExclusiveSyncPoint or EphemeralRead (primitives/Txn.java:211-214),
 * ACC_WT_RANGE_DOMAIN when the record has an appliedOrInvalidated set (Command.java:1435); execute_at_least (all-zero:
 * null); key[] = keyDeps.keys() codes, sorted unique, with key_wait[] (u8, 0 / 1); dep[] = rangeDeps.txnIds(), sorted
 * unique, with dep_state[] (u8): ACC_WT_NOT_WAITING, ACC_WT_WAITING, or ACC_WT_APPLIED_OR_INVALIDATED (not waiting and
 * the bit is set in appliedOrInvalidated). The Java pair (waiting, appliedOrInvalidated) never holds (1, 1), so the
 * three states are exact; in the Java bitsets txn i is bit i and key k is bit n_dep + k. Beside the records the store
 * keeps an index from a dep TxnId to the slots that hold it (the dep slots in TxnId order), rebuilt whenever the record
 * table is rebuilt (register, erase): acc_waiting_notify evaluates only the slots of the changed deps. (The state
 * columns are copied once per notify, so that a failed call changes nothing, and the ready list is one pass over the
 * records; neither reads a slot's dep.)
 *
 * evaluate(W, i) for a slot whose state is WAITING; D = W.dep[i], found in the acc_rcmd table by Timestamp.equals;
 * status ordinals as in acc_range_cmds_in (NotDefined 0 .. PreCommitted 4 .. Applied 8, Truncated 9, Invalidated 10):
 *   0. D is absent or its status is below 4: nothing (ifLoadedAndInitialised null or not hasBeen(PreCommitted), :763-765);
 *   1. known = 4 <= status <= 9 and D.executeAt is not all-zero (the convention for Erased: an erased row whose
 *      executeAt is unknown carries zeros). If W awaits only deps, known, and D.executeAt > W.txnId:
 *      execute_at_least = max(D.executeAt, execute_at_least), the new value on a tie (:782-783);
 *   2. status >= 9: setAppliedOrInvalidated(i): the state becomes 2 for a range-domain W, 0 otherwise
 *      (Command.java:1552-1566);
 *   3. else if D.executeAt > W.executeAt and W does not await only deps: removeWaitingOn, the state becomes 0 (:804-810);
 *   4. else if status == 8: setAppliedAndPropagate (Command.java:1568-1584): slot i is set as in step 2; if D has a
 *      record R in this store and R is range-domain, every dep E common to R.dep and W.dep with R.dep_state[E] == 2 is
 *      set in W as in step 2 if it is WAITING there. R is read as it stood when the call began. An Applied D whose
 *      record still waits (on a key or a dep) is the reference's broken invariant: ACC_E_STATE, nothing changes;
 *   5. else W keeps waiting.
 * A record's slots are evaluated in descending slot order and a slot cleared earlier in the walk is not visited
 * (utils/SimpleBitSet.java:373-387). The order matters: with deps E < D, D Applied, R_D.dep_state[E] == 2 and E executing
 * after W, the descending walk leaves E at 2 where an ascending one would leave 0.
 * Deliberate divergence: the reference's ranged reverseForEach(from, to) indexes every word with fromIndex
 * (SimpleBitSet.java:404-407), so with 64 or more txnIds it re-visits slots 0..63 and never visits the rest. These calls
 * visit every waiting slot below n_dep once, descending: what the method's single-word path does.
 *
 * acc_waiting_register is initialiseWaitingOn for a batch: per waiter TxnId and executeAt, its keys with key_wait and
 * its deps with dep_wait, the initial bits (NULL: all ones). The caller decides them: rangeDeps.forEach(
 * executionParticipants) and the keys inside the store's ranges (:746-751) are topology decisions, and
 * acc_rangedeps_stab answers the first. Each new record runs evaluate over its waiting slots; the new records enter the
 * table by a stable merge. out, per waiter: waiting = the slots (deps and keys) it still waits on (0: ready at once) and
 * execute_at_least. ACC_E_ARG, store unchanged: a bad mem; offsets not starting at 0, decreasing or not ending at the
 * counts; keys or deps not sorted unique; a key-domain dep TxnId; a kind ordinal above 5; a wait byte above 1; the same
 * waiter twice in one call or a waiter already registered; an unknown tier. ACC_E_STATE: a waiter that rcmd holds at
 * status >= 8 (so every new record reads finished records only and the batch is order-free); the step-4 invariant.
 * ACC_E_CAP at 2^32 - 1 records or slots. n_waiters == 0 is a no-op.
 *
 * acc_waiting_notify: changed = dep TxnIds, sorted unique (changed.msb == NULL: every waiting slot is re-evaluated);
 * per record the waiting slots whose dep is in changed run evaluate, descending (updateDependencyAndMaybeExecute for
 * each). Then the release pairs (rel_txn, rel_key, rel_flags, rel_until), in any order, duplicates allowed: bit 0 of
 * rel_flags (ACC_WT_REL_KEY) clears the record's key_wait for that key (removeWaitingOnKeyAndMaybeExecute); a pair with
 * no record, or with bit 0 set and a key not in the record or a bit already clear, is ignored and counted; a non-zero
 * rel_until on an awaits-only-deps record raises execute_at_least when it is strictly above it (the guarded
 * updateExecuteAtLeast of local/CommandsForKey.java:1372-1381, 1476-1484; the existing value stays on a tie). out: the records that were
 * waiting before the call and are not after it, in TxnId order: ready_rec (record index before any erase), ready_txn,
 * ready_execute_at_least; n_changed = the slots (deps and keys) that stopped waiting. Errors as for register where they
 * apply (mem, tier, changed not sorted unique, a rel_flags byte above 1: ACC_E_ARG; step 4: ACC_E_STATE); a failed
 * call leaves the store unchanged.
 *
 * acc_waiting_erase: TxnIds sorted unique; their records leave by a stable compaction and the index is rebuilt. Absent
 * ids are counted and ignored; a record that still waits may be erased (truncation).
 * acc_waiting_view: the columns above and per record n_wait_dep, n_wait_key and next_waiting_on = the highest WAITING
 * dep slot or ACC_WT_NONE (WaitingOn.nextWaitingOn, :1359-1363).
 * Inputs take mem HOST or DEVICE; outputs are DEVICE pointers, valid until the context's next compute call; the view
 * until the store's next change. Records with at most WT_LANE_MAX (16) dep slots are walked by one lane, longer ones by
 * one wave; a non-zero tier forces one. Results do not depend on it.
 * Stats: wt.records, wt.slots (dep and key slots), wt.register_evaluated and wt.notify_slots (the slots that were
 * WAITING when the call began among those it was asked to evaluate: every slot of a new record; the slots whose dep is
 * in changed), wt.propagated, wt.ready, wt.key_released, wt.key_ignored, wt.erased, wt.register_us, wt.notify_us,
 * wt.erase_us.
 * Out of scope: removeRedundantDependencies / hasLocallyRedundantDependencies (:758-760); isFullyPreBootstrapOrStale;
 * the TruncatedApply checkState (:793); listeners and the progress log. */
#define ACC_WT_NOT_WAITING            0
#define ACC_WT_WAITING                1
#define ACC_WT_APPLIED_OR_INVALIDATED 2
#define ACC_WT_AWAITS_ONLY_DEPS       1u
#define ACC_WT_RANGE_DOMAIN           2u
#define ACC_WT_REL_KEY                1u
#define ACC_WT_NONE                   0xFFFFFFFFu
#define ACC_WT_TIER_LANE              1
#define ACC_WT_TIER_WAVE              2
typedef struct acc_waiting acc_waiting;
typedef struct acc_waiting_register_in {
    uint32_t mem, n_waiters;     /* ACC_MEM_HOST or ACC_MEM_DEVICE for every pointer */
    uint64_t n_keys, n_deps;
    acc_ts_cols txn_id, execute_at;   /* [n_waiters] */
    const uint32_t *key_off;     /* [n_waiters+1] */
    const uint64_t *key;         /* [n_keys] sorted unique per waiter */
    const uint8_t  *key_wait;    /* [n_keys] 0 / 1; NULL: all ones */
    const uint32_t *dep_off;     /* [n_waiters+1] */
    acc_ts_cols dep;             /* [n_deps] range-domain TxnIds, sorted unique per waiter */
    const uint8_t  *dep_wait;    /* [n_deps] 0 / 1; NULL: all ones */
    uint32_t tier;               /* 0: library default; ACC_WT_TIER_LANE / _WAVE force one kernel tier (tests) */
} acc_waiting_register_in;
typedef struct acc_waiting_register_out {
    uint32_t n_waiters, reserved;
    const uint32_t *waiting;     /* [n_waiters] slots still waited on; 0: ready */
    acc_ts_cols execute_at_least;
} acc_waiting_register_out;
typedef struct acc_waiting_notify_in {
    uint32_t mem, n_changed;
    acc_ts_cols changed;         /* [n_changed] sorted unique; msb == NULL: every waiting slot */
    uint32_t n_rel, tier;
    acc_ts_cols rel_txn;         /* [n_rel] */
    const uint64_t *rel_key;
    const uint8_t  *rel_flags;   /* bit 0: ACC_WT_REL_KEY */
    acc_ts_cols rel_until;       /* zeros: none */
} acc_waiting_notify_in;
typedef struct acc_waiting_notify_out {
    uint32_t n_ready, reserved;
    uint64_t n_changed;
    const uint32_t *ready_rec;   /* [n_ready] */
    acc_ts_cols ready_txn, ready_execute_at_least;
} acc_waiting_notify_out;
typedef struct acc_waiting_erase_in {
    uint32_t mem, n_ids;
    acc_ts_cols txn_id;          /* [n_ids] sorted unique */
} acc_waiting_erase_in;
typedef struct acc_waiting_table {   /* DEVICE pointers */
    uint32_t n_rec, reserved;
    uint64_t n_keys, n_deps;
    acc_ts_cols txn_id, execute_at, execute_at_least;   /* [n_rec] */
    const uint8_t  *flags;       /* [n_rec] ACC_WT_AWAITS_ONLY_DEPS | ACC_WT_RANGE_DOMAIN */
    const uint32_t *key_off;     /* [n_rec+1] */
    const uint64_t *key;         /* [n_keys] */
    const uint8_t  *key_wait;    /* [n_keys] */
    const uint32_t *dep_off;     /* [n_rec+1] */
    acc_ts_cols dep;             /* [n_deps] */
    const uint8_t  *dep_state;   /* [n_deps] ACC_WT_NOT_WAITING / _WAITING / _APPLIED_OR_INVALIDATED */
    const uint32_t *n_wait_dep, *n_wait_key, *next_waiting_on;   /* [n_rec] */
} acc_waiting_table;
int  acc_waiting_create(acc_ctx *ctx, acc_waiting **out);
void acc_waiting_destroy(acc_waiting *w);
int  acc_waiting_register(acc_ctx *ctx, acc_waiting *w, acc_rcmd *rcmd, const acc_waiting_register_in *in,
                          acc_waiting_register_out *out);
int  acc_waiting_notify(acc_ctx *ctx, acc_waiting *w, acc_rcmd *rcmd, const acc_waiting_notify_in *in,
                        acc_waiting_notify_out *out);
int  acc_waiting_erase(acc_ctx *ctx, acc_waiting *w, const acc_waiting_erase_in *in);
int  acc_waiting_view(acc_ctx *ctx, acc_waiting *w, acc_waiting_table *out);

/* ---- Levelisation of a dependency graph by executeAt ----
 * Graph over n txns: deps of txn t = dep[off[t] .. off[t+1]) (batch indices); exec_rank[t] = order
 * rank of t.executeAt. Edges whose dep has exec_rank >= exec_rank[t] are ignored (Commands.java:804-810).
 * level[t] = 0 without remaining preds, else 1 + max level(pred); order = txns sorted by
 * (level, exec_rank, index). Outputs are caller buffers of n elements in `mem`. */
typedef struct acc_graph_in {
    uint32_t mem;
    uint32_t n;
    const uint64_t *off;       /* [n+1] */
    const uint32_t *dep;       /* [off[n]] */
    const uint32_t *exec_rank; /* [n] */
} acc_graph_in;

int acc_levelise(acc_ctx *ctx, const acc_graph_in *in, uint32_t *level, uint32_t *order, uint32_t *n_levels);

/* ---- Ranges algebra (host code, no context; primitives/Ranges.java, AbstractRanges.java) ----
 * A Ranges is a sorted, deoverlapped list of Range (start, end) key codes of one bound type (Range.EndInclusive (s, e]
 * or Range.StartInclusive [s, e), Range.java:40-138); operations on ranges alone do not depend on the bound type.
 * Results go to caller arrays of `cap` entries; *out_n is always the result size (ACC_E_CAP when > cap; bounds:
 * with / subtract <= a.n + b.n, merge_touching <= a.n, select <= k, of <= in.n). Inputs that must be sorted and
 * deoverlapped are checked (Ranges.ofSortedAndDeoverlapped: IllegalArgumentException -> ACC_E_ARG). */
/* (acc_rlist is declared at the top of this header) */

/* Ranges.of(Range...)                          AbstractRanges.java:689-707 (sort by Range::compare, merge overlaps) */
int acc_ranges_of(const acc_rlist *in, uint64_t *out_start, uint64_t *out_end, uint32_t cap, uint32_t *out_n);
/* a.with(b) = union(MERGE_OVERLAPPING)         Ranges.java:119-127, AbstractRanges.java:439-585 */
int acc_ranges_with(const acc_rlist *a, const acc_rlist *b, uint64_t *out_start, uint64_t *out_end, uint32_t cap,
                    uint32_t *out_n);
/* a.subtract(b)                                AbstractRanges.java:223-287 */
int acc_ranges_subtract(const acc_rlist *a, const acc_rlist *b, uint64_t *out_start, uint64_t *out_end, uint32_t cap,
                        uint32_t *out_n);
/* a.mergeTouching()                            AbstractRanges.java:637-675 */
int acc_ranges_merge_touching(const acc_rlist *a, uint64_t *out_start, uint64_t *out_end, uint32_t cap, uint32_t *out_n);
/* a.select(int[] indexes)                      Ranges.java:76-82 */
int acc_ranges_select(const acc_rlist *a, const uint32_t *idx, uint32_t k, uint64_t *out_start, uint64_t *out_end,
                      uint32_t cap, uint32_t *out_n);
/* a.indexOf(key): index, or -(insertion point) - 1   AbstractRanges.java:51-54 (SortedArrays FAST search) */
int acc_ranges_index_of(const acc_rlist *a, uint32_t end_inclusive, uint64_t key, int64_t *out_index);
/* a.containsAll(Keys) (sorted unique key codes) AbstractRanges.java:86-91; a.containsAll(Ranges) :96-101 */
int acc_ranges_contains_all_keys(const acc_rlist *a, uint32_t end_inclusive, const uint64_t *keys, uint32_t n_keys,
                                 int32_t *out);
int acc_ranges_contains_all(const acc_rlist *a, const acc_rlist *b, int32_t *out);
/* RangeDeps.isCoveredBy(covering) over a RangeDeps' ranges (sorted by Range::compare) primitives/RangeDeps.java:595-613 */
int acc_rangedeps_is_covered_by(const acc_rlist *range_deps_ranges, const acc_rlist *covering, int32_t *out);

/* ---- timing (ACC_OPT_TIMING) ---- */
/* Per-kernel accumulated device time since the last reset: name[i], total ms, launch count. */
int  acc_timing_count(acc_ctx *ctx);
int  acc_timing_get(acc_ctx *ctx, int i, const char **name, double *total_ms, uint64_t *launches);
void acc_timing_reset(acc_ctx *ctx);
/* Restrict the per-kernel events to the launches whose tag is in the comma-separated list (NULL or "" = every launch).
   Each timed launch adds two event records to the stream; a bench times its step with only the kernel it reports. */
int  acc_timing_filter(acc_ctx *ctx, const char *tags_csv);

/* ---- counters of the last call (e.g. "keydeps.path_replay", "keydeps.big_txns", "keydeps.big_entries") ---- */
int acc_stats_count(acc_ctx *ctx);
int acc_stats_get(acc_ctx *ctx, int i, const char **name, uint64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* ACCORD_AMD_H */
