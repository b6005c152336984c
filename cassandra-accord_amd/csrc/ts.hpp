// ts.hpp — the one definition of Timestamp order, of the Timestamp value type Ts that carries it, and of
// Kind.witnesses() on the device, shared by every path that compares TxnIds / executeAts or filters by kind (keydeps,
// rangedeps, cfk, cfkdeps, conflicts, recovery, rmm, the resident stores). search.hpp has the searches in this order.
// latest.hip's Ballot compare and wire.hip's Big::cmp are other orders and keep their own code.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace acc {

// Timestamp words in compare order (Timestamp.compareTo, primitives/Timestamp.java:208-217): w0 = msb (unsigned),
// w1 = lsb & IDENTITY_LSB (lowHlc then identity flags, unsigned compare is exact because lowHlc < 2^48),
// w2 = node ^ 0x80000000 (signed -> unsigned order). Equal words <=> Timestamp.equals (:244-249).
constexpr uint64_t IDENTITY_LSB = 0xFFFFFFFFFFFF001EULL;

__device__ __forceinline__ uint64_t ts_w1(uint64_t lsb) { return lsb & IDENTITY_LSB; }
__device__ __forceinline__ uint64_t ts_w2(int32_t node) { return (uint64_t)((uint32_t)node ^ 0x80000000u); }

// Timestamp.compareTo (primitives/Timestamp.java:208-217): msb, then lsb & IDENTITY_LSB, then the signed node
__device__ __forceinline__ int ts_cmp(uint64_t am, uint64_t al, int32_t an, uint64_t bm, uint64_t bl, int32_t bn)
{
    if (am != bm) return am < bm ? -1 : 1;
    uint64_t a1 = ts_w1(al), b1 = ts_w1(bl);
    if (a1 != b1) return a1 < b1 ? -1 : 1;
    if (an != bn) return an < bn ? -1 : 1;
    return 0;
}

// A Timestamp (TxnId, executeAt, bound) by value: msb, lsb, node. Stored as such in cfkdeps.hip's device buffers.
struct Ts {
    uint64_t m, l;
    int32_t n;
};
static_assert(sizeof(Ts) == 24 && offsetof(Ts, n) == 16, "Ts is stored in device buffers: 24 B, node at 16");
__device__ __forceinline__ int cmp(const Ts &a, const Ts &b) { return ts_cmp(a.m, a.l, a.n, b.m, b.l, b.n); }
__device__ __forceinline__ bool is_null(const Ts &a) { return a.m == 0 && a.l == 0 && a.n == 0; }   // Timestamp.NONE / absent
// element i of a column triple
__device__ __forceinline__ Ts ts_at(const uint64_t *m, const uint64_t *l, const int32_t *n, uint32_t i) { return Ts{ m[i], l[i], n[i] }; }

// Kind.witnesses() as a bitmask over Kind ordinals (primitives/Txn.java:221-236); 0 = throws.
__device__ __forceinline__ uint32_t witnesses(uint32_t kind)
{
    switch (kind) {
    case 0: case 2: return 1u << 1;                                   // Read, EphemeralRead -> Ws
    case 1: case 3: return (1u << 0) | (1u << 1);                     // Write, SyncPoint -> RsOrWs
    case 4:         return (1u << 0) | (1u << 1) | (1u << 3) | (1u << 4);  // ESP -> AnyGloballyVisible
    default:        return 0;
    }
}

// Kind.witnessedBy() (primitives/Txn.java:247-262) as a mask over Kind ordinals: EphemeralRead -> Nothing,
// Read -> WsOrSyncPoints, Write -> AnyGloballyVisible, SyncPoint / ExclusiveSyncPoint -> ExclusiveSyncPoints;
// -1 = throws (LocalOnly) or no such ordinal. The recovery scans' default Kinds (recovery.hip, cfkquery.hip).
__device__ __forceinline__ int witnessed_by(uint32_t kind)
{
    switch (kind) {
    case 2:         return 0;
    case 0:         return (1 << 1) | (1 << 3) | (1 << 4);
    case 1:         return (1 << 0) | (1 << 1) | (1 << 3) | (1 << 4);
    case 3: case 4: return 1 << 4;
    default:        return -1;
    }
}

// Kind class for the Kinds predicates (Txn.java:140-152): Read 0, Write 1, SyncPoint/ExclusiveSyncPoint 2;
// EphemeralRead and LocalOnly are witnessed by no predicate (3 = none).
__device__ __forceinline__ uint32_t kind_class(uint32_t kind)
{
    return kind == 0 ? 0u : kind == 1 ? 1u : (kind == 3 || kind == 4) ? 2u : 3u;
}

// "Bumped committed" as the run-based KeyDeps scan lists it, a per-txn property: committed (InternalStatus 4..6), of a
// kind some predicate witnesses, executeAt != TxnId (v2_code, keydeps.hip, decides the same per CFK position).
__device__ __forceinline__ bool bumped_committed(uint32_t status, uint32_t kind, bool bumped)
{
    return bumped && status >= 4 && status <= 6 && kind_class(kind) < 3;
}

}  // namespace acc
