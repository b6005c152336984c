// cfkunmanaged.hip — the Unmanaged pending records of the resident CommandsForKey store: commands that wait on keys
// without being CommandsForKey members (range-domain txns: range reads and sync points; key-domain EphemeralRead and
// LocalOnly). acc_cfk_register_unmanaged is CommandsForKey.registerUnmanaged (local/CommandsForKey.java:1406-1498) for
// every (waiter, key) pair of a batch; acc_cfk_notify_unmanaged is the tail of notifyAndUpdatePending (:1206-1212):
// notifyUnmanaged (:1270-1316) with updatePending (:1333-1388), in closed form over the pending table.
//
// register, all pairs at once against the store as it stands (an outcome does not depend on the TRANSITIVELY_KNOWN
// entries another pair of the call inserts: such a dep counts as not committed absent or present):
//   1. k_um_waiters / k_um_pairs / k_um_deporder: kinds and offsets validated per waiter, key order per pair, dep order
//      per dep (one sync point lists every key, and a hot key's pair every entry: no lane walks a whole list to check
//      it); each pair's waiter, store key, and the lower bound of RB(key) in its deps (deps below the bound take no
//      part; a dep equal to it stays);
//   2. the evaluation, a merge-join of the pair's trimmed deps with the key's segment, by one of two tiers:
//        LANE  trimmed deps <= UM_LANE_MAX: one lane per pair walks both lists (the reference's loop as it is);
//        WAVE  the rest: one wave per pair, a lane per dep searching the segment (galloping on from where the lane's
//              previous dep, 64 deps lower, was found), the two flags reduced by ballot and executesAt by a wave max
//              (ties to the lower dep, as the sequential max keeps the earlier);
//      a dep absent from the segment sets its flag in the dep space;
//   3. scans: the missing flags, the not-ready pairs, their kept dep counts; one read-back (errors, the three totals,
//      the outcome counts; the waiters' own errors and the count of distinct waiter TxnIds are read before step 1's
//      pair pass, which finds each pair's waiter through key_off);
//   4. the missing (key, TxnId) sorted by four stable radix passes (node, lsb, msb, key), run heads marked and
//      compacted, the heads of keys the store lacks compacted too; one read-back of the two counts;
//   5. old keys, new keys, old entries and additions each placed at their own index plus their rank in the other
//      list (a binary search); miss_off from a scan of the per-entry counts; the missing columns copied as they are.
// notify, a thread per record: the COMMIT threshold against minUncommitted, updatePending's walk, the APPLY threshold
// against next.executeAt; event and keep flags scanned; released records leave by rb_segcopy over the record columns
// and the dep CSR.
#include "cfkunmanaged.hpp"
#include "cfkredundant.hpp"
#include "prims.hpp"
#include "search.hpp"

namespace acc {
namespace um {

constexpr uint32_t UM_LANE_MAX = 16;   // trimmed deps of a pair the lane tier walks by default
constexpr uint32_t NONE = 0xFFFFFFFFu;

using mc::Map;

enum : uint64_t { E_OFF = 1, E_KEYS = 2, E_DEPOFF = 4, E_DEPS = 8, E_KIND = 16, E_MANAGED = 32, E_ILLEGAL = 64 };
enum : uint32_t { T_LANE = ACC_UNM_TIER_LANE, T_WAVE = ACC_UNM_TIER_WAVE };

__host__ __device__ __forceinline__ uint32_t tier_of(uint32_t n, uint32_t forced)
{
    return forced ? forced : n <= UM_LANE_MAX ? T_LANE : T_WAVE;
}

// Txn.Kind.awaitsOnlyDeps (primitives/Txn.java:211-214): ExclusiveSyncPoint or EphemeralRead
__device__ __forceinline__ bool awaits_only_deps(uint64_t lsb)
{
    const uint32_t k = (uint32_t)(lsb >> 1) & 7u;
    return k == ACC_KIND_EXCLUSIVE_SYNC_POINT || k == ACC_KIND_EPHEMERAL_READ;
}

__device__ __forceinline__ Ts dep_of(const In &d, uint32_t i) { return Ts{ d.dm[i], d.dl[i], d.dn[i] }; }
__device__ __forceinline__ Ts id_of(const CfkResident &s, uint32_t e) { return Ts{ s.em[e], s.el[e], s.en[e] }; }
__device__ __forceinline__ Ts x_of(const CfkResident &s, uint32_t e) { return Ts{ s.xm[e], s.xl[e], s.xn[e] }; }

// first entry of [from, hi) with TxnId >= t, from a lower bound `from` of the answer: doubling steps, then a bisection of
// the last step
__device__ __forceinline__ uint32_t gallop_entry(const CfkResident &s, uint32_t from, uint32_t hi, const Ts &t)
{
    if (from >= hi || cmp(id_of(s, from), t) >= 0) return from;
    uint32_t lo = from, w = 1;   // entry lo is below t
    while (lo + w < hi && cmp(id_of(s, lo + w), t) < 0) { lo += w; w <<= 1; }
    return lower_bound_ts(s.em, s.el, s.en, lo + 1, min(lo + w, hi), t);
}

// ---------------------------------------------------------------- register: validation

__global__ __launch_bounds__(BLOCK) void k_um_waiters(In d, uint64_t *__restrict__ errs, uint64_t *__restrict__ w0,
                                                      uint64_t *__restrict__ w1, uint64_t *__restrict__ w2)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= d.nw) return;
    uint64_t e = 0;
    const uint64_t l = d.tl[i];
    const uint32_t kind = (uint32_t)(l >> 1) & 7u;
    if (kind > ACC_KIND_LOCAL_ONLY) e |= E_KIND;
    else if (!(l & 1u) && kind != ACC_KIND_EPHEMERAL_READ && kind != ACC_KIND_LOCAL_ONLY) e |= E_MANAGED;   // SafeCommandStore.java:224
    const uint32_t k0 = d.key_off[i], k1 = d.key_off[i + 1];
    if (k1 < k0 || k1 > d.NP || (i == 0 && k0 != 0) || (i + 1 == d.nw && k1 != d.NP)) e |= E_OFF;
    w0[i] = d.tm[i];
    w1[i] = l & IDENTITY_LSB;
    w2[i] = (uint64_t)((uint32_t)d.tn[i] ^ 0x80000000u);
    if (e) atomicOr((unsigned long long *)errs, (unsigned long long)e);
}

struct Pairs {
    uint32_t *waiter, *kidx, *cut;   // per pair: its waiter, its store key (NONE: no CFK), the first dep >= RB(key)
};

// a pair with malformed offsets gets cut = NONE: nothing indexes through it, and the call fails
__global__ __launch_bounds__(BLOCK) void k_um_pairs(In d, Map mp, int has_rb, CfkResident s, Pairs p, uint64_t *__restrict__ errs)
{
    const uint64_t j64 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j64 >= d.NP) return;
    const uint32_t j = (uint32_t)j64;
    const uint32_t a = d.dep_off[j], b = d.dep_off[j + 1];
    const uint32_t w = seg_of(d.key_off, d.nw, j);
    p.waiter[j] = w;
    p.kidx[j] = NONE;
    // a waiter's keys sorted unique, checked pair by pair: one sync point may list every key of the store
    if (j > d.key_off[w] && d.key[j - 1] >= d.key[j]) atomicOr((unsigned long long *)errs, (unsigned long long)E_KEYS);
    if (b < a || b > d.ND || (j == 0 && a != 0) || (j64 + 1 == d.NP && b != d.ND)) {
        atomicOr((unsigned long long *)errs, (unsigned long long)E_DEPOFF);
        p.cut[j] = NONE;
        return;
    }
    const uint64_t c = d.key[j];
    p.kidx[j] = find_sorted(s.key, s.nk, c);
    const Ts bound = has_rb ? mc::point(mp, c) : Ts{ 0, 0, 0 };
    p.cut[j] = lower_bound_ts(d.dm, d.dl, d.dn, a, b, bound);   // txnIds.find(shardRedundantBefore): the index, or the insert point
}

// deps of a pair sorted unique, checked dep by dep (one sync point's pair may hold a hot key's every entry): a dep that
// is not above the one before it must be the first of its pair. An unsorted list is still walked within its bounds by
// the evaluation below; the call fails at the read-back.
__global__ __launch_bounds__(BLOCK) void k_um_deporder(In d, uint64_t *__restrict__ errs)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i64 == 0 || i64 >= d.ND) return;
    const uint32_t i = (uint32_t)i64;
    if (cmp(dep_of(d, i - 1), dep_of(d, i)) < 0) return;
    if (d.dep_off[seg_of(d.dep_off, (uint32_t)d.NP, i)] != i) atomicOr((unsigned long long *)errs, (unsigned long long)E_DEPS);
}

// ---------------------------------------------------------------- register: evaluation

struct EvalOut {
    uint8_t *outcome;
    uint64_t *um, *ul;
    int32_t *un;
    uint32_t *dmiss;    // [ND] the dep is absent from its key's entries
    uint32_t *nr;       // [NP] the pair becomes a record
    uint32_t *rdc;      // [NP] deps the record keeps
    unsigned long long *counts;   // ready, pending commit, pending apply
};

__device__ __forceinline__ void finish(const In &d, const EvalOut &o, uint32_t j, uint32_t n, bool ready, bool wta, bool has_x,
                                       const Ts &x)
{
    const uint32_t a = d.dep_off[j], b = d.dep_off[j + 1];
    uint32_t oc = ACC_UNM_READY;
    Ts u{ 0, 0, 0 };
    if (n != 0 && !ready) {
        if (wta && has_x) { oc = ACC_UNM_PENDING_APPLY; u = x; }
        else { oc = ACC_UNM_PENDING_COMMIT; u = dep_of(d, b - 1); }
    }
    o.outcome[j] = (uint8_t)oc;
    o.um[j] = u.m; o.ul[j] = u.l; o.un[j] = u.n;
    o.nr[j] = oc != ACC_UNM_READY;
    o.rdc[j] = oc == ACC_UNM_PENDING_COMMIT ? b - a : 0u;
    // one atomic per wave and outcome (the lanes that reach here; the wave tier's lane 0 alone)
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        const unsigned long long b = __ballot(oc == c);
        if (b && lane_id() == (uint32_t)__ffsll((long long)b) - 1u) atomicAdd(o.counts + c, (unsigned long long)__popcll(b));
    }
}

// registerUnmanaged :1430-1441 for one dep that the segment holds at entry e; returns whether the entry's executeAt
// (ex) enters executesAt
__device__ __forceinline__ bool see(const CfkResident &s, uint32_t e, bool aod, const Ts &wx, bool &ready, bool &wta, Ts &ex)
{
    const uint32_t st = s.st[e];
    if (st < ACC_ST_COMMITTED) { ready = wta = false; return false; }
    ex = x_of(s, e);
    if (!aod && cmp(ex, wx) >= 0) return false;
    ready &= st >= ACC_ST_APPLIED;
    return true;
}

__global__ __launch_bounds__(BLOCK) void k_um_eval_lane(In d, CfkResident s, Pairs p, uint32_t forced, EvalOut o)
{
    const uint64_t j64 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j64 >= d.NP) return;
    const uint32_t j = (uint32_t)j64, b = d.dep_off[j + 1];
    uint32_t i = p.cut[j];
    if (i == NONE) return;   // malformed offsets: the call fails
    const uint32_t n = b - i;
    if (tier_of(n, forced) != T_LANE) return;
    const uint32_t w = p.waiter[j], k = p.kidx[j];
    const bool aod = awaits_only_deps(d.tl[w]);
    const Ts wx{ d.xm[w], d.xl[w], d.xn[w] };
    bool ready = true, wta = true, has_x = false;
    Ts x{ 0, 0, 0 };
    if (n) {
        const uint32_t e1 = k == NONE ? 0u : s.ent_off[k + 1];
        uint32_t e = k == NONE ? 0u : lower_bound_ts(s.em, s.el, s.en, s.ent_off[k], e1, dep_of(d, i));
        while (i < b) {
            const int c = e == e1 ? -1 : cmp(dep_of(d, i), id_of(s, e));
            if (c == 0) {   // Timestamp.nonNullOrMax: of two equal executeAts the earlier stays
                Ts ex;
                if (see(s, e, aod, wx, ready, wta, ex) && (!has_x || cmp(x, ex) < 0)) { x = ex; has_x = true; }
                ++i; ++e;
            }
            else if (c > 0) ++e;
            else { ready = wta = false; o.dmiss[i] = 1; ++i; }
        }
    }
    finish(d, o, j, n, ready, wta, has_x, x);
}

__global__ __launch_bounds__(BLOCK) void k_um_eval_wave(uint64_t first, In d, CfkResident s, Pairs p, uint32_t forced, EvalOut o)
{
    const uint64_t j64 = first + (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (j64 >= d.NP) return;   // (the whole wave)
    const uint32_t j = (uint32_t)j64, b = d.dep_off[j + 1];
    const uint32_t i0 = p.cut[j];
    if (i0 == NONE) return;   // malformed offsets: the call fails
    const uint32_t n = b - i0;
    if (tier_of(n, forced) != T_WAVE) return;
    const uint32_t w = p.waiter[j], k = p.kidx[j], lane = lane_id();
    const bool aod = awaits_only_deps(d.tl[w]);
    const Ts wx{ d.xm[w], d.xl[w], d.xn[w] };
    const uint32_t e0 = k == NONE ? 0u : s.ent_off[k], e1 = k == NONE ? 0u : s.ent_off[k + 1];
    bool ready = true, wta = true, has_x = false;
    Ts x{ 0, 0, 0 };
    uint32_t xi = NONE;   // the dep x came from
    uint32_t e = e0;
    for (uint32_t i = i0 + lane; i < b; i += 64) {
        const Ts t = dep_of(d, i);
        e = gallop_entry(s, e, e1, t);
        if (e < e1 && cmp(id_of(s, e), t) == 0) {
            Ts ex;
            if (see(s, e, aod, wx, ready, wta, ex) && (!has_x || cmp(x, ex) < 0)) { x = ex; xi = i; has_x = true; }
        } else {
            ready = wta = false;
            o.dmiss[i] = 1;
        }
    }
    ready = __ballot(!ready) == 0;
    wta = __ballot(!wta) == 0;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const Ts y{ shfl_xor(x.m, m), shfl_xor(x.l, m), (int32_t)shfl_xor((uint32_t)x.n, m) };
        const uint32_t yi = shfl_xor(xi, m);
        const bool yh = shfl_xor((uint32_t)has_x, m) != 0;
        if (yh) {
            const int c = has_x ? cmp(y, x) : 1;
            if (c > 0 || (c == 0 && yi < xi)) { x = y; xi = yi; has_x = true; }
        }
    }
    if (lane == 0) finish(d, o, j, n, ready, wta, has_x, x);
}

// ---------------------------------------------------------------- register: the missing (key, TxnId), sorted unique

__global__ __launch_bounds__(BLOCK) void k_um_miss_emit(In d, const uint32_t *__restrict__ dmiss, const uint32_t *__restrict__ dpos,
                                                        uint32_t *__restrict__ msrc, uint64_t *__restrict__ mkey)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= d.ND || !dmiss[i]) return;
    const uint32_t q = dpos[i];
    msrc[q] = (uint32_t)i;
    mkey[q] = d.key[seg_of(d.dep_off, (uint32_t)d.NP, (uint32_t)i)];
}

// sort word `word` of the element at sorted position r: 0 node, 1 lsb, 2 msb (ts.hpp's word order), 3 the key code
__global__ __launch_bounds__(BLOCK) void k_um_sortkey(uint32_t M, int word, const uint32_t *__restrict__ perm, In d,
                                                      const uint32_t *__restrict__ msrc, const uint64_t *__restrict__ mkey,
                                                      uint64_t *__restrict__ key)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= M) return;
    const uint32_t q = perm ? perm[r] : r, i = msrc[q];
    key[r] = word == 0 ? ts_w2(d.dn[i]) : word == 1 ? ts_w1(d.dl[i]) : word == 2 ? d.dm[i] : mkey[q];
}

// run heads of the sorted list: hflag = the first of each (key, TxnId), kflag = the first of each key the store lacks
__global__ __launch_bounds__(BLOCK) void k_um_heads(uint32_t M, const uint32_t *__restrict__ perm, In d, const uint32_t *__restrict__ msrc,
                                                    const uint64_t *__restrict__ mkey, CfkResident s, uint32_t *__restrict__ hflag,
                                                    uint32_t *__restrict__ kflag)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= M) return;
    const uint32_t q = perm[r];
    const uint64_t c = mkey[q];
    bool khead = r == 0, head = r == 0;
    if (r > 0) {
        const uint32_t q0 = perm[r - 1];
        khead = mkey[q0] != c;
        head = khead || cmp(dep_of(d, msrc[q0]), dep_of(d, msrc[q])) != 0;
    }
    hflag[r] = head;
    if (khead) {
        khead = find_sorted(s.key, s.nk, c) == NONE;
    }
    kflag[r] = khead;
}

struct Adds {
    uint32_t nu, nkn;
    const uint64_t *ukey;   // [nu] the additions' keys, ascending
    const uint32_t *usrc;   // [nu] the dep that names each addition's TxnId
    const uint64_t *nkey;   // [nkn] the keys the store lacks, ascending
};

__global__ __launch_bounds__(BLOCK) void k_um_uniq(uint32_t M, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ msrc,
                                                   const uint64_t *__restrict__ mkey, const uint32_t *__restrict__ hflag,
                                                   const uint32_t *__restrict__ hpos, const uint32_t *__restrict__ kflag,
                                                   const uint32_t *__restrict__ kpos, uint64_t *__restrict__ ukey,
                                                   uint32_t *__restrict__ usrc, uint64_t *__restrict__ nkey)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= M || !hflag[r]) return;
    const uint32_t q = perm[r];
    ukey[hpos[r]] = mkey[q];
    usrc[hpos[r]] = msrc[q];
    if (kflag[r]) nkey[kpos[r]] = mkey[q];
}

// ---------------------------------------------------------------- register: placement by rank

struct StateOut {
    uint64_t *key;
    uint32_t *ent_off;
    uint64_t *em, *el, *xm, *xl;
    int32_t *en, *xn;
    uint8_t *st;
    uint32_t *mcnt;
};

// additions with (key, TxnId) < (c, t)
__device__ __forceinline__ uint32_t adds_below(const Adds &a, const In &d, uint64_t c, const Ts &t)
{
    return partition_point(0u, a.nu, [&](uint32_t m) {
        const uint64_t mk = a.ukey[m];
        return mk < c || (mk == c && cmp(dep_of(d, a.usrc[m]), t) < 0);
    });
}

// the key list merged: an old key moves up by the new keys below it, a new key by the old keys below it; each key's
// first entry moves up by the additions on lower keys
__global__ __launch_bounds__(BLOCK) void k_um_place_keys(CfkResident s, uint32_t ne, Adds a, StateOut o)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= s.nk + a.nkn) return;
    if (i == 0) o.ent_off[s.nk + a.nkn] = ne + a.nu;
    if (i < s.nk) {
        const uint64_t c = s.key[i];
        const uint32_t dst = i + lower_bound(a.nkey, 0, a.nkn, c);
        o.key[dst] = c;
        o.ent_off[dst] = s.ent_off[i] + lower_bound(a.ukey, 0, a.nu, c);
    } else {
        const uint32_t i2 = i - s.nk;
        const uint64_t c = a.nkey[i2];
        const uint32_t pk = lower_bound(s.key, 0, s.nk, c);
        o.key[i2 + pk] = c;
        o.ent_off[i2 + pk] = (s.nk ? s.ent_off[pk] : 0u) + lower_bound(a.ukey, 0, a.nu, c);
    }
}

__global__ __launch_bounds__(BLOCK) void k_um_place_ent(CfkResident s, uint32_t ne, Adds a, In d, StateOut o)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i64 >= (uint64_t)ne + a.nu) return;
    const uint32_t i = (uint32_t)i64;
    if (i < ne) {
        const uint64_t c = s.key[seg_of(s.ent_off, s.nk, i)];
        const uint32_t dst = i + adds_below(a, d, c, id_of(s, i));
        o.em[dst] = s.em[i]; o.el[dst] = s.el[i]; o.en[dst] = s.en[i];
        o.xm[dst] = s.xm[i]; o.xl[dst] = s.xl[i]; o.xn[dst] = s.xn[i];
        o.st[dst] = s.st[i];
        o.mcnt[dst] = s.miss_off[i + 1] - s.miss_off[i];
    } else {   // TxnInfo.create(id, TRANSITIVELY_KNOWN): executeAt = TxnId, no missing[]
        const uint32_t u = i - ne;
        const uint64_t c = a.ukey[u];
        const Ts t = dep_of(d, a.usrc[u]);
        const uint32_t pk = lower_bound(s.key, 0, s.nk, c);
        uint32_t below = s.nk ? s.ent_off[pk] : 0u;   // the old entries on lower keys
        if (pk < s.nk && s.key[pk] == c) below = lower_bound_ts(s.em, s.el, s.en, s.ent_off[pk], s.ent_off[pk + 1], t);
        const uint32_t dst = u + below;
        o.em[dst] = t.m; o.el[dst] = t.l; o.en[dst] = t.n;
        o.xm[dst] = t.m; o.xl[dst] = t.l; o.xn[dst] = t.n;
        o.st[dst] = ACC_ST_TRANSITIVELY_KNOWN;
        o.mcnt[dst] = 0;
    }
}

// ---------------------------------------------------------------- register: the new records

struct Recs {
    uint64_t *key, *um, *ul, *tm, *tl, *xm, *xl;
    int32_t *un, *tn, *xn;
    uint8_t *pending;
    uint32_t *dep_off;
};

__device__ __host__ inline Recs recs_of(const Table &t)
{
    return Recs{ t.key, t.um, t.ul, t.tm, t.tl, t.xm, t.xl, t.un, t.tn, t.xn, t.pending, t.dep_off };
}

__global__ __launch_bounds__(BLOCK) void k_um_append(In d, const uint32_t *__restrict__ waiter, const uint8_t *__restrict__ outcome,
                                                     const uint64_t *__restrict__ um, const uint64_t *__restrict__ ul,
                                                     const int32_t *__restrict__ un, const uint32_t *__restrict__ nr,
                                                     const uint32_t *__restrict__ roff, const uint32_t *__restrict__ rdo,
                                                     uint32_t n_rec, uint32_t n_dep, uint32_t n_new, uint32_t n_new_dep, Recs t)
{
    const uint64_t j64 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j64 >= d.NP) return;
    const uint32_t j = (uint32_t)j64;
    if (j == 0) t.dep_off[n_rec + n_new] = n_dep + n_new_dep;
    if (!nr[j]) return;
    const uint32_t r = n_rec + roff[j], w = waiter[j];
    t.key[r] = d.key[j];
    t.pending[r] = outcome[j] == ACC_UNM_PENDING_APPLY ? ACC_UNM_APPLY : ACC_UNM_COMMIT;
    t.um[r] = um[j]; t.ul[r] = ul[j]; t.un[r] = un[j];
    t.tm[r] = d.tm[w]; t.tl[r] = d.tl[w]; t.tn[r] = d.tn[w];
    t.xm[r] = d.xm[w]; t.xl[r] = d.xl[w]; t.xn[r] = d.xn[w];
    t.dep_off[r] = n_dep + rdo[j];
}

// ---------------------------------------------------------------- notify

struct Step {
    uint8_t *act;       // 0: untouched, 1: COMMIT -> APPLY in its slot, 2: released
    uint8_t *fl;        // bit 0: re-evaluated from COMMIT in this call
    uint64_t *vm, *vl;  // the record's APPLY waiting_until (zeros: it never had one)
    int32_t *vn;
    uint32_t *evf, *keep;
    unsigned long long *counts;   // re-evaluated, released
};

__global__ __launch_bounds__(BLOCK) void k_um_step(uint32_t n_rec, Recs t, const uint64_t *__restrict__ dm, const uint64_t *__restrict__ dl,
                                                   const int32_t *__restrict__ dn, CfkResident s, Map mp, int has_rb,
                                                   const uint64_t *__restrict__ akey, uint32_t n_asked,
                                                   const uint32_t *__restrict__ min_unc, const uint32_t *__restrict__ next, Step o,
                                                   uint64_t *__restrict__ errs)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_rec) return;
    const uint64_t c = t.key[r];
    const uint32_t k = find_sorted(s.key, s.nk, c);
    uint32_t row = k;          // akey == null: the rows are the store's keys, a key without a CFK has an empty one
    bool asked = true;
    if (akey) {
        row = lower_bound(akey, 0, n_asked, c);
        asked = row < n_asked && akey[row] == c;
    }
    uint32_t act = 0, fl = 0;
    Ts v{ 0, 0, 0 };
    if (asked) {
        const uint32_t mu = row == NONE ? NONE : min_unc[row], nx = row == NONE ? NONE : next[row];
        uint32_t pend = t.pending[r];
        Ts until{ t.um[r], t.ul[r], t.un[r] };
        bool gone = false;
        // COMMIT: findPendingCommit is exclusive (:1277-1279, CEIL), minUncommitted == null -> Timestamp.MAX
        if (pend == ACC_UNM_COMMIT && (mu == NONE || cmp(until, id_of(s, mu)) < 0)) {
            fl = 1;
            atomicAdd(o.counts, 1ull);
            // updatePending :1342-1388
            const uint32_t d1 = t.dep_off[r + 1];
            const Ts bound = has_rb ? mc::point(mp, c) : Ts{ 0, 0, 0 };
            uint32_t i = lower_bound_ts(dm, dl, dn, t.dep_off[r], d1, bound);
            bool ready = true, has_x = false;
            Ts x{ 0, 0, 0 };
            if (i < d1) {
                const bool aod = awaits_only_deps(t.tl[r]);
                const Ts wx{ t.xm[r], t.xl[r], t.xn[r] };
                const uint32_t e1 = k == NONE ? 0u : s.ent_off[k + 1];
                uint32_t e = k == NONE ? 0u : lower_bound_ts(s.em, s.el, s.en, s.ent_off[k], e1, Ts{ dm[i], dl[i], dn[i] });
                while (i < d1 && e < e1) {
                    const int cc = cmp(Ts{ dm[i], dl[i], dn[i] }, id_of(s, e));
                    if (cc > 0) ++e;
                    else if (cc < 0) { atomicOr((unsigned long long *)errs, (unsigned long long)E_ILLEGAL); break; }
                    else {
                        const Ts ex = x_of(s, e);
                        if (aod || cmp(ex, wx) < 0) {
                            ready &= s.st[e] >= ACC_ST_APPLIED;
                            if (!has_x || cmp(x, ex) < 0) x = ex;
                            has_x = true;
                        }
                        ++i; ++e;
                    }
                }
            }
            if (ready) gone = true;
            else { pend = ACC_UNM_APPLY; until = x; v = x; act = 1; }
        } else if (pend == ACC_UNM_APPLY) v = until;
        // APPLY: only if minUncommitted == null || next != null (:1211); next == null -> Timestamp.MAX; exclusive
        if (!gone && pend == ACC_UNM_APPLY && (mu == NONE || nx != NONE) && (nx == NONE || cmp(until, x_of(s, nx)) < 0))
            gone = true;
        if (gone) { act = 2; atomicAdd(o.counts + 1, 1ull); }
    }
    o.act[r] = (uint8_t)act;
    o.fl[r] = (uint8_t)fl;
    o.vm[r] = v.m; o.vl[r] = v.l; o.vn[r] = v.n;
    o.evf[r] = act != 0;
    o.keep[r] = act != 2;
}

struct Events {
    uint8_t *kind, *flags;
    uint64_t *key, *tm, *tl, *um, *ul;
    int32_t *tn, *un;
};

// the events in table order; a converted record takes its APPLY form in its slot; per kept record (new index) the
// deps it keeps and where they lie
__global__ __launch_bounds__(BLOCK) void k_um_emit(uint32_t n_rec, Recs t, Step o, const uint32_t *__restrict__ evpos,
                                                   const uint32_t *__restrict__ kpos, Events e, uint32_t *__restrict__ ncnt,
                                                   uint32_t *__restrict__ nsrc)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_rec) return;
    const uint32_t act = o.act[r];
    if (act) {
        const uint32_t q = evpos[r];
        e.kind[q] = act == 2 ? ACC_UNM_EV_RELEASE : ACC_UNM_EV_TO_APPLY;
        e.flags[q] = o.fl[r];
        e.key[q] = t.key[r];
        e.tm[q] = t.tm[r]; e.tl[q] = t.tl[r]; e.tn[q] = t.tn[r];
        e.um[q] = o.vm[r]; e.ul[q] = o.vl[r]; e.un[q] = o.vn[r];
    }
    if (act == 1) {
        t.pending[r] = ACC_UNM_APPLY;
        t.um[r] = o.vm[r]; t.ul[r] = o.vl[r]; t.un[r] = o.vn[r];
    }
    if (act != 2) {
        const uint32_t q = kpos[r];
        const bool commit = act == 0 && t.pending[r] == ACC_UNM_COMMIT;
        ncnt[q] = commit ? t.dep_off[r + 1] - t.dep_off[r] : 0u;
        nsrc[q] = t.dep_off[r];
    }
}

namespace {

template <class T>
void grow(acc_ctx *ctx, T *&p, size_t keep, size_t cap, std::vector<void *> &old)
{
    T *q = nullptr;
    ACC_HIP(hipMalloc(&q, cap * sizeof(T)));
    if (p && keep) ACC_HIP(hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    if (p) old.push_back(p);
    p = q;
}

// capacity for n_rec records and n_dep deps; the content is kept
void reserve(acc_ctx *ctx, Table &t, size_t n_rec, size_t n_dep)
{
    std::vector<void *> old;
    if (n_rec + 1 > t.cap_rec) {
        const size_t c = n_rec + n_rec / 2 + 64, n = t.n_rec;
        grow(ctx, t.key, n, c, old); grow(ctx, t.um, n, c, old); grow(ctx, t.ul, n, c, old); grow(ctx, t.tm, n, c, old);
        grow(ctx, t.tl, n, c, old); grow(ctx, t.xm, n, c, old); grow(ctx, t.xl, n, c, old); grow(ctx, t.un, n, c, old);
        grow(ctx, t.tn, n, c, old); grow(ctx, t.xn, n, c, old); grow(ctx, t.pending, n, c, old);
        const bool had = t.dep_off != nullptr;
        grow(ctx, t.dep_off, had ? n + 1 : 0, c, old);
        if (!had) ACC_HIP(hipMemsetAsync(t.dep_off, 0, 4, ctx->stream));
        t.cap_rec = c;
    }
    if (n_dep + 1 > t.cap_dep) {
        const size_t c = n_dep + n_dep / 2 + 64, n = (size_t)t.n_dep;
        grow(ctx, t.dm, n, c, old); grow(ctx, t.dl, n, c, old); grow(ctx, t.dn, n, c, old);
        t.cap_dep = c;
    }
    if (!old.empty()) {
        ctx->sync();
        for (void *p : old) (void)hipFree(p);
    }
}

}  // namespace

void table_free(Table &t)
{
    for (void *p : { (void *)t.key, (void *)t.um, (void *)t.ul, (void *)t.tm, (void *)t.tl, (void *)t.xm, (void *)t.xl, (void *)t.un,
                     (void *)t.tn, (void *)t.xn, (void *)t.pending, (void *)t.dep_off, (void *)t.dm, (void *)t.dl, (void *)t.dn })
        (void)hipFree(p);
    t = Table{};
}

static In stage(acc_ctx *ctx, const acc_cfk_unmanaged_in *in)
{
    const uint32_t nw = in->n_waiters, mem = in->mem;
    const uint64_t NP = in->n_pairs, ND = in->n_deps;
    In d{};
    d.nw = nw; d.NP = NP; d.ND = ND;
    d.tm = stage_in(ctx, "um_in_tm", in->txn_id.msb, nw, mem);
    d.tl = stage_in(ctx, "um_in_tl", in->txn_id.lsb, nw, mem);
    d.tn = stage_in(ctx, "um_in_tn", in->txn_id.node, nw, mem);
    d.xm = stage_in(ctx, "um_in_xm", in->execute_at.msb, nw, mem);
    d.xl = stage_in(ctx, "um_in_xl", in->execute_at.lsb, nw, mem);
    d.xn = stage_in(ctx, "um_in_xn", in->execute_at.node, nw, mem);
    d.key_off = stage_in(ctx, "um_in_koff", in->key_off, (size_t)nw + 1, mem);
    d.key = stage_in(ctx, "um_in_key", in->key, NP, mem);
    d.dep_off = stage_in(ctx, "um_in_doff", in->dep_off, NP + 1, mem);
    d.dm = stage_in(ctx, "um_in_dm", in->deps.msb, ND, mem);
    d.dl = stage_in(ctx, "um_in_dl", in->deps.lsb, ND, mem);
    d.dn = stage_in(ctx, "um_in_dn", in->deps.node, ND, mem);
    return d;
}

Registered register_eval(acc_ctx *ctx, const acc_maxconflicts *rb, const CfkResident &s, uint64_t ne, uint64_t nm, Table &t,
                         const acc_cfk_unmanaged_in *in, acc_cfk_unmanaged_out *out)
{
    hipStream_t st = ctx->stream;
    const uint32_t nw = in->n_waiters, forced = in->tier;
    const uint64_t NP = in->n_pairs, ND = in->n_deps;
    if (NP >= 0xFFFFFFFFull || ND >= 0xFFFFFFFFull) fail(ACC_E_CAP, "more than 2^32-2 pairs / deps");
    const In d = stage(ctx, in);
    const int has_rb = rb && rb->nv;
    const Map mp = has_rb ? mc_map(rb) : Map{};
    Registered R;
    R.n_pairs = NP;
    R.in = d;

    // ---- 1. validation
    uint64_t *errs = ctx->get<uint64_t>("um_errs", 1);
    unsigned long long *counts = ctx->get<unsigned long long>("um_counts", 3);
    ACC_HIP(hipMemsetAsync(errs, 0, 8, st));
    ACC_HIP(hipMemsetAsync(counts, 0, 24, st));
    uint64_t *w[3] = { ctx->get<uint64_t>("um_w0", nw), ctx->get<uint64_t>("um_w1", nw), ctx->get<uint64_t>("um_w2", nw) };
    launch(ctx, "um_waiters", k_um_waiters, dim3(grid_for(nw, BLOCK)), dim3(BLOCK), 0, d, errs, w[0], w[1], w[2]);
    const uint64_t *words[3] = { w[0], w[1], w[2] };
    const DenseRank dr = dense_rank(ctx, "um_dr", nw, 3, words, nullptr, nullptr, false);
    {   // the waiters first: the pair pass finds each pair's waiter through key_off
        ReadBack rbk(ctx);
        const auto h_err = rbk.u64(errs), h_cnt = rbk.u64(dr.count_dev);
        rbk.wait();
        const uint64_t e = h_err;
        if (e & E_KIND) fail(ACC_E_ARG, "Kind.ofOrdinal: invalid kind ordinal in a waiter's TxnId flags");
        if (e & E_MANAGED) fail(ACC_E_ARG, "a key-domain, globally visible waiter is managed by CommandsForKey, not Unmanaged");
        if (e & E_OFF) fail(ACC_E_ARG, "key_off must start at 0, be non-decreasing and end at n_pairs");
        if ((uint64_t)h_cnt != nw) fail(ACC_E_ARG, "waiter TxnIds of one call must be distinct");
    }
    const Pairs P{ ctx->get<uint32_t>("um_waiter", NP), ctx->get<uint32_t>("um_kidx", NP), ctx->get<uint32_t>("um_cut", NP) };
    if (NP) launch(ctx, "um_pairs", k_um_pairs, dim3(grid_for(NP, BLOCK)), dim3(BLOCK), 0, d, mp, has_rb, s, P, errs);
    if (NP && ND) launch(ctx, "um_deporder", k_um_deporder, dim3(grid_for(ND, BLOCK)), dim3(BLOCK), 0, d, errs);

    // ---- 2. evaluation
    EvalOut E{};
    E.outcome = ctx->get<uint8_t>("um_outcome", NP);
    E.um = ctx->get<uint64_t>("um_um", NP); E.ul = ctx->get<uint64_t>("um_ul", NP); E.un = ctx->get<int32_t>("um_un", NP);
    E.dmiss = ctx->get<uint32_t>("um_dmiss", ND);
    E.nr = ctx->get<uint32_t>("um_nr", NP); E.rdc = ctx->get<uint32_t>("um_rdc", NP);
    E.counts = counts;
    if (ND) ACC_HIP(hipMemsetAsync(E.dmiss, 0, ND * 4, st));
    if (NP && forced != T_WAVE)
        launch(ctx, "um_eval_lane", k_um_eval_lane, dim3(grid_for(NP, BLOCK)), dim3(BLOCK), 0, d, s, P, forced, E);
    if (NP && forced != T_LANE) launch_waves(ctx, "um_eval_wave", k_um_eval_wave, NP, d, s, P, forced, E);

    // ---- 3. scans and the read-back
    uint32_t *dpos = ctx->get<uint32_t>("um_dpos", ND + 1), *roff = ctx->get<uint32_t>("um_roff", NP + 1);
    uint32_t *rdo = ctx->get<uint32_t>("um_rdo", NP + 1);
    {
        const uint32_t *in3[3] = { E.dmiss, E.nr, E.rdc };
        uint32_t *out3[3] = { dpos, roff, rdo }, *tot3[3] = { dpos + ND, roff + NP, rdo + NP };
        const size_t n3[3] = { ND, NP, NP };
        scan_multi<uint32_t, OpAdd<uint32_t>>(ctx, 3, in3, out3, n3, true, tot3);
    }
    uint32_t M = 0;
    {
        ReadBack rbk(ctx);
        const auto h_err = rbk.u64(errs);
        const auto h_m = rbk.u32(dpos + ND), h_nr = rbk.u32(roff + NP), h_nd = rbk.u32(rdo + NP);
        const auto h_c = rbk.words((const uint64_t *)counts, 3);
        rbk.wait();
        const uint64_t e = h_err;
        if (e & E_KEYS) fail(ACC_E_ARG, "keys of a waiter must be sorted and unique");
        if (e & E_DEPOFF) fail(ACC_E_ARG, "dep_off must start at 0, be non-decreasing and end at n_deps");
        if (e & E_DEPS) fail(ACC_E_ARG, "deps of a pair must be sorted and unique");
        M = h_m; R.n_new_rec = h_nr; R.n_new_dep = h_nd;
        R.ready = h_c[ACC_UNM_READY]; R.pending_commit = h_c[ACC_UNM_PENDING_COMMIT]; R.pending_apply = h_c[ACC_UNM_PENDING_APPLY];
        if (M > ND || R.n_new_rec > NP || R.n_new_dep > ND) fail(ACC_E_STATE, "internal: more missing deps or records than given");
    }
    if ((uint64_t)t.n_rec + R.n_new_rec >= 0xFFFFFFFFull || t.n_dep + R.n_new_dep >= 0xFFFFFFFFull)
        fail(ACC_E_CAP, "the pending table would hold 2^32-1 records or deps");
    if (R.n_new_rec) reserve(ctx, t, (size_t)t.n_rec + R.n_new_rec, (size_t)(t.n_dep + R.n_new_dep));
    *out = acc_cfk_unmanaged_out{ NP, 0, E.outcome, acc_ts_cols{ E.um, E.ul, E.un } };
    if (M == 0) return R;
    if (ne + M >= 0xFFFFFFFFull) fail(ACC_E_CAP, "more than 2^32-2 CommandsForKey entries");

    // ---- 4. the missing (key, TxnId), sorted, unique
    uint32_t *msrc = ctx->get<uint32_t>("um_msrc", M);
    uint64_t *mkey = ctx->get<uint64_t>("um_mkey", M);
    launch(ctx, "um_miss_emit", k_um_miss_emit, dim3(grid_for(ND, BLOCK)), dim3(BLOCK), 0, d, (const uint32_t *)E.dmiss,
           (const uint32_t *)dpos, msrc, mkey);
    uint64_t *skey = ctx->get<uint64_t>("um_skey", M);
    static const char *const tag[4] = { "um_s0", "um_s1", "um_s2", "um_s3" };
    const int bits[4] = { 32, 64, 64, 64 };
    const uint32_t *perm = nullptr;
    for (int wd = 0; wd < 4; ++wd) {
        launch(ctx, "um_sortkey", k_um_sortkey, dim3(grid_for(M, BLOCK)), dim3(BLOCK), 0, M, wd, perm, d, (const uint32_t *)msrc,
               (const uint64_t *)mkey, skey);
        perm = radix_sort(ctx, tag[wd], skey, perm, M, bits[wd]).vals;
    }
    uint32_t *hflag = ctx->get<uint32_t>("um_hflag", M), *kflag = ctx->get<uint32_t>("um_kflag", M);
    uint32_t *hpos = ctx->get<uint32_t>("um_hpos", (size_t)M + 1), *kpos = ctx->get<uint32_t>("um_kpos", (size_t)M + 1);
    launch(ctx, "um_heads", k_um_heads, dim3(grid_for(M, BLOCK)), dim3(BLOCK), 0, M, perm, d, (const uint32_t *)msrc,
           (const uint64_t *)mkey, s, hflag, kflag);
    {
        const uint32_t *in2[2] = { hflag, kflag };
        uint32_t *out2[2] = { hpos, kpos }, *tot2[2] = { hpos + M, kpos + M };
        const size_t n2[2] = { M, M };
        scan_multi<uint32_t, OpAdd<uint32_t>>(ctx, 2, in2, out2, n2, true, tot2);
    }
    uint32_t NU = 0, NKN = 0;
    {
        ReadBack rbk(ctx);
        const auto h_u = rbk.u32(hpos + M), h_k = rbk.u32(kpos + M);
        rbk.wait();
        NU = h_u; NKN = h_k;
        if (NU == 0 || NU > M || NKN > NU) fail(ACC_E_STATE, "internal: run heads of the missing deps");
    }
    if ((uint64_t)s.nk + NKN >= 0xFFFFFFFFull) fail(ACC_E_CAP, "more than 2^32-2 keys");
    uint64_t *ukey = ctx->get<uint64_t>("um_ukey", NU), *nkey = ctx->get<uint64_t>("um_nkey", NKN);
    uint32_t *usrc = ctx->get<uint32_t>("um_usrc", NU);
    launch(ctx, "um_uniq", k_um_uniq, dim3(grid_for(M, BLOCK)), dim3(BLOCK), 0, M, perm, (const uint32_t *)msrc, (const uint64_t *)mkey,
           (const uint32_t *)hflag, (const uint32_t *)hpos, (const uint32_t *)kflag, (const uint32_t *)kpos, ukey, usrc, nkey);
    const Adds A{ NU, NKN, ukey, usrc, nkey };

    // ---- 5. the merged state in the buffers acc_cfk_apply leaves its result in
    const uint32_t nk2 = s.nk + NKN;
    const uint64_t ne2 = ne + NU;
    StateOut o{};
    o.key = ctx->get<uint64_t>("cd_okey", nk2);
    o.ent_off = ctx->get<uint32_t>("cd_oent_off", (size_t)nk2 + 1);
    o.em = ctx->get<uint64_t>("cd_oem", ne2); o.el = ctx->get<uint64_t>("cd_oel", ne2); o.en = ctx->get<int32_t>("cd_oen", ne2);
    o.xm = ctx->get<uint64_t>("cd_oxm", ne2); o.xl = ctx->get<uint64_t>("cd_oxl", ne2); o.xn = ctx->get<int32_t>("cd_oxn", ne2);
    o.st = ctx->get<uint8_t>("cd_ost", ne2);
    uint32_t *omoff = ctx->get<uint32_t>("cd_omoff", ne2 + 1);
    uint64_t *omm = ctx->get<uint64_t>("cd_omm", nm), *oml = ctx->get<uint64_t>("cd_oml", nm);
    int32_t *omn = ctx->get<int32_t>("cd_omn", nm);
    o.mcnt = ctx->get<uint32_t>("um_mcnt", ne2);
    launch(ctx, "um_place_keys", k_um_place_keys, dim3(grid_for(nk2, BLOCK)), dim3(BLOCK), 0, s, (uint32_t)ne, A, o);
    launch(ctx, "um_place_ent", k_um_place_ent, dim3(grid_for(ne2, BLOCK)), dim3(BLOCK), 0, s, (uint32_t)ne, A, d, o);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, o.mcnt, omoff, ne2, true, omoff + ne2);
    if (nm) {
        ACC_HIP(hipMemcpyAsync(omm, s.mm, nm * 8, hipMemcpyDeviceToDevice, st));
        ACC_HIP(hipMemcpyAsync(oml, s.ml, nm * 8, hipMemcpyDeviceToDevice, st));
        ACC_HIP(hipMemcpyAsync(omn, s.mn, nm * 4, hipMemcpyDeviceToDevice, st));
    }
    R.n_inserted = NU;
    out->n_inserted = NU;
    acc_cfk_snap_view &v = R.view;
    v.n_keys = nk2; v.n_entries = ne2; v.n_missing = nm;
    v.key = o.key; v.ent_off = o.ent_off;
    v.txn_id = acc_ts_cols{ o.em, o.el, o.en };
    v.execute_at = acc_ts_cols{ o.xm, o.xl, o.xn };
    v.status = o.st; v.miss_off = omoff;
    v.missing = acc_ts_cols{ omm, oml, omn };
    return R;
}

void register_append(acc_ctx *ctx, Table &t, const Registered &r)
{
    if (r.n_new_rec == 0) return;
    const uint64_t NP = r.n_pairs;
    // the staged input and the per-pair results of register_eval, where it left them
    const In &d = r.in;
    const uint32_t *waiter = ctx->get<uint32_t>("um_waiter", NP), *nr = ctx->get<uint32_t>("um_nr", NP);
    const uint32_t *roff = ctx->get<uint32_t>("um_roff", NP + 1), *rdo = ctx->get<uint32_t>("um_rdo", NP + 1);
    const uint8_t *outcome = ctx->get<uint8_t>("um_outcome", NP);
    const uint64_t *um = ctx->get<uint64_t>("um_um", NP), *ul = ctx->get<uint64_t>("um_ul", NP);
    const int32_t *un = ctx->get<int32_t>("um_un", NP);
    launch(ctx, "um_append", k_um_append, dim3(grid_for(NP, BLOCK)), dim3(BLOCK), 0, d, waiter, outcome, um, ul, un, nr, roff, rdo,
           t.n_rec, (uint32_t)t.n_dep, r.n_new_rec, (uint32_t)r.n_new_dep, recs_of(t));
    if (r.n_new_dep) {
        rb::Cols c{};
        c.s64[0] = d.dm; c.s64[1] = d.dl; c.d64[0] = t.dm + t.n_dep; c.d64[1] = t.dl + t.n_dep;
        c.s32[0] = d.dn; c.d32[0] = t.dn + t.n_dep;
        c.n64 = 2; c.n32 = 1;
        rb_segcopy(ctx, "um_copy_deps", c, r.n_new_dep, rdo + NP, (uint32_t)NP, rdo, d.dep_off);
    }
    ctx->sync();
    t.n_rec += r.n_new_rec;
    t.n_dep += r.n_new_dep;
}

void notify(acc_ctx *ctx, const acc_maxconflicts *rb, const CfkResident &s, Table &t, const uint64_t *akey, uint32_t n_asked,
            const uint32_t *min_unc, const uint32_t *next, acc_cfk_unmanaged_events *out)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = t.n_rec;
    *out = acc_cfk_unmanaged_events{};
    out->n_rec = n;
    ctx->stat("cfk.unmanaged_reevaluated", 0);
    ctx->stat("cfk.unmanaged_released", 0);
    if (n == 0) return;
    const int has_rb = rb && rb->nv;
    const Map mp = has_rb ? mc_map(rb) : Map{};
    uint64_t *errs = ctx->get<uint64_t>("um_errs", 1);
    unsigned long long *counts = ctx->get<unsigned long long>("um_counts", 3);
    ACC_HIP(hipMemsetAsync(errs, 0, 8, st));
    ACC_HIP(hipMemsetAsync(counts, 0, 24, st));
    Step S{};
    S.act = ctx->get<uint8_t>("um_act", n); S.fl = ctx->get<uint8_t>("um_fl", n);
    S.vm = ctx->get<uint64_t>("um_vm", n); S.vl = ctx->get<uint64_t>("um_vl", n); S.vn = ctx->get<int32_t>("um_vn", n);
    S.evf = ctx->get<uint32_t>("um_evf", n); S.keep = ctx->get<uint32_t>("um_keep", n);
    S.counts = counts;
    const Recs T = recs_of(t);
    launch(ctx, "um_step", k_um_step, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, T, (const uint64_t *)t.dm, (const uint64_t *)t.dl,
           (const int32_t *)t.dn, s, mp, has_rb, akey, n_asked, min_unc, next, S, errs);
    uint32_t *evpos = ctx->get<uint32_t>("um_evpos", (size_t)n + 1), *kpos = ctx->get<uint32_t>("um_keeppos", (size_t)n + 1);
    {
        const uint32_t *in2[2] = { S.evf, S.keep };
        uint32_t *out2[2] = { evpos, kpos }, *tot2[2] = { evpos + n, kpos + n };
        const size_t n2[2] = { n, n };
        scan_multi<uint32_t, OpAdd<uint32_t>>(ctx, 2, in2, out2, n2, true, tot2);
    }
    uint32_t NE = 0, NK = 0;
    uint64_t n_re = 0, n_rel = 0;
    {
        ReadBack rbk(ctx);
        const auto h_err = rbk.u64(errs);
        const auto h_e = rbk.u32(evpos + n), h_k = rbk.u32(kpos + n);
        const auto h_c = rbk.words((const uint64_t *)counts, 2);
        rbk.wait();
        if ((uint64_t)h_err & E_ILLEGAL)
            fail(ACC_E_STATE, "Transaction not found: a dep of a pending record is absent below the key's last entry (illegalState)");
        NE = h_e; NK = h_k; n_re = h_c[0]; n_rel = h_c[1];
        if (NE > n || NK > n) fail(ACC_E_STATE, "internal: more events or records than records");
    }
    ctx->stat("cfk.unmanaged_reevaluated", n_re);
    ctx->stat("cfk.unmanaged_released", n_rel);
    if (NE == 0) return;   // nothing moved: the table and its view stay as they are
    Events E{ ctx->get<uint8_t>("um_ev_kind", NE), ctx->get<uint8_t>("um_ev_flags", NE), ctx->get<uint64_t>("um_ev_key", NE),
              ctx->get<uint64_t>("um_ev_tm", NE), ctx->get<uint64_t>("um_ev_tl", NE), ctx->get<uint64_t>("um_ev_um", NE),
              ctx->get<uint64_t>("um_ev_ul", NE), ctx->get<int32_t>("um_ev_tn", NE), ctx->get<int32_t>("um_ev_un", NE) };
    uint32_t *ncnt = ctx->get<uint32_t>("um_ncnt", NK), *nsrc = ctx->get<uint32_t>("um_nsrc", NK);
    uint32_t *ndoff = ctx->get<uint32_t>("um_ndoff", (size_t)NK + 1);
    launch(ctx, "um_emit", k_um_emit, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, T, S, (const uint32_t *)evpos, (const uint32_t *)kpos, E,
           ncnt, nsrc);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, ncnt, ndoff, NK, true, ndoff + NK);
    // the stable compaction: the record columns (one segment per old record, empty where it left), then the dep CSR
    uint32_t *iota = ctx->get<uint32_t>("um_iota", n);
    launch(ctx, "um_iota", k_iota, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, iota, (size_t)n);
    uint64_t *c64[7];
    int32_t *c32[3];
    static const char *const n64[7] = { "um_c_key", "um_c_um", "um_c_ul", "um_c_tm", "um_c_tl", "um_c_xm", "um_c_xl" };
    static const char *const n32[3] = { "um_c_un", "um_c_tn", "um_c_xn" };
    for (int i = 0; i < 7; ++i) c64[i] = ctx->get<uint64_t>(n64[i], NK);
    for (int i = 0; i < 3; ++i) c32[i] = ctx->get<int32_t>(n32[i], NK);
    uint8_t *cpend = ctx->get<uint8_t>("um_c_pending", NK);
    uint64_t *const t64[7] = { t.key, t.um, t.ul, t.tm, t.tl, t.xm, t.xl };
    int32_t *const t32[3] = { t.un, t.tn, t.xn };
    {
        rb::Cols a{};
        for (int i = 0; i < 4; ++i) { a.s64[i] = t64[i]; a.d64[i] = c64[i]; }
        a.s32[0] = t.un; a.d32[0] = c32[0]; a.s32[1] = t.tn; a.d32[1] = c32[1];
        a.s8 = t.pending; a.d8 = cpend;
        a.n64 = 4; a.n32 = 2;
        rb_segcopy(ctx, "um_copy_rec", a, NK, kpos + n, n, kpos, iota);
        rb::Cols b{};
        for (int i = 0; i < 3; ++i) { b.s64[i] = t64[4 + i]; b.d64[i] = c64[4 + i]; }
        b.s32[0] = t.xn; b.d32[0] = c32[2];
        b.n64 = 3; b.n32 = 1;
        rb_segcopy(ctx, "um_copy_rec", b, NK, kpos + n, n, kpos, iota);
    }
    uint32_t ND2 = 0;
    {
        ReadBack rbk(ctx);
        const auto h_d = rbk.u32(ndoff + NK);
        rbk.wait();
        ND2 = h_d;
        if (ND2 > t.n_dep) fail(ACC_E_STATE, "internal: a compaction grew the pending deps");
    }
    uint64_t *cdm = ctx->get<uint64_t>("um_c_dm", ND2), *cdl = ctx->get<uint64_t>("um_c_dl", ND2);
    int32_t *cdn = ctx->get<int32_t>("um_c_dn", ND2);
    if (ND2) {
        rb::Cols c{};
        c.s64[0] = t.dm; c.s64[1] = t.dl; c.d64[0] = cdm; c.d64[1] = cdl;
        c.s32[0] = t.dn; c.d32[0] = cdn;
        c.n64 = 2; c.n32 = 1;
        rb_segcopy(ctx, "um_copy_recdeps", c, ND2, ndoff + NK, NK, ndoff, nsrc);
    }
    // back into the table's own arrays (the compacted table is no larger)
    for (int i = 0; i < 7; ++i)
        if (NK) ACC_HIP(hipMemcpyAsync(t64[i], c64[i], (size_t)NK * 8, hipMemcpyDeviceToDevice, st));
    for (int i = 0; i < 3; ++i)
        if (NK) ACC_HIP(hipMemcpyAsync(t32[i], c32[i], (size_t)NK * 4, hipMemcpyDeviceToDevice, st));
    if (NK) ACC_HIP(hipMemcpyAsync(t.pending, cpend, NK, hipMemcpyDeviceToDevice, st));
    if (NK) ACC_HIP(hipMemcpyAsync(t.dep_off, ndoff, ((size_t)NK + 1) * 4, hipMemcpyDeviceToDevice, st));
    else ACC_HIP(hipMemsetAsync(t.dep_off, 0, 4, st));
    if (ND2) {
        ACC_HIP(hipMemcpyAsync(t.dm, cdm, (size_t)ND2 * 8, hipMemcpyDeviceToDevice, st));
        ACC_HIP(hipMemcpyAsync(t.dl, cdl, (size_t)ND2 * 8, hipMemcpyDeviceToDevice, st));
        ACC_HIP(hipMemcpyAsync(t.dn, cdn, (size_t)ND2 * 4, hipMemcpyDeviceToDevice, st));
    }
    ctx->sync();
    t.n_rec = NK;
    t.n_dep = ND2;
    out->n_events = NE;
    out->n_rec = NK;
    out->ev_kind = E.kind; out->ev_flags = E.flags; out->ev_key = E.key;
    out->ev_txn = acc_ts_cols{ E.tm, E.tl, E.tn };
    out->ev_until = acc_ts_cols{ E.um, E.ul, E.un };
}

}  // namespace um
}  // namespace acc
