// cfknotify.hip — execution releases from the resident CommandsForKey store (acc_cfk_notify): for every asked key the
// derived fields of the CommandsForKey constructor (local/CommandsForKey.java:422-470: minUncommitted, next, nextWrite,
// committed[]) and the full-range scan notify(AnyGloballyVisible, 0, committed.length) (:1512-1635), restated in closed
// form (DESIGN.md "acc_cfk_notify") so that no pass walks a key's entries once per candidate.
//
// The asked keys' segments are laid side by side in an "asked entry" index space a = 0 .. nea (aoff[i] .. aoff[i + 1] is
// asked key i; src[a] the acc_cfk_state entry). Over it, all data-parallel:
//   1. k_nt_keys: the asked keys validated (sorted unique) and found in the store; a scan -> aoff;
//   2. k_nt_flags: per entry eight 0/1 flags, scanned exclusively (two scan_multi launches) into the prefix counts
//        PU    committed-class entries with executeAt == TxnId (applied included): already in executeAt order
//        PUc   the unapplied ones of them by class c (Read, Write, SyncPoint | ExclusiveSyncPoint)
//        PNc   uncommitted entries by class
//        PB    committed-class entries with executeAt != TxnId ("bumped", applied included): the only ones to sort;
//   3. the bumped entries compacted (bidx) and ranked per key by (executeAt, TxnId) into bperm, by one of three tiers
//      chosen by the key's bumped count nb:  LANE  nb <= NT_LANE_MAX: one lane per key, insertion sort;
//                                            WAVE  nb <= NT_WAVE_MAX: one wave per key, bitonic sort of the indices in LDS;
//                                            SORT  the rest, all keys at once: four stable radix sorts, least significant
//                                                  word first (node, lsb, msb, key), the project's radix_sort;
//   4. k_nt_bflags: the unapplied flags by class in sorted-bumped order, scanned -> Qc; each bumped entry's rank (binv);
//   5. k_nt_keymin: minUncommitted per key, a binary search on PN;
//   6. k_nt_eval, a thread per entry: committed[] is the merge of the unbumped run and the sorted bumped run, so a
//      candidate's index and its c[] are two prefix differences, one read at its own place in its own run, the other at
//      the place one binary search finds in the other run; u[] is the PN difference at the lower bound of executeAt;
//      missingCount one binary search in missing[]; then the predicate;
//   7. a scan of the event flags, k_nt_emit (the view index of every event as k_cq_emit finds it; rel_keys by integer
//      atomicAdd), k_nt_keyout (ev_off, next, nextWrite: the first unapplied of each run by binary search on the prefix
//      counts, the lesser of the two, nulled by minUncommitted).
// Work per key is O(n log n) in its entries; nothing is candidates x segment length.
#include "cfkquery.hpp"
#include "prims.hpp"
#include "search.hpp"

#include <chrono>

namespace acc {
namespace nt {

constexpr uint32_t NT_LANE_MAX = 16;         // bumped entries of a key the lane tier ranks by default
constexpr uint32_t NT_LANE_FORCE_MAX = 64;   // ... when the lane tier is forced (insertion sort: quadratic)
constexpr uint32_t NT_WAVE_MAX = 1024;       // bumped entries of a key the wave tier holds in LDS (u32 each, per wave)
constexpr uint32_t NONE = 0xFFFFFFFFu;

enum : uint64_t { E_KEYS = 1, E_KIND = 2 };
enum : uint32_t { T_LANE = ACC_NOTIFY_TIER_LANE, T_WAVE = ACC_NOTIFY_TIER_WAVE, T_SORT = ACC_NOTIFY_TIER_SORT };

__host__ __device__ __forceinline__ uint32_t tier_of(uint32_t nb, uint32_t forced)
{
    switch (forced) {
    case T_LANE: return nb <= NT_LANE_FORCE_MAX ? T_LANE : T_SORT;
    case T_WAVE: return nb <= NT_WAVE_MAX ? T_WAVE : T_SORT;
    case T_SORT: return T_SORT;
    default:     return nb <= NT_LANE_MAX ? T_LANE : nb <= NT_WAVE_MAX ? T_WAVE : T_SORT;
    }
}

// the asked entry space and its prefix counts (all [nea + 1] but src / akey [nea])
struct Asked {
    uint32_t nk, nea;
    const uint32_t *aoff;    // [nk + 1]
    const uint32_t *kidx;    // [nk] store key, NONE: no CFK
    const uint32_t *src;     // acc_cfk_state entry
    const uint32_t *akey;    // asked key
    const uint32_t *PU, *PUc[3], *PNc[3], *PB;
};

__device__ __forceinline__ Ts id_of(const CfkResident &s, uint32_t se) { return Ts{ s.em[se], s.el[se], s.en[se] }; }
__device__ __forceinline__ Ts x_of(const CfkResident &s, uint32_t se) { return Ts{ s.xm[se], s.xl[se], s.xn[se] }; }

__global__ __launch_bounds__(BLOCK) void k_nt_keys(uint32_t nk, const uint64_t *__restrict__ key, CfkResident s,
                                                   uint32_t *__restrict__ kidx, uint32_t *__restrict__ cnt, uint64_t *__restrict__ errs)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nk) return;
    uint32_t k = i;
    if (key) {
        const uint64_t c = key[i];
        if (i > 0 && key[i - 1] >= c) atomicOr((unsigned long long *)errs, (unsigned long long)E_KEYS);
        k = find_sorted(s.key, s.nk, c);
    }
    kidx[i] = k;
    cnt[i] = k == NONE ? 0u : s.ent_off[k + 1] - s.ent_off[k];
}

struct Flags { uint32_t *U, *Uc[3], *Nc[3], *B; };

__global__ __launch_bounds__(BLOCK) void k_nt_flags(uint32_t nea, uint32_t nk, const uint32_t *__restrict__ aoff,
                                                    const uint32_t *__restrict__ kidx, CfkResident s, uint32_t *__restrict__ src,
                                                    uint32_t *__restrict__ akey, Flags f, uint64_t *__restrict__ errs)
{
    const uint32_t a = blockIdx.x * BLOCK + threadIdx.x;
    if (a >= nea) return;
    const uint32_t i = seg_of(aoff, nk, a);
    const uint32_t se = s.ent_off[kidx[i]] + (a - aoff[i]);
    src[a] = se;
    akey[a] = i;
    const uint32_t st = s.st[se], cls = kind_class((uint32_t)(s.el[se] >> 1) & 7u);
    if (cls == 3) atomicOr((unsigned long long *)errs, (unsigned long long)E_KIND);
    const bool com = st >= ACC_ST_COMMITTED && st <= ACC_ST_APPLIED, unc = st < ACC_ST_COMMITTED;
    const bool bumped = com && cmp(x_of(s, se), id_of(s, se)) != 0;
    const bool live = com && st != ACC_ST_APPLIED;
    f.U[a] = com && !bumped;
    f.B[a] = bumped;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        f.Uc[c][a] = live && !bumped && cls == c;
        f.Nc[c][a] = unc && cls == c;
    }
}

// the bumped entries in key-major TxnId order, and which of them the sort tier ranks
__global__ __launch_bounds__(BLOCK) void k_nt_bidx(Asked A, const uint32_t *__restrict__ fB, uint32_t forced,
                                                   uint32_t *__restrict__ bidx, uint32_t *__restrict__ sflag)
{
    const uint32_t a = blockIdx.x * BLOCK + threadIdx.x;
    if (a >= A.nea || !fB[a]) return;
    const uint32_t i = A.akey[a], j = A.PB[a];
    bidx[j] = a;
    sflag[j] = tier_of(A.PB[A.aoff[i + 1]] - A.PB[A.aoff[i]], forced) == T_SORT;
}

// asked entries a, b of one key in committed[] order: executeAt, then TxnId (= index) order
__device__ __forceinline__ bool before(const CfkResident &s, const uint32_t *src, uint32_t a, uint32_t b)
{
    const int c = cmp(x_of(s, src[a]), x_of(s, src[b]));
    return c < 0 || (c == 0 && a < b);
}

__global__ __launch_bounds__(BLOCK) void k_nt_rank_lane(Asked A, CfkResident s, uint32_t forced, const uint32_t *__restrict__ bidx,
                                                        uint32_t *__restrict__ bperm)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= A.nk) return;
    const uint32_t b0 = A.PB[A.aoff[i]], nb = A.PB[A.aoff[i + 1]] - b0;
    if (nb == 0 || tier_of(nb, forced) != T_LANE) return;
    for (uint32_t j = 0; j < nb; ++j) {
        const uint32_t v = bidx[b0 + j];
        uint32_t p = j;
        while (p > 0 && before(s, A.src, v, bperm[b0 + p - 1])) { bperm[b0 + p] = bperm[b0 + p - 1]; --p; }
        bperm[b0 + p] = v;
    }
}

__global__ __launch_bounds__(BLOCK) void k_nt_rank_wave(uint64_t first, Asked A, CfkResident s, uint32_t forced,
                                                        const uint32_t *__restrict__ bidx, uint32_t *__restrict__ bperm)
{
    __shared__ uint32_t lds[WAVES][NT_WAVE_MAX];
    const uint64_t wi = first + (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (wi >= A.nk) return;
    const uint32_t i = (uint32_t)wi;
    const uint32_t b0 = A.PB[A.aoff[i]], nb = A.PB[A.aoff[i + 1]] - b0;
    if (nb == 0 || tier_of(nb, forced) != T_WAVE) return;
    const uint32_t lane = lane_id();
    uint32_t *buf = lds[threadIdx.x >> 6];
    uint32_t n2 = 64;
    while (n2 < nb) n2 <<= 1;   // <= NT_WAVE_MAX
    for (uint32_t t = lane; t < n2; t += 64) buf[t] = t < nb ? bidx[b0 + t] : NONE;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    for (uint32_t k = 2; k <= n2; k <<= 1) {
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            for (uint32_t t = lane; t < n2; t += 64) {
                const uint32_t l = t ^ jj;
                if (l > t) {
                    const uint32_t x = buf[t], y = buf[l];
                    // x after y; the padding (NONE) after every entry
                    const bool gt = y == NONE ? false : x == NONE ? true : before(s, A.src, y, x);
                    const bool up = (t & k) == 0;
                    if (gt == up && x != y) { buf[t] = y; buf[l] = x; }
                }
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        }
    }
    for (uint32_t t = lane; t < nb; t += 64) bperm[b0 + t] = buf[t];
}

// the sort tier's elements, compacted: sel[t] = their slot in the bumped space
__global__ __launch_bounds__(BLOCK) void k_nt_sel(uint32_t nea, const uint32_t *__restrict__ nb_dev, const uint32_t *__restrict__ sflag,
                                                  const uint32_t *__restrict__ spos, uint32_t *__restrict__ sel)
{
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= nea || j >= *nb_dev || !sflag[j]) return;
    sel[spos[j]] = j;
}

// sort word `word` of the element at sorted position r (perm: the previous pass's order; null: the identity):
// 0 node, 1 lsb, 2 msb in Timestamp.compareTo's word order (ts.hpp), 3 the asked key
__global__ __launch_bounds__(BLOCK) void k_nt_sortkey(uint32_t ns, int word, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ sel,
                                                      const uint32_t *__restrict__ bidx, Asked A, CfkResident s, uint64_t *__restrict__ key)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= ns) return;
    const uint32_t a = bidx[sel[perm ? perm[r] : r]], se = A.src[a];
    key[r] = word == 0 ? ts_w2(s.xn[se]) : word == 1 ? ts_w1(s.xl[se]) : word == 2 ? s.xm[se] : (uint64_t)A.akey[a];
}

// sorted position r is slot sel[r]: the sorted order lists the keys in ascending order, as sel does, with the same counts
__global__ __launch_bounds__(BLOCK) void k_nt_sort_out(uint32_t ns, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ sel,
                                                       const uint32_t *__restrict__ bidx, uint32_t *__restrict__ bperm)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= ns) return;
    bperm[sel[r]] = bidx[sel[perm[r]]];
}

struct BFlags { uint32_t *c[3]; };

__global__ __launch_bounds__(BLOCK) void k_nt_bflags(uint32_t nb, Asked A, CfkResident s, const uint32_t *__restrict__ bperm, BFlags g,
                                                     uint32_t *__restrict__ binv)
{
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= nb) return;
    const uint32_t a = bperm[j];
    if (a >= A.nea) return;   // (every slot is ranked by exactly one tier)
    const uint32_t se = A.src[a];
    binv[a] = j;
    const uint32_t cls = kind_class((uint32_t)(s.el[se] >> 1) & 7u);
    const bool live = s.st[se] != ACC_ST_APPLIED;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) g.c[c][j] = live && cls == c;
}

// first t of [lo, hi) with P[t + 1] > P[lo] (P an exclusive prefix count): the first counted element; hi: none
template <class F>
__device__ __forceinline__ uint32_t first_counted(uint32_t lo, uint32_t hi, F count_through)
{
    return partition_point(lo, hi, [&](uint32_t m) { return count_through(m) == 0; });
}

__global__ __launch_bounds__(BLOCK) void k_nt_keymin(Asked A, uint32_t *__restrict__ kmin)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= A.nk) return;
    const uint32_t s0 = A.aoff[i], s1 = A.aoff[i + 1];
    const uint32_t base = A.PNc[0][s0] + A.PNc[1][s0] + A.PNc[2][s0];
    const uint32_t a = first_counted(s0, s1, [&](uint32_t m) { return A.PNc[0][m + 1] + A.PNc[1][m + 1] + A.PNc[2][m + 1] - base; });
    kmin[i] = a < s1 ? a : NONE;
}

struct Eval {
    const uint32_t *bperm, *binv, *Qc[3], *kmin;
    uint32_t *evflag, *evpos;
    uint8_t *evkind;
    unsigned long long *counts;   // [0] candidates, [1] releases
};

__global__ __launch_bounds__(BLOCK) void k_nt_eval(Asked A, CfkResident s, Eval v)
{
    const uint32_t a = blockIdx.x * BLOCK + threadIdx.x;
    bool cand = false, rel = false;
    if (a < A.nea) {
        const uint32_t se = A.src[a], st = s.st[se];
        cand = st == ACC_ST_COMMITTED || st == ACC_ST_STABLE;
        uint32_t flag = 0, kind = ACC_NOTIFY_WAITING_TO_EXECUTE, pos = 0;
        if (cand) {
            const uint32_t i = A.akey[a], s0 = A.aoff[i], s1 = A.aoff[i + 1], b0 = A.PB[s0], b1 = A.PB[s1];
            const Ts id = id_of(s, se), x = x_of(s, se);
            const bool bumped = cmp(x, id) != 0;
            uint32_t p, q, lbx;   // its place in the unbumped run, in the sorted bumped run; the lower bound of executeAt
            if (bumped) {
                q = v.binv[a];
                p = partition_point(s0, s1, [&](uint32_t m) {   // unbumped e (executeAt = TxnId) precedes it: (e, e) < (x, id)
                    const Ts e = id_of(s, A.src[m]);
                    const int c = cmp(e, x);
                    return c < 0 || (c == 0 && cmp(e, id) < 0);
                });
                lbx = p > s0 && cmp(id_of(s, A.src[p - 1]), x) == 0 ? p - 1 : p;
            } else {
                p = a;
                lbx = a;
                q = partition_point(b0, b1, [&](uint32_t m) {   // bumped b precedes it: (b.x, b) < (id, id)
                    const uint32_t b = v.bperm[m];
                    const int c = cmp(x_of(s, A.src[b]), id);
                    return c < 0 || (c == 0 && b < a);
                });
            }
            pos = (A.PU[p] - A.PU[s0]) + (q - b0);
            flag = 1;
            if (st == ACC_ST_STABLE) {
                uint32_t w[3];   // (c + u) by class: Read, Write, sync points
#pragma unroll
                for (uint32_t c = 0; c < 3; ++c)
                    w[c] = (A.PUc[c][p] - A.PUc[c][s0]) + (v.Qc[c][q] - v.Qc[c][b0]) + (A.PNc[c][lbx] - A.PNc[c][s0]);
                const uint32_t cls = kind_class((uint32_t)(id.l >> 1) & 7u);
                const uint32_t expect = w[1] + (cls >= 1 ? w[0] : 0u) + (cls == 2 ? w[2] : 0u);
                const uint32_t m0 = s.miss_off[se], m1 = s.miss_off[se + 1];
                uint32_t mc = m1 - m0;
                const uint32_t km = v.kmin[i];
                if (mc > 0 && km != NONE) {
                    const Ts mu = id_of(s, A.src[km]);
                    mc -= lower_bound_ts(s.mm, s.ml, s.mn, m0, m1, mu) - m0;
                }
                rel = expect == mc;
                flag = rel;
                kind = ACC_NOTIFY_RELEASE;
            }
        }
        v.evflag[a] = flag;
        v.evkind[a] = (uint8_t)kind;
        v.evpos[a] = pos;
    }
    const unsigned long long bc = __ballot(cand), br = __ballot(rel);
    if (lane_id() == 0) {
        if (bc) atomicAdd(v.counts, (unsigned long long)__popcll(bc));
        if (br) atomicAdd(v.counts + 1, (unsigned long long)__popcll(br));
    }
}

// entry e as its index in the store's txn-major view (k_cq_emit's lower bound)
__device__ __forceinline__ uint32_t view_index(const CfkResident &s, uint32_t e)
{
    return lower_bound_ts(s.tm, s.tl, s.tn, 0, s.n_txn, id_of(s, e));
}

struct Events { uint32_t *entry, *txn, *pos; uint8_t *kind; uint32_t *rel_keys; };

__global__ __launch_bounds__(BLOCK) void k_nt_emit(Asked A, CfkResident s, const uint32_t *__restrict__ evflag,
                                                   const uint32_t *__restrict__ evoff, const uint8_t *__restrict__ evkind,
                                                   const uint32_t *__restrict__ evpos, Events o)
{
    const uint32_t a = blockIdx.x * BLOCK + threadIdx.x;
    if (a >= A.nea || !evflag[a]) return;
    const uint32_t d = evoff[a], se = A.src[a], t = view_index(s, se);
    o.entry[d] = se;
    o.txn[d] = t;
    o.pos[d] = evpos[a];
    o.kind[d] = evkind[a];
    if (evkind[a] == ACC_NOTIFY_RELEASE && t < s.n_txn) atomicAdd(&o.rel_keys[t], 1u);
}

struct KeyOut { uint32_t *min_unc, *next, *next_write; uint64_t *ev_off; };

// the unapplied committed-class entry of key [s0, s1) with the least (executeAt, TxnId) among class mask `cm`
__device__ __forceinline__ uint32_t least_live(const Asked &A, const CfkResident &s, const Eval &v, uint32_t s0, uint32_t s1,
                                               uint32_t b0, uint32_t b1, uint32_t cm)
{
    auto pu = [&](uint32_t t) { uint32_t r = 0; for (uint32_t c = 0; c < 3; ++c) if ((cm >> c) & 1u) r += A.PUc[c][t]; return r; };
    auto qb = [&](uint32_t t) { uint32_t r = 0; for (uint32_t c = 0; c < 3; ++c) if ((cm >> c) & 1u) r += v.Qc[c][t]; return r; };
    const uint32_t ub = pu(s0), bb = qb(b0);
    const uint32_t u = first_counted(s0, s1, [&](uint32_t m) { return pu(m + 1) - ub; });
    const uint32_t j = first_counted(b0, b1, [&](uint32_t m) { return qb(m + 1) - bb; });
    const uint32_t b = j < b1 ? v.bperm[j] : NONE;
    if (u >= s1) return b;
    if (b == NONE) return u;
    return before(s, A.src, b, u) ? b : u;
}

__global__ __launch_bounds__(BLOCK) void k_nt_keyout(Asked A, CfkResident s, Eval v, const uint32_t *__restrict__ evoff, KeyOut o)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= A.nk) return;
    const uint32_t s0 = A.aoff[i], s1 = A.aoff[i + 1], b0 = A.PB[s0], b1 = A.PB[s1];
    o.ev_off[i] = evoff[s0];
    if (i + 1 == A.nk) o.ev_off[A.nk] = evoff[A.nea];
    const uint32_t km = v.kmin[i];
    uint32_t nx = least_live(A, s, v, s0, s1, b0, b1, 7u), nw = least_live(A, s, v, s0, s1, b0, b1, 2u);
    if (km != NONE) {   // minUncommitted.compareTo(next.executeAt) < 0 (:451-458)
        const Ts mu = id_of(s, A.src[km]);
        if (nx != NONE && cmp(mu, x_of(s, A.src[nx])) < 0) nx = NONE;
        if (nw != NONE && cmp(mu, x_of(s, A.src[nw])) < 0) nw = NONE;
    }
    o.min_unc[i] = km == NONE ? NONE : A.src[km];
    o.next[i] = nx == NONE ? NONE : A.src[nx];
    o.next_write[i] = nw == NONE ? NONE : A.src[nw];
}

}  // namespace nt

using namespace nt;

void cfk_notify(acc_ctx *ctx, acc_cfk *cfk, const acc_cfk_notify_in *in, acc_cfk_notify_view *out)
{
    if (!cfk || !in || !out) fail(ACC_E_ARG, "null argument");
    if (in->mem != ACC_MEM_HOST && in->mem != ACC_MEM_DEVICE) fail(ACC_E_ARG, "mem must be ACC_MEM_HOST or ACC_MEM_DEVICE");
    if (in->tier > ACC_NOTIFY_TIER_SORT) fail(ACC_E_ARG, "tier must be 0 (default) or ACC_NOTIFY_TIER_LANE / _WAVE / _SORT");
    const CfkResident s = cfk_resident(cfk);
    if (!s.deps && s.n_txn)
        fail(ACC_E_STATE, "the store holds status-only state (acc_cfk_update): it has no key-major CommandsForKey to scan");
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = ctx->stream;
    const uint32_t forced = in->tier;
    const uint32_t nk = in->key_code ? in->n_keys : s.nk;
    const uint64_t *key = in->key_code ? stage_in(ctx, "nt_in_key", in->key_code, nk, in->mem) : nullptr;

    // ---- 1. the asked keys
    uint64_t *errs = ctx->get<uint64_t>("nt_errs", 1);
    unsigned long long *counts = ctx->get<unsigned long long>("nt_counts", 2);
    ACC_HIP(hipMemsetAsync(errs, 0, 8, st));
    ACC_HIP(hipMemsetAsync(counts, 0, 16, st));
    uint32_t *kidx = ctx->get<uint32_t>("nt_kidx", nk), *kcnt = ctx->get<uint32_t>("nt_kcnt", nk);
    uint32_t *aoff = ctx->get<uint32_t>("nt_aoff", (size_t)nk + 1);
    uint64_t *asum = ctx->get<uint64_t>("nt_asum", 1);
    if (nk) launch(ctx, "nt_keys", k_nt_keys, dim3(grid_for(nk, BLOCK)), dim3(BLOCK), 0, nk, key, s, kidx, kcnt, errs);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, kcnt, aoff, nk, true, aoff + nk);
    sum_u32(ctx, kcnt, nk, asum);
    uint32_t nea = 0;
    {
        ReadBack rb(ctx);
        const auto h_err = rb.u64(errs), h_sum = rb.u64(asum);
        rb.wait();
        const uint64_t e = h_err;
        if (e & E_KEYS) fail(ACC_E_ARG, "key_code must be sorted and unique");
        if ((uint64_t)h_sum >= 0xFFFFFFFFull) fail(ACC_E_CAP, "more than 2^32-2 entries in the asked keys");
        nea = (uint32_t)(uint64_t)h_sum;
    }

    // ---- 2. flags and prefix counts
    const size_t np = (size_t)nea + 1;
    uint32_t *src = ctx->get<uint32_t>("nt_src", nea), *akey = ctx->get<uint32_t>("nt_akey", nea);
    static const char *const fn[8] = { "nt_fU", "nt_fUr", "nt_fUw", "nt_fUs", "nt_fNr", "nt_fNw", "nt_fNs", "nt_fB" };
    static const char *const pn[8] = { "nt_pU", "nt_pUr", "nt_pUw", "nt_pUs", "nt_pNr", "nt_pNw", "nt_pNs", "nt_pB" };
    uint32_t *fl[8], *pr[8];
    for (int i = 0; i < 8; ++i) { fl[i] = ctx->get<uint32_t>(fn[i], nea); pr[i] = ctx->get<uint32_t>(pn[i], np); }
    const Flags F{ fl[0], { fl[1], fl[2], fl[3] }, { fl[4], fl[5], fl[6] }, fl[7] };
    if (nea)
        launch(ctx, "nt_flags", k_nt_flags, dim3(grid_for(nea, BLOCK)), dim3(BLOCK), 0, nea, nk, (const uint32_t *)aoff,
               (const uint32_t *)kidx, s, src, akey, F, errs);
    for (int h = 0; h < 2; ++h) {
        const uint32_t *in4[4];
        uint32_t *out4[4], *tot4[4];
        size_t n4[4];
        for (int i = 0; i < 4; ++i) { in4[i] = fl[4 * h + i]; out4[i] = pr[4 * h + i]; tot4[i] = pr[4 * h + i] + nea; n4[i] = nea; }
        scan_multi<uint32_t, OpAdd<uint32_t>>(ctx, 4, in4, out4, n4, true, tot4);
    }
    Asked A{};
    A.nk = nk; A.nea = nea; A.aoff = aoff; A.kidx = kidx; A.src = src; A.akey = akey;
    A.PU = pr[0]; A.PB = pr[7];
    for (int c = 0; c < 3; ++c) { A.PUc[c] = pr[1 + c]; A.PNc[c] = pr[4 + c]; }

    // ---- 3. the bumped entries, ranked per key
    uint32_t *bidx = ctx->get<uint32_t>("nt_bidx", nea), *bperm = ctx->get<uint32_t>("nt_bperm", nea);
    uint32_t *sflag = ctx->get<uint32_t>("nt_sflag", nea), *spos = ctx->get<uint32_t>("nt_spos", np);
    if (nea) {
        ACC_HIP(hipMemsetAsync(sflag, 0, (size_t)nea * 4, st));
        launch(ctx, "nt_bidx", k_nt_bidx, dim3(grid_for(nea, BLOCK)), dim3(BLOCK), 0, A, (const uint32_t *)fl[7], forced, bidx, sflag);
    }
    scan<uint32_t, OpAdd<uint32_t>>(ctx, sflag, spos, nea, true, spos + nea);
    uint32_t NB = 0, NS = 0;
    {
        ReadBack rb(ctx);
        const auto h_err = rb.u64(errs);
        const auto h_nb = rb.u32(pr[7] + nea), h_ns = rb.u32(spos + nea);
        rb.wait();
        const uint64_t e = h_err;
        if (e & E_KIND) fail(ACC_E_STATE, "Invalid Txn.Kind for CommandsForKey: LocalOnly or EphemeralRead (illegalState)");
        NB = h_nb; NS = h_ns;
        if (NB > nea || NS > NB) fail(ACC_E_STATE, "internal: more bumped entries than entries");
    }
    if (NB && nk) {
        if (forced != T_WAVE && forced != T_SORT)
            launch(ctx, "nt_rank_lane", k_nt_rank_lane, dim3(grid_for(nk, BLOCK)), dim3(BLOCK), 0, A, s, forced, (const uint32_t *)bidx, bperm);
        if (forced != T_LANE && forced != T_SORT)
            launch_waves(ctx, "nt_rank_wave", k_nt_rank_wave, nk, A, s, forced, (const uint32_t *)bidx, bperm);
    }
    if (NS) {
        uint32_t *sel = ctx->get<uint32_t>("nt_sel", NS);
        launch(ctx, "nt_sel", k_nt_sel, dim3(grid_for(NB, BLOCK)), dim3(BLOCK), 0, nea, (const uint32_t *)(pr[7] + nea),
               (const uint32_t *)sflag, (const uint32_t *)spos, sel);
        uint64_t *skey = ctx->get<uint64_t>("nt_skey", NS);
        static const char *const tag[4] = { "nt_s0", "nt_s1", "nt_s2", "nt_s3" };
        const int bits[4] = { 32, 64, 64, bits_for(nk ? nk - 1 : 0) };
        const uint32_t *perm = nullptr;
        for (int w = 0; w < 4; ++w) {
            launch(ctx, "nt_sortkey", k_nt_sortkey, dim3(grid_for(NS, BLOCK)), dim3(BLOCK), 0, NS, w, perm, (const uint32_t *)sel,
                   (const uint32_t *)bidx, A, s, skey);
            perm = radix_sort(ctx, tag[w], skey, perm, NS, bits[w]).vals;
        }
        launch(ctx, "nt_sort_out", k_nt_sort_out, dim3(grid_for(NS, BLOCK)), dim3(BLOCK), 0, NS, perm, (const uint32_t *)sel,
               (const uint32_t *)bidx, bperm);
    }

    // ---- 4. unapplied counts by class along the sorted bumped run
    uint32_t *binv = ctx->get<uint32_t>("nt_binv", nea);
    static const char *const gn[3] = { "nt_gr", "nt_gw", "nt_gs" }, *const qn[3] = { "nt_qr", "nt_qw", "nt_qs" };
    uint32_t *gf[3], *qc[3];
    for (int c = 0; c < 3; ++c) { gf[c] = ctx->get<uint32_t>(gn[c], NB); qc[c] = ctx->get<uint32_t>(qn[c], (size_t)NB + 1); }
    if (NB)
        launch(ctx, "nt_bflags", k_nt_bflags, dim3(grid_for(NB, BLOCK)), dim3(BLOCK), 0, NB, A, s, (const uint32_t *)bperm,
               BFlags{ { gf[0], gf[1], gf[2] } }, binv);
    {
        const uint32_t *in3[3] = { gf[0], gf[1], gf[2] };
        uint32_t *out3[3] = { qc[0], qc[1], qc[2] }, *tot3[3] = { qc[0] + NB, qc[1] + NB, qc[2] + NB };
        const size_t n3[3] = { NB, NB, NB };
        scan_multi<uint32_t, OpAdd<uint32_t>>(ctx, 3, in3, out3, n3, true, tot3);
    }

    // ---- 5, 6. minUncommitted, then every candidate
    uint32_t *kmin = ctx->get<uint32_t>("nt_kmin", nk);
    uint32_t *evflag = ctx->get<uint32_t>("nt_evflag", nea), *evpos = ctx->get<uint32_t>("nt_evpos", nea);
    uint32_t *evoff = ctx->get<uint32_t>("nt_evoff", np);
    uint8_t *evkind = ctx->get<uint8_t>("nt_evkind", nea);
    const Eval V{ bperm, binv, { qc[0], qc[1], qc[2] }, kmin, evflag, evpos, evkind, counts };
    if (nk) launch(ctx, "nt_keymin", k_nt_keymin, dim3(grid_for(nk, BLOCK)), dim3(BLOCK), 0, A, kmin);
    if (nea) launch(ctx, "nt_eval", k_nt_eval, dim3(grid_for(nea, BLOCK)), dim3(BLOCK), 0, A, s, V);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, evflag, evoff, nea, true, evoff + nea);
    uint32_t NE = 0;
    uint64_t n_cand = 0, n_rel = 0;
    {
        ReadBack rb(ctx);
        const auto h_ne = rb.u32(evoff + nea);
        const auto h_c = rb.words((const uint64_t *)counts, 2);
        rb.wait();
        NE = h_ne; n_cand = h_c[0]; n_rel = h_c[1];
        if (NE > nea) fail(ACC_E_STATE, "internal: more events than entries");
    }

    // ---- 7. events and per-key rows
    Events E{ ctx->get<uint32_t>("nt_ev_entry", NE), ctx->get<uint32_t>("nt_ev_txn", NE), ctx->get<uint32_t>("nt_ev_pos", NE),
              ctx->get<uint8_t>("nt_ev_kind", NE), ctx->get<uint32_t>("nt_rel_keys", s.n_txn) };
    KeyOut K{ ctx->get<uint32_t>("nt_min_unc", nk), ctx->get<uint32_t>("nt_next", nk), ctx->get<uint32_t>("nt_next_write", nk),
              ctx->get<uint64_t>("nt_ev_off", (size_t)nk + 1) };
    if (s.n_txn) ACC_HIP(hipMemsetAsync(E.rel_keys, 0, (size_t)s.n_txn * 4, st));
    if (NE)
        launch(ctx, "nt_emit", k_nt_emit, dim3(grid_for(nea, BLOCK)), dim3(BLOCK), 0, A, s, (const uint32_t *)evflag,
               (const uint32_t *)evoff, (const uint8_t *)evkind, (const uint32_t *)evpos, E);
    if (nk) launch(ctx, "nt_keyout", k_nt_keyout, dim3(grid_for(nk, BLOCK)), dim3(BLOCK), 0, A, s, V, (const uint32_t *)evoff, K);
    else ACC_HIP(hipMemsetAsync(K.ev_off, 0, 8, st));
    ctx->sync();

    *out = acc_cfk_notify_view{ nk, s.n_txn, NE, K.min_unc, K.next, K.next_write, K.ev_off, E.entry, E.txn, E.pos, E.kind, E.rel_keys };
    ctx->stat("cfk.notify_keys", nk);
    ctx->stat("cfk.notify_candidates", n_cand);
    ctx->stat("cfk.notify_releases", n_rel);
    ctx->stat("cfk.notify_sorted", NS);
    ctx->stat("cfk.notify_us",
              (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
}

}  // namespace acc
