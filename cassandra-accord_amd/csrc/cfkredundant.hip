// cfkredundant.hip — RedundantBefore on the resident CommandsForKey store (acc_cfk_redundant_before):
// CommandsForKey.withRedundantBefore (local/CommandsForKey.java:1654-1684) for every stored key whose
// shardRedundantBefore rose, and the deps.find(shardRedundantBefore) start of the additions / missing merge (:1088-1089)
// as a pre-pass of acc_cfk_apply_deps.
//
// The store's RedundantBefore map (local/RedundantBefore.java: a ReducingRangeMap merged with max), reduced to the
// shardRedundantBefore TxnId of each Entry, is an acc_maxconflicts map (conflicts.hip): disjoint closed intervals over
// the key codes with one Timestamp each, merged pointwise by Timestamp.compareTo max.
//
// One call (rb_merge_map, then rb_prune):
//   1. the input ranges validated (sorted, non-overlapping, start < end); RB_old(k) of every stored key by point lookup;
//      the input as an acc_conflicts_in built on the device (one update per range), merged by mc_update;
//   2. a thread per stored key: RB_new(k) by point lookup, advanced = RB_new > RB_old, pos = the lower bound of RB_new
//      among the key's TxnIds (an entry equal to the bound stays), the key's surviving entry count;
//   3. one scan of the surviving counts and the non-empty flags -> new entry offsets, compacted key indices;
//   4. a thread per surviving entry: its source entry, and where its key dropped a prefix (pos != 0) the lower bound of
//      the bound in its missing[] (an id equal to the bound stays); a scan of the surviving missing counts;
//   5. one read-back: keys advanced and the three new sizes. No key advanced: nothing is rewritten;
//   6. the compacted keys and offsets, then two segmented copies (k_rb_segcopy) of the entry columns (one segment per
//      key: a contiguous suffix of its old entries) and of the missing columns (one segment per entry: a contiguous
//      suffix of its old missing[]). Untouched keys are segments like any other.
// The segmented copy is the bandwidth-bound part: a lane moves four consecutive destination elements of every column,
// a wave 256, with 16-byte stores and, where the four lie in one segment and the source address is 16-byte aligned,
// 16-byte loads; four elements that straddle a segment boundary are read one by one.
#include "cfkredundant.hpp"

#include <algorithm>

namespace acc {
namespace rb {

using mc::Map;

enum : uint64_t { E_RANGE = 1, E_DEPS = 2 };

// ranges sorted, non-overlapping (touching allowed), start < end
__global__ __launch_bounds__(BLOCK) void k_rb_ranges(uint32_t n, const uint64_t *__restrict__ rs, const uint64_t *__restrict__ re,
                                                     uint64_t *__restrict__ err)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (rs[i] >= re[i] || (i > 0 && re[i - 1] > rs[i])) atomicOr((unsigned long long *)err, (unsigned long long)E_RANGE);
}

// the input as MaxConflicts updates: update i holds range i and no key
__global__ __launch_bounds__(BLOCK) void k_rb_mkupd(uint32_t n, uint32_t *__restrict__ key_off, uint32_t *__restrict__ rng_off)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > n) return;
    key_off[i] = 0;
    rng_off[i] = i;
}

// RB(k) of every stored key
__global__ __launch_bounds__(BLOCK) void k_rb_lookup(Map mp, uint32_t nk, const uint64_t *__restrict__ key, uint64_t *__restrict__ bm,
                                                     uint64_t *__restrict__ bl, int32_t *__restrict__ bn)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= nk) return;
    const Ts b = mc::point(mp, key[k]);
    bm[k] = b.m; bl[k] = b.l; bn[k] = b.n;
}

struct Keys {          // per stored key, written by k_rb_key
    uint32_t *cnt;     // surviving entries
    uint32_t *flag;    // cnt != 0
    uint32_t *src;     // old index of its first surviving entry
    uint32_t *trim;    // advanced with pos != 0: its entries' missing[] lose their prefix below the bound
    uint64_t *bm, *bl; // in: RB_old; out: RB_new
    int32_t *bn;
};

__global__ __launch_bounds__(BLOCK) void k_rb_key(Map mp, CfkResident s, Keys o, unsigned long long *__restrict__ advanced)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    bool adv = false;
    if (k < s.nk) {
        const Ts nb = mc::point(mp, s.key[k]), ob{ o.bm[k], o.bl[k], o.bn[k] };
        const uint32_t e0 = s.ent_off[k], e1 = s.ent_off[k + 1];
        uint32_t lo = e0;
        adv = cmp(nb, ob) > 0;
        if (adv) {   // insertPos(0, shardRedundantBefore): the first entry with TxnId >= the bound
            lo = lower_bound_ts(s.em, s.el, s.en, e0, e1, nb);
        }
        o.cnt[k] = e1 - lo;
        o.flag[k] = e1 != lo;
        o.src[k] = lo;
        o.trim[k] = lo != e0;
        o.bm[k] = nb.m; o.bl[k] = nb.l; o.bn[k] = nb.n;
    }
    const unsigned long long b = __ballot(adv);
    if (b && lane_id() == 0) atomicAdd(advanced, (unsigned long long)__popcll(b));
}

// a thread per entry slot of the old state: slot e2 below the new entry count is new entry e2 (its source entry, the
// start of its surviving missing[] and that count); the slots past it count 0, so one scan over the old length serves
__global__ __launch_bounds__(BLOCK) void k_rb_entry(uint64_t ne_old, CfkResident s, Keys k, const uint32_t *__restrict__ keo,
                                                    uint32_t *__restrict__ msrc, uint32_t *__restrict__ mcnt)
{
    const uint64_t e2 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e2 >= ne_old) return;
    if (e2 >= keo[s.nk]) { mcnt[e2] = 0; return; }
    const uint32_t kk = seg_of(keo, s.nk, (uint32_t)e2);
    const uint32_t e = k.src[kk] + ((uint32_t)e2 - keo[kk]);
    uint32_t m0 = s.miss_off[e];
    const uint32_t m1 = s.miss_off[e + 1];
    if (k.trim[kk] && m1 > m0) {   // Arrays.binarySearch(missing, bound): the insert point, or the equal id, which stays
        m0 = lower_bound_ts(s.mm, s.ml, s.mn, m0, m1, ts_at(k.bm, k.bl, k.bn, kk));
    }
    msrc[e2] = m0;
    mcnt[e2] = m1 - m0;
}

// the compacted key list: codes, new entry offsets, each key's first source entry
__global__ __launch_bounds__(BLOCK) void k_rb_keys_out(uint32_t nk, const uint64_t *__restrict__ key, Keys k,
                                                       const uint32_t *__restrict__ keo, const uint32_t *__restrict__ kidx,
                                                       uint64_t *__restrict__ okey, uint32_t *__restrict__ oent_off,
                                                       uint32_t *__restrict__ osrc)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nk) return;
    if (k.flag[i]) {
        const uint32_t d = kidx[i];
        okey[d] = key[i];
        oent_off[d] = keo[i];
        osrc[d] = k.src[i];
    }
    if (i + 1 == nk) oent_off[kidx[nk]] = keo[nk];
}

constexpr uint32_t RB_VEC = 4;   // destination elements per lane

template <class T>
__device__ __forceinline__ bool aligned16(const T *p) { return ((uintptr_t)p & 15u) == 0; }

// Segmented copy. Destination elements [doff[s], doff[s + 1]) come from source elements sstart[s] + 0, 1, ...;
// doff[0] = 0, doff[ns] = n (read from the device: *n_dev), non-decreasing. n_cap bounds the launch.
__global__ __launch_bounds__(BLOCK) void k_rb_segcopy(Cols c, const uint32_t *__restrict__ n_dev, uint32_t ns,
                                                      const uint32_t *__restrict__ doff, const uint32_t *__restrict__ sstart)
{
    const uint64_t d64 = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) * RB_VEC;
    const uint32_t n = *n_dev;
    if (d64 >= n || ns == 0) return;
    const uint32_t d0 = (uint32_t)d64;
    uint32_t sg = seg_of(doff, ns, d0);
    uint32_t send = doff[sg + 1];
    const uint32_t cnt = min(RB_VEC, n - d0);
    uint32_t src[RB_VEC];
    src[0] = sstart[sg] + (d0 - doff[sg]);
    const bool whole = cnt == RB_VEC && d0 + RB_VEC <= send;   // four elements of one segment: consecutive sources
    if (whole) {
#pragma unroll
        for (uint32_t i = 1; i < RB_VEC; ++i) src[i] = src[0] + i;
    } else {
        for (uint32_t i = 1; i < RB_VEC; ++i) {
            src[i] = src[0];
            if (i >= cnt) continue;
            if (d0 + i >= send && sg + 1 < ns) {   // the segment that holds d0 + i: mostly the next one, else past a run of empty ones
                if (sg + 2 <= ns && doff[sg + 2] > d0 + i) ++sg;
                else sg += 1 + seg_of(doff + sg + 1, ns - sg - 1, d0 + i);
                send = doff[sg + 1];
            }
            src[i] = sstart[sg] + (d0 + i - doff[sg]);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q >= c.n64) break;
        const uint64_t *sp = c.s64[q];
        uint64_t *dp = c.d64[q] + d0;
        uint64_t v[RB_VEC];
        if (whole && aligned16(sp + src[0])) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(sp + src[0]);
            const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(sp + src[0] + 2);
            v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < RB_VEC; ++i) v[i] = i < cnt ? sp[src[i]] : 0;
        }
        if (cnt == RB_VEC && aligned16(dp)) {
            *reinterpret_cast<ulonglong2 *>(dp) = make_ulonglong2(v[0], v[1]);
            *reinterpret_cast<ulonglong2 *>(dp + 2) = make_ulonglong2(v[2], v[3]);
        } else {
            for (uint32_t i = 0; i < cnt; ++i) dp[i] = v[i];
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (q >= c.n32) break;
        const int32_t *sp = c.s32[q];
        int32_t *dp = c.d32[q] + d0;
        int32_t v[RB_VEC];
        if (whole && aligned16(sp + src[0])) {
            const int4 a = *reinterpret_cast<const int4 *>(sp + src[0]);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < RB_VEC; ++i) v[i] = i < cnt ? sp[src[i]] : 0;
        }
        if (cnt == RB_VEC && aligned16(dp)) *reinterpret_cast<int4 *>(dp) = make_int4(v[0], v[1], v[2], v[3]);
        else
            for (uint32_t i = 0; i < cnt; ++i) dp[i] = v[i];
    }
    if (c.s8) {
        uint8_t *dp = c.d8 + d0;
        uint32_t w = 0;
#pragma unroll
        for (uint32_t i = 0; i < RB_VEC; ++i)
            if (i < cnt) w |= (uint32_t)c.s8[src[i]] << (8 * i);
        if (cnt == RB_VEC && ((uintptr_t)dp & 3u) == 0) *reinterpret_cast<uint32_t *>(dp) = w;
        else
            for (uint32_t i = 0; i < cnt; ++i) dp[i] = (uint8_t)(w >> (8 * i));
    }
}

}  // namespace rb

// n_cap: a host-side upper bound of *n_dev (sizes the launch)
void rb_segcopy(acc_ctx *ctx, const char *name, const rb::Cols &c, uint64_t n_cap, const uint32_t *n_dev, uint32_t ns,
                const uint32_t *doff, const uint32_t *sstart)
{
    using namespace rb;
    if (n_cap == 0 || ns == 0) return;
    launch(ctx, name, k_rb_segcopy, dim3(grid_for((n_cap + RB_VEC - 1) / RB_VEC, BLOCK)), dim3(BLOCK), 0, c, n_dev, ns, doff, sstart);
}

namespace rb {

// per (update, key) pair: offsets and order validated as acc_cfk_apply does, the lower bound of RB(key) in its deps
__global__ __launch_bounds__(BLOCK) void k_rb_dep_cut(Map mp, uint64_t NP, uint64_t ND, const uint64_t *__restrict__ key,
                                                      const uint32_t *__restrict__ dep_off, const uint64_t *__restrict__ dm,
                                                      const uint64_t *__restrict__ dl, const int32_t *__restrict__ dn,
                                                      uint32_t *__restrict__ cut, uint32_t *__restrict__ cnt, uint64_t *__restrict__ err)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= NP) return;
    uint32_t a = dep_off[j];
    const uint32_t b = dep_off[j + 1];
    bool bad = b < a || b > ND || (j == 0 && a != 0) || (j + 1 == NP && b != ND);
    if (!bad) {
        for (uint32_t i = a + 1; i < b; ++i)
            if (ts_cmp(dm[i - 1], dl[i - 1], dn[i - 1], dm[i], dl[i], dn[i]) >= 0) { bad = true; break; }
    }
    if (bad) {   // nothing below indexes through this pair; the host hands the untrimmed input to acc_cfk_apply
        atomicOr((unsigned long long *)err, (unsigned long long)E_DEPS);
        cut[j] = 0; cnt[j] = 0;
        return;
    }
    const Ts rb = mc::point(mp, key[j]);
    a = lower_bound_ts(dm, dl, dn, a, b, rb);   // deps.find(shardRedundantBefore): the first dep >= the bound
    cut[j] = a;
    cnt[j] = b - a;
}

}  // namespace rb

using namespace rb;

RbInput rb_stage_ranges(acc_ctx *ctx, const acc_cfk_redundant_in *in)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = in->n_ranges;
    RbInput r;
    r.n = n;
    r.rs = stage_in(ctx, "rb_rs", in->rng_start, n, in->mem);
    r.re = stage_in(ctx, "rb_re", in->rng_end, n, in->mem);
    r.bm = stage_in(ctx, "rb_inm", in->bound.msb, n, in->mem);
    r.bl = stage_in(ctx, "rb_inl", in->bound.lsb, n, in->mem);
    r.bn = stage_in(ctx, "rb_inn", in->bound.node, n, in->mem);
    uint64_t *errs = ctx->get<uint64_t>("rb_errs", 1);
    ACC_HIP(hipMemsetAsync(errs, 0, 8, st));
    launch(ctx, "rb_ranges", k_rb_ranges, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, r.rs, r.re, errs);
    ACC_HIP(hipMemcpyAsync(ctx->pinned, errs, 8, hipMemcpyDeviceToHost, st));
    ctx->sync();
    if (ctx->pinned[0] & E_RANGE) fail(ACC_E_ARG, "ranges must be sorted, non-overlapping, start < end");
    return r;
}

void rb_merge_staged(acc_ctx *ctx, acc_maxconflicts *rb, const RbInput &r)
{
    const uint32_t n = r.n;
    uint32_t *ko = ctx->get<uint32_t>("rb_uko", (size_t)n + 1), *ro = ctx->get<uint32_t>("rb_uro", (size_t)n + 1);
    launch(ctx, "rb_mkupd", k_rb_mkupd, dim3(grid_for((size_t)n + 1, BLOCK)), dim3(BLOCK), 0, n, ko, ro);
    acc_conflicts_in ci{};
    ci.mem = ACC_MEM_DEVICE; ci.n_upd = n; ci.end_inclusive = rb->end_inclusive;
    ci.n_keys = 0; ci.n_ranges = n;
    ci.execute_at = acc_ts_cols{ r.bm, r.bl, r.bn };
    ci.key_off = ko; ci.key = nullptr; ci.rng_off = ro; ci.rng_start = r.rs; ci.rng_end = r.re;
    mc_update(ctx, rb, &ci);
}

void rb_merge_map(acc_ctx *ctx, acc_maxconflicts *rb, const acc_cfk_redundant_in *in, const CfkResident &s)
{
    hipStream_t st = ctx->stream;
    const RbInput r = rb_stage_ranges(ctx, in);
    if (s.nk) {   // RB_old of every stored key, before the map moves
        uint64_t *om = ctx->get<uint64_t>("rb_kbm", s.nk), *ol = ctx->get<uint64_t>("rb_kbl", s.nk);
        int32_t *on = ctx->get<int32_t>("rb_kbn", s.nk);
        if (rb->nv)
            launch(ctx, "rb_lookup", k_rb_lookup, dim3(grid_for(s.nk, BLOCK)), dim3(BLOCK), 0, mc_map(rb), s.nk, s.key, om, ol, on);
        else {
            ACC_HIP(hipMemsetAsync(om, 0, (size_t)s.nk * 8, st));
            ACC_HIP(hipMemsetAsync(ol, 0, (size_t)s.nk * 8, st));
            ACC_HIP(hipMemsetAsync(on, 0, (size_t)s.nk * 4, st));
        }
    }
    rb_merge_staged(ctx, rb, r);
}

RbPruned rb_prune(acc_ctx *ctx, const acc_maxconflicts *rb, const CfkResident &s, uint64_t ne, uint64_t nm, acc_cfk_snap_view *view)
{
    hipStream_t st = ctx->stream;
    const uint32_t nk = s.nk;
    RbPruned r;
    r.nk = nk; r.ne = ne; r.nm = nm;
    if (nk == 0 || ne == 0) return r;
    if (ne >= 0xFFFFFFFFull || nm >= 0xFFFFFFFFull) fail(ACC_E_CAP, "more than 2^32-1 entries / missing");
    Keys k{};
    k.cnt = ctx->get<uint32_t>("rb_kcnt", nk); k.flag = ctx->get<uint32_t>("rb_kflag", nk);
    k.src = ctx->get<uint32_t>("rb_ksrc", nk); k.trim = ctx->get<uint32_t>("rb_ktrim", nk);
    k.bm = ctx->get<uint64_t>("rb_kbm", nk); k.bl = ctx->get<uint64_t>("rb_kbl", nk); k.bn = ctx->get<int32_t>("rb_kbn", nk);
    unsigned long long *adv = ctx->get<unsigned long long>("rb_adv", 1);
    ACC_HIP(hipMemsetAsync(adv, 0, 8, st));
    launch(ctx, "rb_key", k_rb_key, dim3(grid_for(nk, BLOCK)), dim3(BLOCK), 0, mc_map(rb), s, k, adv);
    uint32_t *keo = ctx->get<uint32_t>("rb_keo", (size_t)nk + 1), *kidx = ctx->get<uint32_t>("rb_kidx", (size_t)nk + 1);
    {
        const uint32_t *in2[2] = { k.cnt, k.flag };
        uint32_t *out2[2] = { keo, kidx }, *tot2[2] = { keo + nk, kidx + nk };
        const size_t n2[2] = { nk, nk };
        scan_multi<uint32_t, OpAdd<uint32_t>>(ctx, 2, in2, out2, n2, true, tot2);
    }
    // the new state's arrays, sized by the old state (a prune only shrinks): the buffers acc_cfk_apply leaves its
    // result in, so the store adopts either call's result the same way
    uint64_t *okey = ctx->get<uint64_t>("cd_okey", nk);
    uint32_t *oeo = ctx->get<uint32_t>("cd_oent_off", (size_t)nk + 1);
    uint64_t *oem = ctx->get<uint64_t>("cd_oem", ne), *oel = ctx->get<uint64_t>("cd_oel", ne);
    int32_t *oen = ctx->get<int32_t>("cd_oen", ne);
    uint64_t *oxm = ctx->get<uint64_t>("cd_oxm", ne), *oxl = ctx->get<uint64_t>("cd_oxl", ne);
    int32_t *oxn = ctx->get<int32_t>("cd_oxn", ne);
    uint8_t *ost = ctx->get<uint8_t>("cd_ost", ne);
    uint32_t *omoff = ctx->get<uint32_t>("cd_omoff", ne + 1);
    uint64_t *omm = ctx->get<uint64_t>("cd_omm", nm), *oml = ctx->get<uint64_t>("cd_oml", nm);
    int32_t *omn = ctx->get<int32_t>("cd_omn", nm);
    uint32_t *msrc = ctx->get<uint32_t>("rb_msrc", ne), *mcnt = ctx->get<uint32_t>("rb_mcnt", ne);
    launch(ctx, "rb_entry", k_rb_entry, dim3(grid_for(ne, BLOCK)), dim3(BLOCK), 0, ne, s, k, (const uint32_t *)keo, msrc, mcnt);
    // (slots past the new entry count hold 0: omoff[new count] is the total as well as omoff[ne])
    scan<uint32_t, OpAdd<uint32_t>>(ctx, mcnt, omoff, ne, true, omoff + ne);
    // the one read-back: keys advanced, new key / entry / missing counts
    ACC_HIP(hipMemcpyAsync(ctx->pinned, adv, 8, hipMemcpyDeviceToHost, st));
    ACC_HIP(hipMemcpyAsync(ctx->pinned + 1, kidx + nk, 4, hipMemcpyDeviceToHost, st));
    ACC_HIP(hipMemcpyAsync(ctx->pinned + 2, keo + nk, 4, hipMemcpyDeviceToHost, st));
    ACC_HIP(hipMemcpyAsync(ctx->pinned + 3, omoff + ne, 4, hipMemcpyDeviceToHost, st));
    ctx->sync();
    r.advanced = ctx->pinned[0];
    if (r.advanced == 0) return r;
    r.nk = (uint32_t)(ctx->pinned[1] & 0xFFFFFFFFull);
    r.ne = ctx->pinned[2] & 0xFFFFFFFFull;
    r.nm = ctx->pinned[3] & 0xFFFFFFFFull;
    if (r.nk > nk || r.ne > ne || r.nm > nm) fail(ACC_E_STATE, "internal: a prune grew the CommandsForKey state");
    uint32_t *osrc = ctx->get<uint32_t>("rb_osrc", nk);
    launch(ctx, "rb_keys_out", k_rb_keys_out, dim3(grid_for(nk, BLOCK)), dim3(BLOCK), 0, nk, s.key, k, (const uint32_t *)keo,
           (const uint32_t *)kidx, okey, oeo, osrc);
    Cols ce{};
    ce.s64[0] = s.em; ce.s64[1] = s.el; ce.s64[2] = s.xm; ce.s64[3] = s.xl;
    ce.d64[0] = oem; ce.d64[1] = oel; ce.d64[2] = oxm; ce.d64[3] = oxl;
    ce.s32[0] = s.en; ce.s32[1] = s.xn; ce.d32[0] = oen; ce.d32[1] = oxn;
    ce.s8 = s.st; ce.d8 = ost;
    ce.n64 = 4; ce.n32 = 2;
    rb_segcopy(ctx, "rb_copy_ent", ce, r.ne, keo + nk, r.nk, oeo, osrc);
    Cols cm{};
    cm.s64[0] = s.mm; cm.s64[1] = s.ml; cm.d64[0] = omm; cm.d64[1] = oml;
    cm.s32[0] = s.mn; cm.d32[0] = omn;
    cm.n64 = 2; cm.n32 = 1;
    rb_segcopy(ctx, "rb_copy_miss", cm, r.nm, omoff + ne, (uint32_t)r.ne, omoff, msrc);
    view->n_keys = r.nk; view->n_entries = r.ne; view->n_missing = r.nm;
    view->key = okey; view->ent_off = oeo;
    view->txn_id = acc_ts_cols{ oem, oel, oen };
    view->execute_at = acc_ts_cols{ oxm, oxl, oxn };
    view->status = ost; view->miss_off = omoff;
    view->missing = acc_ts_cols{ omm, oml, omn };
    return r;
}

uint64_t rb_trim_deps(acc_ctx *ctx, const acc_maxconflicts *rb, const acc_cfk_updates *up, acc_cfk_updates *out)
{
    hipStream_t st = ctx->stream;
    if (up->mem != ACC_MEM_HOST && up->mem != ACC_MEM_DEVICE) fail(ACC_E_ARG, "mem must be ACC_MEM_HOST or ACC_MEM_DEVICE");
    const uint32_t nu = up->n_upd;
    const uint64_t NP = up->n_pairs, ND = up->n_deps;
    if (nu == 0 && (NP || ND)) fail(ACC_E_ARG, "pairs without updates");
    if (NP >= 0xFFFFFFFFull || ND >= 0xFFFFFFFFull) fail(ACC_E_CAP, "more than 2^32-1 pairs / deps");
    // the updates on the device, under the names acc_cfk_apply stages them by (it takes DEVICE pointers as they are)
    acc_cfk_updates d = *up;
    d.mem = ACC_MEM_DEVICE;
    d.txn_id = acc_ts_cols{ stage_in(ctx, "cd_um", up->txn_id.msb, nu, up->mem), stage_in(ctx, "cd_ul", up->txn_id.lsb, nu, up->mem),
                            stage_in(ctx, "cd_un", up->txn_id.node, nu, up->mem) };
    d.execute_at = acc_ts_cols{ stage_in(ctx, "cd_uxm", up->execute_at.msb, nu, up->mem),
                                stage_in(ctx, "cd_uxl", up->execute_at.lsb, nu, up->mem),
                                stage_in(ctx, "cd_uxn", up->execute_at.node, nu, up->mem) };
    d.status = stage_in(ctx, "cd_ust", up->status, nu, up->mem);
    d.flags = stage_in(ctx, "cd_ufl", up->flags, nu, up->mem);
    d.key_off = stage_in(ctx, "cd_ukoff", up->key_off, (size_t)nu + 1, up->mem);
    d.key = stage_in(ctx, "cd_ukey", up->key, NP, up->mem);
    d.dep_off = stage_in(ctx, "cd_udoff", up->dep_off, NP + 1, up->mem);
    d.deps = acc_ts_cols{ stage_in(ctx, "cd_udm", up->deps.msb, ND, up->mem), stage_in(ctx, "cd_udl", up->deps.lsb, ND, up->mem),
                          stage_in(ctx, "cd_udn", up->deps.node, ND, up->mem) };
    *out = d;
    if (NP == 0 || ND == 0) return 0;
    uint64_t *errs = ctx->get<uint64_t>("rb_errs", 1);
    ACC_HIP(hipMemsetAsync(errs, 0, 8, st));
    uint32_t *cut = ctx->get<uint32_t>("rb_dcut", NP), *cnt = ctx->get<uint32_t>("rb_dcnt", NP);
    uint32_t *ndoff = ctx->get<uint32_t>("rb_ndoff", NP + 1);
    launch(ctx, "rb_dep_cut", k_rb_dep_cut, dim3(grid_for(NP, BLOCK)), dim3(BLOCK), 0, mc_map(rb), NP, ND, d.key, d.dep_off,
           d.deps.msb, d.deps.lsb, d.deps.node, cut, cnt, errs);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, cnt, ndoff, NP, true, ndoff + NP);
    ACC_HIP(hipMemcpyAsync(ctx->pinned, errs, 8, hipMemcpyDeviceToHost, st));
    ACC_HIP(hipMemcpyAsync(ctx->pinned + 1, ndoff + NP, 4, hipMemcpyDeviceToHost, st));
    ctx->sync();
    if (ctx->pinned[0]) return 0;   // acc_cfk_apply reports the malformed input
    const uint64_t nd2 = ctx->pinned[1] & 0xFFFFFFFFull;
    if (nd2 > ND) fail(ACC_E_STATE, "internal: the deps pre-pass grew the deps");
    if (nd2 == ND) return 0;        // nothing below any bound: the input as it is
    uint64_t *ndm = ctx->get<uint64_t>("rb_ndm", nd2), *ndl = ctx->get<uint64_t>("rb_ndl", nd2);
    int32_t *ndn = ctx->get<int32_t>("rb_ndn", nd2);
    Cols c{};
    c.s64[0] = d.deps.msb; c.s64[1] = d.deps.lsb; c.d64[0] = ndm; c.d64[1] = ndl;
    c.s32[0] = d.deps.node; c.d32[0] = ndn;
    c.n64 = 2; c.n32 = 1;
    rb_segcopy(ctx, "rb_copy_deps", c, nd2, ndoff + NP, (uint32_t)NP, ndoff, cut);
    out->n_deps = nd2;
    out->dep_off = ndoff;
    out->deps = acc_ts_cols{ ndm, ndl, ndn };
    return ND - nd2;
}

}  // namespace acc
