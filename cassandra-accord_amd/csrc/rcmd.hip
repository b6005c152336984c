// rcmd.hip — a device-resident range-command store and the RangeDeps of new txns read from it.
//
// The reference keeps a CommandStore's range commands as a live TreeMap<TxnId, RangeCommand>
// (impl/InMemoryCommandStore.java: rangeCommands) that InMemorySafeStore.update adds to per command (:739-762:
// key-domain TxnIds return early, computeIfAbsent, then RangeCommand.update: ranges = ranges == null ? add :
// ranges.with(add), :524-539), and that mapReduceActive -> mapReduceRangesInternal (:863-870, :883-960) asks about the
// incoming txn only. acc_rcmd is that map in HBM:
//   the table   per TxnId in Timestamp.compareTo order: the raw TxnId of its first update, an erased flag
//               (saveStatus >= Erased: never visited, :891-892) and its Ranges, sorted and non-overlapping;
//   the index   the stabbing index over the ranges of the non-erased commands in the form rd_range_dict (rangedeps.hip)
//               leaves it: the dictionary of distinct stored ranges in Range::compare order, the entries in (width
//               class, start) order with (range id, table index) and kind, class_off.
//
// acc_rcmd_update (one stream, every column written once into fresh arrays, which the store then adopts):
//   1. the delta validated; every later loop runs inside the offsets that passed;
//   2. the delta's TxnIds dense-ranked by a stable sort: a TxnId listed several times is one group whose updates stay in
//      array order (Ranges.with is not order-independent);
//   3. each group searched among the stored TxnIds: stored row j moves to j + #inserted below it, an inserted TxnId
//      lands at its insert position + its rank among the inserts;
//   4. k_rc_fold, a lane per touched command: the exact replay of Ranges.with (ranges_with.hpp, the code the host's
//      acc_ranges_with runs) over the command's updates in array order, in two scratch buffers of stored + added ranges
//      that take turns as the sink; the result may also be the stored ranges or an update's ranges themselves (the
//      superset short-cut returns the object it was given), so the lane ends with a pointer and a count;
//   5. one scan of the row counts for rng_off, one write of every column;
//   6. the index rebuilt from the new table by rd_range_dict as it is, and its arrays and the table moved into the
//      store with acc_ctx::swap_buf (the context keeps the store's previous arrays for its next results).
// acc_rcmd_rangedeps: the queries validated; per query two binary searches over the stored TxnId columns (lim = stored
// TxnIds below executeAt, tpos = its own table index or none); then rd_stab_queries and rd_build_txns as they are, with
// the entry columns, class offsets and dictionary pointing at the store.
// acc_rcmd_update_cmds is the same update with the state columns of each command (status, executeAt, HAS_DEPS and the
// flattened PartialDeps: what RangeCommand.command points at); acc_rcmd_update is the call without them. The fold also
// leaves, per touched command, which update its status / executeAt and which its deps come from; k_rc_counts counts the
// deps of every output row beside its ranges, one more scan gives the new dep_off, and k_rc_write takes each row's state
// and deps span from the stored row or from the delta. The deps arrays are rewritten on every update, like the table.
// acc_rcmd_map_reduce_full (the recovery scans, mapReduceRangesInternal :883-960 with every TestStartedAt / TestDep /
// TestStatus): k_rc_qprep's recovery variant gives lim per TestStartedAt (STARTED_BEFORE: #TxnIds < X; ANY: n;
// STARTED_AFTER: n - #TxnIds <= X over a mirrored position column y' = n - 1 - y, so the stabbing pass's "y < lim" admits
// exactly the commands after X) and the Kinds mask; rd_stab_queries as it is lists the (stored range, command)
// candidates of each participant; k_rcr_filter, a wave per participant, tests each candidate's command (recovery_pred.hpp,
// the predicate acc_map_reduce_full_ranges evaluates) and compacts the survivors in place in the participant's span;
// rd_build_txns as it is builds the result.
// acc_rcmd_redundant_before (InMemoryCommandStore.markShardDurable, impl/InMemoryCommandStore.java:346-370, once per
// distinct bound of the input): the input validated and max-merged into the store's RedundantBefore map (the
// acc_maxconflicts form and the two steps of cfkredundant.hpp), then the prune, count -> scan -> emit:
//   1. k_rp_lim, a thread per input range: lim[j] = #stored TxnIds < bound[j] (the table is in compareTo order, so
//      "C below bound j" is row < lim[j]); max lim beside it;
//   2. k_rp_rowner, a thread per row: the owner row of every stored range;
//   3. k_rp_cut<false>, a thread per stored range: the first input range that ends above its start by binary search, then
//      the walk over the intersecting input ranges, those with row >= lim[j] skipped: its surviving pieces counted;
//   4. one scan of the piece counts; k_rp_rows, a thread per row: its new range count, keep = erased || row >= max lim ||
//      count > 0; one scan (four arrays) of keep, the kept rows' range counts and dep counts, and the cut flags;
//   5. one read-back: the three new sizes and the rows cut. Nothing cut or dropped: nothing is rewritten;
//   6. k_rp_write, a thread per row (every row column, the new offsets, the deps' segments); k_rp_cut<true>, the walk of
//      3. again, writing the pieces with their owner, entry flag and the OR masks; the deps by the segmented copy of
//      cfkredundant.hip; then the index and the adoption as an update ends (finish_table).
// Under a non-empty map the updates' ranges are trimmed first (trim_delta): k_rt_owner, k_rt_trim<false>, a scan,
// k_rt_off, one read-back and, if any range changed, k_rt_trim<true>; the fold then runs on the trimmed columns.
// acc_rcmd_partial_rangedeps (the stab result with RedundantBefore.collectDeps' deps) is rcmd_partial.hip: it runs
// acc_rcmd_rangedeps' front end and tail through the rcmd_* functions of rcmd_partial.hpp, and every call here that
// rewrites the table or merges into the map clears the flag of the union index it caches in the store.
// Integer work only: HBM/latency bound, no MFMA.

#include "rcmd_partial.hpp"
#include "ranges_with.hpp"
#include "recovery_pred.hpp"

#include <type_traits>

namespace acc {

namespace rc {

enum : uint64_t {
    E_KIND = 1, E_FLAGS = 2, E_OFF = 4, E_BOUND = 8, E_ORDER = 16, E_STATUS = 32, E_DOFF = 64, E_DEPS = 128,
    // queries
    E_Q_KIND_ARG = 1 << 8, E_Q_KIND_STATE = 1 << 9, E_Q_KOFF = 1 << 10, E_Q_ROFF = 1 << 11, E_Q_RKEYS = 1 << 12,
    E_Q_KRANGES = 1 << 13, E_Q_KEYS = 1 << 14,
};

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t DROP = 0xFFFFFFFEu;   // a deps source: the command holds none

// a command's deps, flattened: (TxnId, key | range) pairs sorted by TxnId
struct DepCols {
    const uint32_t *off;
    const uint64_t *m, *l;
    const int32_t *n;
    const uint64_t *s, *e;
    const uint8_t *k;
};

struct Delta {
    const uint64_t *tm, *tl;
    const int32_t *tn;
    const uint8_t *flags;
    const uint32_t *rng_off;
    const uint64_t *rs, *re;
    uint32_t D, NR;
    // acc_rcmd_update_cmds (state != 0): executeAt, status and deps of every update
    uint32_t state, ND;
    const uint64_t *xm, *xl;
    const int32_t *xn;
    const uint8_t *status;
    DepCols dep;
};

struct Table {
    const uint64_t *tm, *tl;
    const int32_t *tn;
    const uint8_t *flags;
    const uint32_t *rng_off;
    const uint64_t *rs, *re;
    uint32_t n;
    const uint64_t *em, *el;
    const int32_t *en;
    const uint8_t *status;
    DepCols dep;
};

struct TableOut {
    uint64_t *tm, *tl;
    int32_t *tn;
    uint8_t *flags;
    uint32_t *rng_off;
    uint64_t *rs, *re;
    uint64_t *em, *el;
    int32_t *en;
    uint8_t *status;
    uint32_t *dep_off;
    uint64_t *dm, *dl;
    int32_t *dn;
    uint64_t *ds, *de;
    uint8_t *dk;
};

// a Ranges in two columns, and the sink of one with(): what ranges_with.hpp reads and writes on the device
struct Span {
    const uint64_t *s, *e;
    uint32_t n;
    __device__ size_t size() const { return n; }
    __device__ rg::Rg operator[](size_t i) const { return rg::Rg{ s[i], e[i] }; }
};
struct SpanSink {
    uint64_t *s, *e;
    uint32_t n, cap;
    __device__ void push(const rg::Rg &r)
    {
        if (n < cap) { s[n] = r.s; e[n] = r.e; }   // with() stays within left + right <= cap; nothing is written past it
        ++n;
    }
};

// ---------------------------------------------------------------- update

// Per update: Kind.ofOrdinal, the flag bits, offsets that start at 0, do not decrease and end at n_ranges, and
// Ranges.ofSortedAndDeoverlapped with start < end inside them; the TxnId's compare words. A key-domain TxnId
// (InMemorySafeStore.update: txnId.domain() != Range -> return) gets bit 0 of its second word set, which IDENTITY_LSB
// leaves out: it never groups with a range-domain TxnId. g: [0] errors, [1] key-domain updates.
// With state columns, k_rr_check's rules per update: the Status ordinal, dep_off from 0 to n_deps without decreasing and,
// inside it, TxnIds non-decreasing by Timestamp.compareTo, dep_is_key <= 1 and start < end for a range entry.
__global__ __launch_bounds__(BLOCK) void k_rc_validate(Delta d, uint8_t allowed, uint64_t *__restrict__ g, uint64_t *__restrict__ w0,
                                                       uint64_t *__restrict__ w1, uint64_t *__restrict__ w2)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= d.D) return;
    uint64_t e = 0;
    const uint64_t l = d.tl[i];
    if (((l >> 1) & 7u) > ACC_KIND_LOCAL_ONLY) e |= E_KIND;
    if (d.flags[i] & ~allowed) e |= E_FLAGS;
    if (d.state) {
        if (d.status[i] > 10) e |= E_STATUS;
        const uint32_t d0 = d.dep.off[i], d1 = d.dep.off[i + 1];
        if (d1 < d0 || d1 > d.ND || (i == 0 && d0 != 0) || (i == d.D - 1 && d1 != d.ND)) e |= E_DOFF;
        else
            for (uint32_t j = d0; j < d1; ++j) {
                if (d.dep.k[j] > 1 || (!d.dep.k[j] && d.dep.s[j] >= d.dep.e[j])) e |= E_DEPS;
                if (j > d0 && ts_cmp(d.dep.m[j - 1], d.dep.l[j - 1], d.dep.n[j - 1], d.dep.m[j], d.dep.l[j], d.dep.n[j]) > 0) e |= E_DEPS;
            }
    }
    const uint32_t r0 = d.rng_off[i], r1 = d.rng_off[i + 1];
    if (r1 < r0 || r1 > d.NR || (i == 0 && r0 != 0) || (i == d.D - 1 && r1 != d.NR)) e |= E_OFF;
    else
        for (uint32_t j = r0; j < r1; ++j) {
            if (d.rs[j] >= d.re[j]) e |= E_BOUND;
            if (j > r0 && d.re[j - 1] > d.rs[j]) e |= E_ORDER;
        }
    const bool keydom = !(l & 1u);
    w0[i] = d.tm[i];
    w1[i] = (l & IDENTITY_LSB) | (keydom ? 1u : 0u);
    w2[i] = ts_w2(d.tn[i]);
    if (e) atomicOr((unsigned long long *)&g[0], (unsigned long long)e);
    if (keydom) atomicAdd((unsigned long long *)&g[1], 1ull);
}

// gstart[r] = the first position of group r in the sorted delta order; gstart[G] = D
__global__ __launch_bounds__(BLOCK) void k_rc_gstart(uint32_t D, uint32_t G, const uint32_t *__restrict__ perm,
                                                     const uint32_t *__restrict__ rank, uint32_t *__restrict__ gstart)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= D) return;
    const uint32_t r = rank[perm[p]];
    if (p == 0 || rank[perm[p - 1]] != r) gstart[r] = p;
    if (p == 0) gstart[G] = D;
}

// group r (one TxnId of the delta): its lower bound among the stored TxnIds, member or not, and the bound of its
// folded Ranges = the stored ranges + every range its updates list. Key-domain groups: pos = NONE.
__global__ __launch_bounds__(BLOCK) void k_rc_locate(uint32_t G, Delta d, Table s, const uint32_t *__restrict__ first,
                                                     const uint32_t *__restrict__ perm, const uint32_t *__restrict__ gstart,
                                                     uint32_t *__restrict__ pos, uint32_t *__restrict__ isnew,
                                                     uint64_t *__restrict__ bound)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= G) return;
    const uint32_t i0 = first[r];
    const uint64_t xm = d.tm[i0], xl = d.tl[i0];
    const int32_t xn = d.tn[i0];
    if (!(xl & 1u)) { pos[r] = NONE; isnew[r] = 0; bound[r] = 0; return; }
    const uint32_t lo = lower_bound_ts(s.tm, s.tl, s.tn, 0, s.n, Ts{ xm, xl, xn });
    const bool found = lo < s.n && ts_cmp(s.tm[lo], s.tl[lo], s.tn[lo], xm, xl, xn) == 0;
    uint64_t b = found ? (uint64_t)(s.rng_off[lo + 1] - s.rng_off[lo]) : 0ull;
    for (uint32_t p = gstart[r]; p < gstart[r + 1]; ++p) {
        const uint32_t u = perm[p];
        b += d.rng_off[u + 1] - d.rng_off[u];
    }
    pos[r] = lo;
    isnew[r] = found ? 0u : 1u;
    bound[r] = b;
}

// The fold, a lane per touched command: InMemorySafeStore.update per update of the group in array order.
//   erased already (stored, or by an earlier update of the batch): the update changes nothing (st[0] counts it; st[1]
//   counts the stored commands the batch names);
//   an erased update: the command is erased, its ranges leave the table;
//   else ranges = ranges == null ? add : ranges.with(add), replayed by with_of.
// Scratch of group r: two buffers of bound[r] ranges from 2 * boff[r], taking turns as the sink. Leaves the group's
// row, its Ranges as a pointer pair (stored columns, the delta's columns or scratch) and count, and its erased flag.
// With it the sources of its state: ssrc = the update its status and executeAt come from (NONE: the stored row's, or the
// defaults of a row plain acc_rcmd_update inserts), dsrc = the update its deps and HAS_DEPS bit come from (NONE: the
// stored row's, none for an inserted one; DROP: none).
struct Folded {
    uint32_t *row, *cnt;
    uint8_t *erased;
    const uint64_t **ps, **pe;
    uint32_t *ssrc, *dsrc;
};
__global__ __launch_bounds__(BLOCK) void k_rc_fold(uint32_t G, Delta d, Table s, const uint32_t *__restrict__ perm,
                                                   const uint32_t *__restrict__ gstart, const uint32_t *__restrict__ pos,
                                                   const uint32_t *__restrict__ isnew, const uint32_t *__restrict__ newx,
                                                   const uint64_t *__restrict__ boff, uint64_t *__restrict__ scr_s,
                                                   uint64_t *__restrict__ scr_e, uint32_t *__restrict__ grow, Folded f,
                                                   uint64_t *__restrict__ st)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= G) return;
    const uint32_t lo = pos[r];
    if (lo == NONE) { f.row[r] = NONE; return; }
    const uint32_t row = lo + newx[r];
    grow[row] = r;
    f.row[r] = row;
    bool erased = false;
    Span cur{ nullptr, nullptr, 0 };
    if (!isnew[r]) {
        erased = (s.flags[lo] & ACC_RCMD_ERASED) != 0;
        const uint32_t a = s.rng_off[lo];
        if (!erased) cur = Span{ s.rs + a, s.re + a, s.rng_off[lo + 1] - a };
    }
    const uint64_t b0 = boff[r], cap64 = boff[r + 1] - b0;
    const uint32_t cap = (uint32_t)cap64;
    uint64_t *const bs[2] = { scr_s + 2 * b0, scr_s + 2 * b0 + cap64 };
    uint64_t *const be[2] = { scr_e + 2 * b0, scr_e + 2 * b0 + cap64 };
    uint32_t which = 0, ignored = 0, ssrc = NONE, dsrc = NONE;
    for (uint32_t p = gstart[r]; p < gstart[r + 1]; ++p) {
        const uint32_t u = perm[p];
        if (erased) { ++ignored; continue; }
        if (d.state) ssrc = u;
        if (d.flags[u] & ACC_RCMD_ERASED) { erased = true; cur = Span{ nullptr, nullptr, 0 }; dsrc = DROP; continue; }
        if (d.state && !(d.flags[u] & ACC_RCMD_KEEP_DEPS)) dsrc = u;
        const uint32_t a = d.rng_off[u];
        const Span add{ d.rs + a, d.re + a, d.rng_off[u + 1] - a };
        SpanSink sink{ bs[which], be[which], 0, cap };
        const rg::WithResult w = rg::with_of(cur, add, sink);
        if (w == rg::WITH_RIGHT) cur = add;
        else if (w == rg::WITH_SINK) {
            cur = Span{ sink.s, sink.e, sink.n < cap ? sink.n : cap };
            which ^= 1u;   // the next sink is the buffer cur does not lie in
        }
    }
    f.cnt[r] = cur.n;
    f.erased[r] = erased ? 1 : 0;
    f.ps[r] = cur.s;
    f.pe[r] = cur.e;
    f.ssrc[r] = ssrc;
    f.dsrc[r] = dsrc;
    if (ignored) atomicAdd((unsigned long long *)&st[0], (unsigned long long)ignored);
    if (!isnew[r]) atomicAdd((unsigned long long *)&st[1], 1ull);
}

// insf[x] = 1: new row x holds an inserted TxnId
__global__ __launch_bounds__(BLOCK) void k_rc_insflag(uint32_t n2, const uint32_t *__restrict__ grow, const uint32_t *__restrict__ isnew,
                                                      uint32_t *__restrict__ insf)
{
    const uint32_t x = blockIdx.x * BLOCK + threadIdx.x;
    if (x >= n2) return;
    const uint32_t g = grow[x];
    insf[x] = g != NONE && isnew[g] ? 1u : 0u;
}

// ranges of new row x: its group's fold, or the stored row x - #inserted below it; its deps (dcnt, when asked for):
// those of the update the fold named, else the stored row's
__global__ __launch_bounds__(BLOCK) void k_rc_counts(uint32_t n2, Delta d, Table s, const uint32_t *__restrict__ grow,
                                                     const uint32_t *__restrict__ insx, const uint32_t *__restrict__ isnew, Folded f,
                                                     uint64_t *__restrict__ cnt, uint64_t *__restrict__ dcnt)
{
    const uint32_t x = blockIdx.x * BLOCK + threadIdx.x;
    if (x >= n2) return;
    const uint32_t g = grow[x];
    const uint32_t j = x - insx[x];
    const bool stored = g == NONE || !isnew[g];
    cnt[x] = g != NONE ? f.cnt[g] : s.rng_off[j + 1] - s.rng_off[j];
    if (!dcnt) return;
    const uint32_t src = g != NONE ? f.dsrc[g] : NONE;
    uint32_t nd = 0;
    if (src == NONE) nd = stored ? s.dep.off[j + 1] - s.dep.off[j] : 0u;
    else if (src != DROP) nd = d.dep.off[src + 1] - d.dep.off[src];
    dcnt[x] = nd;
}

// every column of new row x, once; the index's per-row inputs with it (rd_range_dict reads tinfo.y = table index,
// rowner, eflag) and the OR of the range starts and of the ends (g[2], g[3]: the bit compaction plans; a bit set in
// every bound rides along, which keeps the order)
__global__ __launch_bounds__(BLOCK) void k_rc_write(uint32_t n2, Delta d, Table s, const uint32_t *__restrict__ first,
                                                    const uint32_t *__restrict__ grow, const uint32_t *__restrict__ insx,
                                                    const uint32_t *__restrict__ isnew, Folded f,
                                                    const uint64_t *__restrict__ off, const uint64_t *__restrict__ doff,
                                                    TableOut o, uint4 *__restrict__ tinfo,
                                                    uint32_t *__restrict__ rowner, uint32_t *__restrict__ eflag,
                                                    uint64_t *__restrict__ g)
{
    const uint32_t x = blockIdx.x * BLOCK + threadIdx.x;
    uint64_t ms = 0, me = 0;
    if (x < n2) {
        const uint32_t gr = grow[x];
        const uint32_t j = x - insx[x];   // the stored row (unless inserted)
        const uint64_t *ps, *pe;
        uint8_t fl;
        if (gr != NONE && isnew[gr]) {
            const uint32_t i0 = first[gr];   // the raw bits of the first update
            o.tm[x] = d.tm[i0]; o.tl[x] = d.tl[i0]; o.tn[x] = d.tn[i0];
        } else {
            o.tm[x] = s.tm[j]; o.tl[x] = s.tl[j]; o.tn[x] = s.tn[j];
        }
        const bool stored = gr == NONE || !isnew[gr];
        const uint32_t ssrc = gr != NONE ? f.ssrc[gr] : NONE, dsrc = gr != NONE ? f.dsrc[gr] : NONE;
        if (gr != NONE) { ps = f.ps[gr]; pe = f.pe[gr]; fl = f.erased[gr] ? (uint8_t)ACC_RCMD_ERASED : (uint8_t)0; }
        else { const uint32_t a = s.rng_off[j]; ps = s.rs + a; pe = s.re + a; fl = s.flags[j] & ACC_RCMD_ERASED; }
        // state: status and executeAt of the update the fold named, else the stored row's, else NotDefined at the TxnId
        if (ssrc != NONE) { o.em[x] = d.xm[ssrc]; o.el[x] = d.xl[ssrc]; o.en[x] = d.xn[ssrc]; o.status[x] = d.status[ssrc]; }
        else if (stored) { o.em[x] = s.em[j]; o.el[x] = s.el[j]; o.en[x] = s.en[j]; o.status[x] = s.status[j]; }
        else { o.em[x] = o.tm[x]; o.el[x] = o.tl[x]; o.en[x] = o.tn[x]; o.status[x] = 0; }
        // deps and HAS_DEPS likewise; doff == nullptr: no command holds deps, before or after
        DepCols dc = s.dep;
        uint32_t db = 0;
        if (dsrc == NONE) {
            if (stored) { fl |= s.flags[j] & ACC_RCMD_HAS_DEPS; db = doff ? s.dep.off[j] : 0u; }
        } else if (dsrc != DROP) {
            fl |= d.flags[dsrc] & ACC_RCMD_HAS_DEPS;
            dc = d.dep;
            db = d.dep.off[dsrc];
        }
        const uint64_t d0 = doff ? doff[x] : 0ull, d1 = doff ? doff[x + 1] : 0ull;
        o.dep_off[x] = (uint32_t)d0;
        if (x == n2 - 1) o.dep_off[n2] = (uint32_t)d1;
        for (uint64_t k = d0; k < d1; ++k) {
            const uint64_t a = db + (k - d0);
            o.dm[k] = dc.m[a]; o.dl[k] = dc.l[a]; o.dn[k] = dc.n[a];
            o.ds[k] = dc.s[a]; o.de[k] = dc.e[a]; o.dk[k] = dc.k[a];
        }
        o.flags[x] = fl;
        const uint64_t a0 = off[x], a1 = off[x + 1];
        o.rng_off[x] = (uint32_t)a0;
        if (x == n2 - 1) o.rng_off[n2] = (uint32_t)a1;
        tinfo[x] = make_uint4(0u, x, 0u, 1u);
        for (uint64_t k = a0; k < a1; ++k) {
            const uint64_t sv = ps[k - a0], ev = pe[k - a0];
            o.rs[k] = sv; o.re[k] = ev;
            rowner[k] = x;
            eflag[k] = fl & ACC_RCMD_ERASED ? 0u : 1u;
            ms |= sv; me |= ev;
        }
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) { ms |= shfl_xor(ms, dd); me |= shfl_xor(me, dd); }
    if (lane_id() == 0) {
        if (ms) atomicOr((unsigned long long *)&g[2], (unsigned long long)ms);
        if (me) atomicOr((unsigned long long *)&g[3], (unsigned long long)me);
    }
}

// ---------------------------------------------------------------- RedundantBefore: the prune

// the input of one acc_rcmd_redundant_before on the device, with lim[j] = #stored TxnIds < bound[j]
struct Bounds {
    uint32_t m;
    const uint64_t *rs, *re;
    const uint32_t *lim;
};

// g[0] = max lim
__global__ __launch_bounds__(BLOCK) void k_rp_lim(uint32_t m, const uint64_t *__restrict__ bm, const uint64_t *__restrict__ bl,
                                                  const int32_t *__restrict__ bn, Table s, uint32_t *__restrict__ lim,
                                                  uint64_t *__restrict__ g)
{
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t lo = 0;
    if (j < m) {
        lo = lower_bound_ts(s.tm, s.tl, s.tn, 0, s.n, ts_at(bm, bl, bn, j));
        lim[j] = lo;
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) lo = max(lo, shfl_xor(lo, dd));
    if (lane_id() == 0 && lo) atomicMax((unsigned long long *)&g[0], (unsigned long long)lo);
}

__global__ __launch_bounds__(BLOCK) void k_rp_rowner(uint32_t n, const uint32_t *__restrict__ rng_off, uint32_t *__restrict__ rowner)
{
    const uint32_t x = blockIdx.x * BLOCK + threadIdx.x;
    if (x >= n) return;
    for (uint32_t k = rng_off[x]; k < rng_off[x + 1]; ++k) rowner[k] = x;
}

// the first input range that ends above a (the input is sorted and disjoint: its ends ascend)
__device__ __forceinline__ uint32_t first_above(const uint64_t *__restrict__ re, uint32_t m, uint64_t a)
{
    return upper_bound(re, 0, m, a);
}

// What the prune's second pass writes per kept row and per new range.
struct Pruned {
    const uint64_t *poff;    // [R + 1] exclusive scan of the piece counts
    const uint64_t *kidx;    // [n + 1] exclusive scan of keep: the new row
    const uint64_t *roff;    // [n + 1] exclusive scan of the kept rows' range counts
    uint64_t *rs, *re;       // the new table's ranges
    uint32_t *rowner, *eflag;
};

// Stored range k = (a, b) of row r minus the input ranges j with r < lim[j] (AbstractRanges.subtract: its maximal pieces
// outside them, in order, none empty). Rows at or above max lim keep their ranges as they are. WRITE == false: cnt[k] =
// the pieces, chg[r] = 1 where they are not (a, b) itself. WRITE: the pieces at roff[r] + (poff[k] - poff[first range
// of r]), with the new row as owner, and the OR of the starts and ends (g[2], g[3]).
template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_rp_cut(uint32_t R, Table s, const uint32_t *__restrict__ rowner, Bounds in,
                                                  uint64_t *__restrict__ cnt, uint32_t *__restrict__ chg, Pruned o,
                                                  uint64_t *__restrict__ g)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    uint64_t ms = 0, me = 0;
    if (k < R) {
        const uint32_t r = rowner[k];
        const uint32_t maxlim = (uint32_t)g[0];
        const uint64_t a = s.rs[k], b = s.re[k];
        uint64_t dst = 0;
        uint32_t x = 0;
        if constexpr (WRITE) {
            x = (uint32_t)o.kidx[r];
            dst = o.roff[r] + (o.poff[k] - o.poff[s.rng_off[r]]);
        }
        uint32_t pieces = 0;
        bool same = true;
        auto piece = [&](uint64_t ps, uint64_t pe) {
            if constexpr (WRITE) {
                o.rs[dst] = ps; o.re[dst] = pe;
                o.rowner[dst] = x; o.eflag[dst] = 1u;
                ms |= ps; me |= pe;
                ++dst;
            }
            ++pieces;
        };
        if (r >= maxlim) piece(a, b);
        else {
            uint64_t cur = a;
            bool open = true;   // cur < b: something of the range is still uncovered
            for (uint32_t j = first_above(in.re, in.m, a); j < in.m && in.rs[j] < b; ++j) {
                if (r >= in.lim[j]) continue;
                if (cur < in.rs[j]) piece(cur, in.rs[j]);
                same = false;
                if (in.re[j] >= b) { open = false; break; }
                cur = in.re[j];
            }
            if (open) piece(cur, b);
        }
        if constexpr (!WRITE) {
            cnt[k] = pieces;
            if (!same) chg[r] = 1u;
        }
    }
    if constexpr (WRITE) {
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) { ms |= shfl_xor(ms, dd); me |= shfl_xor(me, dd); }
        // the masks only gain bits: a wave whose bits are all in already (nearly every wave after the first few) adds
        // nothing, and thousands of read-modify-writes of one word would serialise
        if (lane_id() == 0) {
            if (ms & ~__hip_atomic_load(&g[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicOr((unsigned long long *)&g[2], (unsigned long long)ms);
            if (me & ~__hip_atomic_load(&g[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicOr((unsigned long long *)&g[3], (unsigned long long)me);
        }
    }
}

// row r: keep = erased || r >= max lim || it has ranges left; the counts of the kept rows; cutf = kept with changed ranges
__global__ __launch_bounds__(BLOCK) void k_rp_rows(Table s, const uint64_t *__restrict__ poff, const uint32_t *__restrict__ chg,
                                                   uint64_t *__restrict__ keep, uint64_t *__restrict__ kcnt,
                                                   uint64_t *__restrict__ kdep, uint64_t *__restrict__ cutf,
                                                   const uint64_t *__restrict__ g)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= s.n) return;
    const uint32_t maxlim = (uint32_t)g[0];
    const uint64_t c = poff[s.rng_off[r + 1]] - poff[s.rng_off[r]];
    const bool k = (s.flags[r] & ACC_RCMD_ERASED) || r >= maxlim || c > 0;
    keep[r] = k ? 1u : 0u;
    kcnt[r] = k ? c : 0u;
    kdep[r] = k ? s.dep.off[r + 1] - s.dep.off[r] : 0u;
    cutf[r] = k && chg[r] ? 1u : 0u;
}

// every row column of the kept rows at their new row, the new offsets (their ends by the thread of the last old row: the
// new table may be empty), the index's per-row input, and each kept row's deps as a segment of the segmented copy
__global__ __launch_bounds__(BLOCK) void k_rp_write(Table s, const uint64_t *__restrict__ keep, const uint64_t *__restrict__ kidx,
                                                    const uint64_t *__restrict__ roff, const uint64_t *__restrict__ doff,
                                                    TableOut o, uint4 *__restrict__ tinfo, uint32_t *__restrict__ dsrc)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= s.n) return;
    if (r == s.n - 1) {
        const uint64_t n2 = kidx[s.n];
        o.rng_off[n2] = (uint32_t)roff[s.n];
        o.dep_off[n2] = (uint32_t)doff[s.n];
    }
    if (!keep[r]) return;
    const uint64_t x = kidx[r];
    o.tm[x] = s.tm[r]; o.tl[x] = s.tl[r]; o.tn[x] = s.tn[r];
    o.flags[x] = s.flags[r];
    o.em[x] = s.em[r]; o.el[x] = s.el[r]; o.en[x] = s.en[r];
    o.status[x] = s.status[r];
    o.rng_off[x] = (uint32_t)roff[r];
    o.dep_off[x] = (uint32_t)doff[r];
    dsrc[x] = s.dep.off[r];
    tinfo[x] = make_uint4(0u, (uint32_t)x, 0u, 1u);
}

// ---------------------------------------------------------------- RedundantBefore: registration under the map

// the owner update of every range of the delta (offsets validated)
__global__ __launch_bounds__(BLOCK) void k_rt_owner(uint32_t D, const uint32_t *__restrict__ rng_off, uint32_t *__restrict__ uown)
{
    const uint32_t u = blockIdx.x * BLOCK + threadIdx.x;
    if (u >= D) return;
    for (uint32_t k = rng_off[u]; k < rng_off[u + 1]; ++k) uown[k] = u;
}

// Range k = (a, b) of non-erasing update u of a range-domain TxnId t minus the map's intervals whose bound is above t
// (RedundantBefore.removeShardRedundant); the ranges of erasing updates and of key-domain TxnIds, which nothing reads,
// stay. A closed interval [st, en] of key codes is (st - 1, en] (EndInclusive) or [st, en + 1) in the store's bound
// type. WRITE == false: cnt[k] = the pieces, *ntrim counts the ranges that do not stay as they are.
template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_rt_trim(Delta d, const uint32_t *__restrict__ uown, mc::Map mp, uint64_t *__restrict__ cnt,
                                                   const uint64_t *__restrict__ toff, uint64_t *__restrict__ ors,
                                                   uint64_t *__restrict__ ore, uint64_t *__restrict__ ntrim)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    bool changed = false;
    if (k < d.NR) {
        const uint32_t u = uown[k];
        const uint64_t a = d.rs[k], b = d.re[k];
        const uint64_t tm = d.tm[u], tl = d.tl[u];
        const int32_t tn = d.tn[u];
        uint64_t dst = 0;
        if constexpr (WRITE) dst = toff[k];
        uint32_t pieces = 0;
        auto piece = [&](uint64_t ps, uint64_t pe) {
            if constexpr (WRITE) { ors[dst] = ps; ore[dst] = pe; ++dst; }
            ++pieces;
        };
        if (!(tl & 1u) || (d.flags[u] & ACC_RCMD_ERASED)) piece(a, b);
        else {
            uint64_t cur = a;
            bool open = true;
            // the first interval whose end lies above a: en > a (EndInclusive), en + 1 > a
            uint64_t i = mp.ei ? lower_bound(mp.en, 0, mp.nv, a + 1) : lower_bound(mp.en, 0, mp.nv, a);
            for (; i < mp.nv; ++i) {
                const uint64_t st = mp.st[i], en = mp.en[i];
                const uint64_t is = mp.ei ? st - 1 : st;
                const uint64_t ie = mp.ei ? en : (en == ~0ull ? en : en + 1);
                if (is >= b) break;
                if (ts_cmp(mp.vm[i], mp.vl[i], mp.vn[i], tm, tl, tn) <= 0) continue;
                if (cur < is) piece(cur, is);
                changed = true;
                if (ie >= b) { open = false; break; }
                cur = ie;
            }
            if (open) piece(cur, b);
        }
        if constexpr (!WRITE) cnt[k] = pieces;
    }
    if constexpr (!WRITE) {
        const unsigned long long bc = __ballot(changed);
        if (bc && lane_id() == 0) atomicAdd((unsigned long long *)ntrim, (unsigned long long)__popcll(bc));
    }
}

// the trimmed delta's rng_off
__global__ __launch_bounds__(BLOCK) void k_rt_off(uint32_t D, const uint32_t *__restrict__ rng_off, const uint64_t *__restrict__ toff,
                                                  uint32_t *__restrict__ out)
{
    const uint32_t u = blockIdx.x * BLOCK + threadIdx.x;
    if (u > D) return;
    out[u] = (uint32_t)toff[rng_off[u]];
}

// ---------------------------------------------------------------- query

// Per query: the checks of acc_cfk_keydeps_mixed (Kind.ofOrdinal, Kind.witnesses(), both offset arrays, the domain of
// its participants, Keys sorted unique, Ranges sorted and deoverlapped with start < end); then, inside offsets that
// passed, its row {lim, tpos, witnesses, domain}: lim = stored TxnIds below S = executeAt (STARTED_BEFORE, :901-902),
// tpos = the table index of a stored TxnId Timestamp.equals to its own (never a dep of itself) or NONE; the owner of
// each of its keys and ranges; the OR-mask of the query low bounds against the first one (g[1]).
// RECOVERY (acc_rcmd_map_reduce_full; X = the query's testTxnId, no executeAt): the mask is test_kinds, or for -1
// X.kind().witnessedBy() with k_rr_query's errors; lower = #stored TxnIds < X and upper = #stored TxnIds <= X give
// lim = lower (STARTED_BEFORE), n (ANY), or n - upper over the mirrored positions (STARTED_AFTER); tpos = NONE: a command
// Timestamp.equals to X is visited like any other (:895-906).
template <bool RECOVERY>
__global__ __launch_bounds__(BLOCK) void k_rc_qprep(Queries Q, Table s, int test_kinds, uint32_t started_at, uint4 *__restrict__ tinfo,
                                                    uint32_t *__restrict__ owner, uint32_t *__restrict__ rowner, uint64_t *__restrict__ g)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    uint64_t ml = 0;
    if (q < Q.nq) {
        uint64_t e = 0;
        const uint64_t l = Q.tl[q];
        const uint32_t kind = (uint32_t)(l >> 1) & 7u;
        uint32_t mask = 0;
        if constexpr (RECOVERY) {
            int m = test_kinds;
            if (m < 0) {
                m = witnessed_by(kind);
                if (m < 0) e |= kind == ACC_KIND_LOCAL_ONLY ? E_Q_KIND_STATE : E_Q_KIND_ARG;
            }
            mask = m < 0 ? 0u : (uint32_t)m;
        } else {
            if (kind > ACC_KIND_LOCAL_ONLY) e |= E_Q_KIND_ARG;          // Kind.ofOrdinal
            else if (witnesses(kind) == 0) e |= E_Q_KIND_STATE;         // Kind.witnesses(): LocalOnly throws
            mask = witnesses(kind);
        }
        const bool range = l & 1u;
        const uint64_t ref = Q.P ? Q.key[0] : Q.R ? Q.rs[0] : 0ull;
        const uint32_t k0 = Q.key_off[q], k1 = Q.key_off[q + 1];
        if (k1 < k0 || k1 > Q.P || (q == 0 && k0 != 0) || (q == Q.nq - 1 && k1 != Q.P)) e |= E_Q_KOFF;
        else if (range) { if (k1 != k0) e |= E_Q_RKEYS; }
        else
            for (uint32_t j = k0; j < k1; ++j) {
                if (j > k0 && Q.key[j - 1] >= Q.key[j]) e |= E_Q_KEYS;
                owner[j] = q;
                ml |= Q.key[j] ^ ref;
            }
        const uint32_t r0 = Q.rng_off[q], r1 = Q.rng_off[q + 1];
        if (r1 < r0 || r1 > Q.R || (q == 0 && r0 != 0) || (q == Q.nq - 1 && r1 != Q.R)) e |= E_Q_ROFF;
        else if (!range) { if (r1 != r0) e |= E_Q_KRANGES; }
        else
            for (uint32_t j = r0; j < r1; ++j) {
                if (Q.rs[j] >= Q.re[j]) e |= E_BOUND;
                if (j > r0 && Q.re[j - 1] > Q.rs[j]) e |= E_ORDER;     // touching ranges are allowed
                rowner[j] = q;
                ml |= Q.rs[j] ^ ref;
            }
        if (e) atomicOr((unsigned long long *)&g[0], (unsigned long long)e);
        if constexpr (RECOVERY) {
            const Ts x{ Q.tm[q], l, Q.tn[q] };
            const uint32_t lower = lower_bound_ts(s.tm, s.tl, s.tn, 0, s.n, x);
            const uint32_t upper = upper_bound_ts(s.tm, s.tl, s.tn, lower, s.n, x);
            const uint32_t lim = started_at == ACC_STARTED_BEFORE ? lower : started_at == ACC_STARTED_AFTER ? s.n - upper : s.n;
            tinfo[q] = make_uint4(lim, NONE, mask, range ? 1u : 0u);
        } else {
            // lim: first stored TxnId >= S; tpos: first stored TxnId >= the query's own, when equal
            const uint32_t lim = lower_bound_ts(s.tm, s.tl, s.tn, 0, s.n, ts_at(Q.xm, Q.xl, Q.xn, q));
            const Ts id{ Q.tm[q], l, Q.tn[q] };
            const uint32_t lo = lower_bound_ts(s.tm, s.tl, s.tn, 0, s.n, id);
            const uint32_t tpos = lo < s.n && cmp(ts_at(s.tm, s.tl, s.tn, lo), id) == 0 ? lo : NONE;
            tinfo[q] = make_uint4(lim, tpos, mask, range ? 1u : 0u);
        }
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) ml |= shfl_xor(ml, dd);
    if (lane_id() == 0 && ml) atomicOr((unsigned long long *)&g[1], (unsigned long long)ml);
}

// ---------------------------------------------------------------- recovery scans

// the store's columns as recovery_pred.hpp names them
struct StateCols {
    const uint64_t *tm, *tl, *em, *el;
    const int32_t *tn, *en;
    const uint8_t *status, *flags;
    const uint32_t *roff;
    const uint64_t *rs, *re;
    const uint32_t *doff;
    const uint64_t *dm, *dl;
    const int32_t *dn;
    const uint64_t *ds, *de;
    const uint8_t *dk;
    uint32_t end_incl;
};

// STARTED_AFTER stabs positions counted from the top of the table
__global__ __launch_bounds__(BLOCK) void k_rcr_mirror(uint32_t NE, uint32_t n, const uint2 *__restrict__ info, uint2 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= NE) return;
    const uint2 v = info[i];
    out[i] = make_uint2(v.x, n - 1u - v.y);
}

// One wave per participant (key or range of a query) over the raw entries the stabbing pass left in its span of ent:
// 64 entries at a time, a lane per entry tests its command (rr_command_passes: flags and status byte, executeAt against
// X, and for what is left under WITH / WITHOUT the search of X in the command's deps); survivors are compacted in entry
// order to the front of the same span (writes never pass the chunk being read) with their table positions un-mirrored,
// and the participant's count is rewritten; its first entry stays. st: [0] entries kept, [1] deps searches.
__global__ __launch_bounds__(BLOCK) void k_rcr_filter(uint64_t first, uint64_t nparts, uint32_t P, const uint32_t *__restrict__ owner,
                                                      const uint32_t *__restrict__ rowner, StateCols c, const uint64_t *__restrict__ qm,
                                                      const uint64_t *__restrict__ ql, const int32_t *__restrict__ qn,
                                                      const uint4 *__restrict__ tinfo, RcParams prm, uint32_t mirror_n,
                                                      ulonglong2 *__restrict__ q_out, uint64_t *__restrict__ ent,
                                                      uint64_t *__restrict__ st)
{
    const uint64_t w = first + (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= nparts) return;
    const uint32_t q = w < P ? owner[w] : rowner[w - P];
    const uint64_t xm = qm[q], xl = ql[q];
    const int32_t xn = qn[q];
    const uint32_t mask = tinfo[q].z;
    const ulonglong2 span = q_out[w];
    const uint64_t lt = (1ull << lane_id()) - 1;
    uint64_t kept = 0;
    uint32_t probes = 0;
    for (uint64_t base = 0; base < span.y; base += 64) {
        const uint64_t k = base + lane_id();
        bool pass = false, probed = false;
        uint64_t x = 0;
        if (k < span.y) {
            x = ent[span.x + k];
            uint32_t pos = (uint32_t)x;
            if (mirror_n) pos = mirror_n - 1u - pos;
            x = (x & 0xFFFFFFFF00000000ull) | pos;
            pass = rr_command_passes(c, prm, pos, mask, xm, xl, xn, &probed);
        }
        const uint64_t bal = __ballot(pass);
        probes += (uint32_t)__popcll(__ballot(probed));
        if (pass) ent[span.x + kept + (uint64_t)__popcll(bal & lt)] = x;
        kept += (uint64_t)__popcll(bal);
    }
    if (lane_id() == 0) {
        q_out[w] = make_ulonglong2(span.x, kept);
        if (kept) atomicAdd((unsigned long long *)&st[0], (unsigned long long)kept);
        if (probes) atomicAdd((unsigned long long *)&st[1], (unsigned long long)probes);
    }
}

}  // namespace rc

using namespace rc;

acc_rcmd *rcmd_new(int device, uint32_t end_inclusive)
{
    if (end_inclusive > 1) fail(ACC_E_ARG, "end_inclusive must be 0 (StartInclusive) or 1 (EndInclusive)");
    acc_rcmd *s = new acc_rcmd();
    s->device = device;
    s->end_inclusive = end_inclusive;
    return s;
}

void rcmd_free(acc_rcmd *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (void *p : { (void *)s->tm, (void *)s->tl, (void *)s->tn, (void *)s->flags, (void *)s->rng_off, (void *)s->rs, (void *)s->re,
                     (void *)s->dict_s, (void *)s->dict_e, (void *)s->dincl, (void *)s->cs_s, (void *)s->cs_e, (void *)s->cs_info,
                     (void *)s->cs_kind, (void *)s->cls, (void *)s->em, (void *)s->el, (void *)s->en, (void *)s->status,
                     (void *)s->dep_off, (void *)s->dm, (void *)s->dl, (void *)s->dn, (void *)s->ds, (void *)s->de, (void *)s->dk })
        (void)hipFree(p);
    mc_free(s->rb);
    rcmd_union_free(s);
    delete s;
}

static Table table_of(const acc_rcmd *s)
{
    return Table{ s->tm, s->tl, s->tn, s->flags, s->rng_off, s->rs, s->re, s->n, s->em, s->el, s->en, s->status,
                  DepCols{ s->dep_off, s->dm, s->dl, s->dn, s->ds, s->de, s->dk } };
}

void rcmd_table(acc_ctx *ctx, acc_rcmd *s, acc_rcmd_table *out)
{
    if (!s || !out) fail(ACC_E_ARG, "null argument");
    // an empty store has no arrays yet: placeholders (rng_off = one zero)
    uint32_t *z = nullptr;
    if (!s->rng_off) {
        z = ctx->get<uint32_t>("rc_zero", 4);
        ACC_HIP(hipMemsetAsync(z, 0, 16, ctx->stream));
        ctx->sync();
    }
    *out = acc_rcmd_table{ s->n, s->end_inclusive, s->R, s->n_dict, 0u, acc_ts_cols{ s->tm, s->tl, s->tn }, s->flags,
                           s->rng_off ? s->rng_off : z, s->rs, s->re, s->dict_s, s->dict_e };
}

void rcmd_state(acc_ctx *ctx, acc_rcmd *s, acc_rcmd_state *out)
{
    if (!s || !out) fail(ACC_E_ARG, "null argument");
    uint32_t *z = nullptr;
    if (!s->dep_off) {   // an empty store: dep_off = one zero
        z = ctx->get<uint32_t>("rc_zero", 4);
        ACC_HIP(hipMemsetAsync(z, 0, 16, ctx->stream));
        ctx->sync();
    }
    *out = acc_rcmd_state{ s->n, 0u, s->ND, acc_ts_cols{ s->em, s->el, s->en }, s->status, s->flags, s->dep_off ? s->dep_off : z,
                           acc_ts_cols{ s->dm, s->dl, s->dn }, s->ds, s->de, s->dk };
}

// The end of every call that rewrites the table (an update, a prune). o: the new table, n2 rows, R2 ranges, ND2 deps, in
// the context's rc_t_* buffers; b: the index's inputs over it (tinfo, rowner, eflag, eidx allocated); g[2], g[3]: the OR
// masks of the range starts and ends, g[4], g[5]: two words of the caller's, read back with them (w). The index is
// rebuilt from the new table by rd_range_dict as acc_rangedeps_batch runs it, and its arrays and the table move into
// the store with acc_ctx::swap_buf (the context keeps the store's previous arrays for its next results).
struct Finished {
    uint64_t w[2];
    uint32_t NE, n_dict;
};
static Finished finish_table(acc_ctx *ctx, acc_rcmd *store, const TableOut &o, RdBuild &b, uint32_t n2, uint64_t R2, uint64_t ND2,
                             const uint64_t *g)
{
    Finished fin{};
    b.tl = o.tl;
    b.rs = o.rs;
    b.re = o.re;
    scan<uint32_t, OpAdd<uint32_t>>(ctx, b.eflag, b.eidx, (size_t)R2, true, b.eidx + R2);
    {
        ReadBack rb(ctx);
        const auto hm = rb.words((const uint64_t *)(g + 2), 4);   // start mask, end mask, the caller's two words
        ReadBack::Word<uint32_t> ne;
        if (R2) ne = rb.u32(b.eidx + R2);
        rb.wait();
        b.mask_s = hm[0]; b.mask_e = hm[1];
        fin.w[0] = hm[2]; fin.w[1] = hm[3];
        b.NE = ne;
    }
    rd_range_dict(ctx, b);
    uint32_t n_dict = 0;
    {
        ReadBack rb(ctx);
        ReadBack::Word<uint32_t> nd;
        if (b.NE) nd = rb.u32(b.dincl + b.NE);
        rb.wait();   // everything of this call is complete: the store may take the arrays
        n_dict = nd;
    }

    // ---- the store adopts the table and the index; the context keeps its previous arrays for the next results
    int bi = 0;
    auto adopt = [&](const char *name, auto *&p) {
        void *v = p;
        ctx->swap_buf(name, v, store->bytes[bi++]);
        p = static_cast<std::remove_reference_t<decltype(p)>>(v);
    };
    adopt("rc_t_tm", store->tm); adopt("rc_t_tl", store->tl); adopt("rc_t_tn", store->tn); adopt("rc_t_flags", store->flags);
    adopt("rc_t_rng_off", store->rng_off); adopt("rc_t_rs", store->rs); adopt("rc_t_re", store->re);
    adopt("rd_dict_s", store->dict_s); adopt("rd_dict_e", store->dict_e); adopt("rd_dincl", store->dincl);
    adopt("rd_cs_s", store->cs_s); adopt("rd_cs_e", store->cs_e); adopt("rd_cs_info", store->cs_info);
    adopt("rd_cs_kind", store->cs_kind); adopt("rd_cls", store->cls);
    adopt("rc_t_em", store->em); adopt("rc_t_el", store->el); adopt("rc_t_en", store->en); adopt("rc_t_status", store->status);
    adopt("rc_t_doff", store->dep_off); adopt("rc_t_dm", store->dm); adopt("rc_t_dl", store->dl); adopt("rc_t_dn", store->dn);
    adopt("rc_t_ds", store->ds); adopt("rc_t_de", store->de); adopt("rc_t_dk", store->dk);
    store->ND = ND2;
    store->n = n2;
    store->R = (uint32_t)R2;
    store->NE = b.NE;
    store->n_dict = n_dict;
    ctx->rd_valid = false;   // an earlier result may name arrays the store or the next call now owns
    store->u.valid = false;  // acc_rcmd_partial_rangedeps rebuilds its union index from the new table
    fin.NE = b.NE;
    fin.n_dict = n_dict;
    return fin;
}

// the new table's arrays (the context's rc_t_* buffers) and the index's inputs over it
static TableOut table_out(acc_ctx *ctx, uint32_t n2, uint64_t R2, uint64_t ND2)
{
    return TableOut{ ctx->get<uint64_t>("rc_t_tm", n2), ctx->get<uint64_t>("rc_t_tl", n2), ctx->get<int32_t>("rc_t_tn", n2),
                     ctx->get<uint8_t>("rc_t_flags", n2), ctx->get<uint32_t>("rc_t_rng_off", (size_t)n2 + 1),
                     ctx->get<uint64_t>("rc_t_rs", R2), ctx->get<uint64_t>("rc_t_re", R2),
                     ctx->get<uint64_t>("rc_t_em", n2), ctx->get<uint64_t>("rc_t_el", n2), ctx->get<int32_t>("rc_t_en", n2),
                     ctx->get<uint8_t>("rc_t_status", n2), ctx->get<uint32_t>("rc_t_doff", (size_t)n2 + 1),
                     ctx->get<uint64_t>("rc_t_dm", ND2), ctx->get<uint64_t>("rc_t_dl", ND2), ctx->get<int32_t>("rc_t_dn", ND2),
                     ctx->get<uint64_t>("rc_t_ds", ND2), ctx->get<uint64_t>("rc_t_de", ND2), ctx->get<uint8_t>("rc_t_dk", ND2) };
}
static RdBuild index_inputs(acc_ctx *ctx, const acc_rcmd *store, uint32_t n2, uint64_t R2)
{
    RdBuild b;
    b.n = n2;
    b.R = (size_t)R2;
    b.end_inclusive = (int)store->end_inclusive;
    b.tinfo = ctx->get<uint4>("rd_tinfo", n2);
    b.rowner = ctx->get<uint32_t>("rd_rowner", R2);
    b.eflag = ctx->get<uint32_t>("rd_eflag", R2);
    b.eidx = ctx->get<uint32_t>("rd_eidx", R2 + 1);
    return b;
}

// Registration under a non-empty map (InMemorySafeStore.update :757-760): the ranges of every non-erasing update of a
// range-domain TxnId t lose what the map's intervals with a bound above t cover. d's range columns are replaced by the
// trimmed ones (a range may split: NR may grow); returns the ranges changed or removed. The offsets have passed
// validation.
static uint64_t trim_delta(acc_ctx *ctx, const acc_maxconflicts *rbm, Delta &d)
{
    if (d.NR == 0) return 0;
    const mc::Map mp = mc_map(rbm);
    uint32_t *uown = ctx->get<uint32_t>("rt_uown", d.NR);
    uint64_t *cnt = ctx->get<uint64_t>("rt_cnt", d.NR), *toff = ctx->get<uint64_t>("rt_toff", (size_t)d.NR + 1);
    uint64_t *ntrim = ctx->get<uint64_t>("rt_ntrim", 1);
    ACC_HIP(hipMemsetAsync(ntrim, 0, 8, ctx->stream));
    launch(ctx, "rt_owner", k_rt_owner, dim3(grid_for(d.D, BLOCK)), dim3(BLOCK), 0, d.D, d.rng_off, uown);
    launch(ctx, "rt_count", k_rt_trim<false>, dim3(grid_for(d.NR, BLOCK)), dim3(BLOCK), 0, d, (const uint32_t *)uown, mp, cnt,
           (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, ntrim);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, cnt, toff, d.NR, true, toff + d.NR);
    uint64_t nt, NR2;
    {
        ReadBack rb(ctx);
        const auto a = rb.u64(ntrim);
        const auto b = rb.u64(toff + d.NR);
        rb.wait();
        nt = a; NR2 = b;
    }
    if (nt == 0) return 0;   // nothing under any bound above its TxnId: the delta as it is
    if (NR2 >= 0xFFFFFFFFull) fail(ACC_E_CAP, "trimmed updates too large (ranges >= 2^32 - 1)");
    uint32_t *noff = ctx->get<uint32_t>("rt_roff", (size_t)d.D + 1);
    uint64_t *ors = ctx->get<uint64_t>("rt_rs", NR2), *ore = ctx->get<uint64_t>("rt_re", NR2);
    launch(ctx, "rt_off", k_rt_off, dim3(grid_for((size_t)d.D + 1, BLOCK)), dim3(BLOCK), 0, d.D, d.rng_off, (const uint64_t *)toff, noff);
    launch(ctx, "rt_write", k_rt_trim<true>, dim3(grid_for(d.NR, BLOCK)), dim3(BLOCK), 0, d, (const uint32_t *)uown, mp,
           (uint64_t *)nullptr, (const uint64_t *)toff, ors, ore, (uint64_t *)nullptr);
    d.rng_off = noff;
    d.rs = ors;
    d.re = ore;
    d.NR = (uint32_t)NR2;
    return nt;
}

// acc_rcmd_update (state == false: in's state columns are not read) and acc_rcmd_update_cmds
static void rcmd_update_impl(acc_ctx *ctx, acc_rcmd *store, const acc_rcmd_cmd_updates *in, bool state)
{
    if (in->mem != ACC_MEM_HOST && in->mem != ACC_MEM_DEVICE) fail(ACC_E_ARG, "mem must be ACC_MEM_HOST or ACC_MEM_DEVICE");
    if (in->n_ranges >= 0xFFFFFFFFull) fail(ACC_E_ARG, "n_ranges must be < 2^32 - 1");
    if (state && in->n_deps >= 0xFFFFFFFFull) fail(ACC_E_ARG, "n_deps must be < 2^32 - 1");
    hipStream_t st = ctx->stream;
    const uint32_t D = in->n_upd, NR = (uint32_t)in->n_ranges, mem = in->mem;
    const uint32_t NDin = state ? (uint32_t)in->n_deps : 0u;
    ctx->stat("rcmd.inserted", 0);
    ctx->stat("rcmd.updated", 0);
    ctx->stat("rcmd.skipped_key_domain", 0);
    ctx->stat("rcmd.erased_ignored", 0);
    ctx->stat("rcmd.entries", store->NE);
    ctx->stat("rcmd.stored_ranges", store->n_dict);
    ctx->stat("rcmd.update_ranges_trimmed", 0);
    if (D == 0) {
        if (NR) fail(ACC_E_ARG, "rng_off must start at 0, be non-decreasing and end at n_ranges");
        if (NDin) fail(ACC_E_ARG, "dep_off must start at 0, be non-decreasing and end at n_deps");
        return;
    }
    Delta d{};
    d.D = D; d.NR = NR;
    d.state = state ? 1u : 0u; d.ND = NDin;
    d.tm = stage_in(ctx, "rc_in_tm", in->txn_id.msb, D, mem);
    d.tl = stage_in(ctx, "rc_in_tl", in->txn_id.lsb, D, mem);
    d.tn = stage_in(ctx, "rc_in_tn", in->txn_id.node, D, mem);
    d.flags = stage_in(ctx, "rc_in_flags", in->flags, D, mem);
    d.rng_off = stage_in(ctx, "rc_in_roff", in->rng_off, (size_t)D + 1, mem);
    d.rs = stage_in(ctx, "rc_in_rs", in->rng_start, NR, mem);
    d.re = stage_in(ctx, "rc_in_re", in->rng_end, NR, mem);
    if (state) {
        if (in->execute_at.msb) {
            d.xm = stage_in(ctx, "rc_in_xm", in->execute_at.msb, D, mem);
            d.xl = stage_in(ctx, "rc_in_xl", in->execute_at.lsb, D, mem);
            d.xn = stage_in(ctx, "rc_in_xn", in->execute_at.node, D, mem);
        } else {
            d.xm = d.tm; d.xl = d.tl; d.xn = d.tn;
        }
        d.status = stage_in(ctx, "rc_in_status", in->status, D, mem);
        d.dep = DepCols{ stage_in(ctx, "rc_in_doff", in->dep_off, (size_t)D + 1, mem),
                         stage_in(ctx, "rc_in_dm", in->dep_txn.msb, NDin, mem), stage_in(ctx, "rc_in_dl", in->dep_txn.lsb, NDin, mem),
                         stage_in(ctx, "rc_in_dn", in->dep_txn.node, NDin, mem), stage_in(ctx, "rc_in_ds", in->dep_start, NDin, mem),
                         stage_in(ctx, "rc_in_de", in->dep_end, NDin, mem), stage_in(ctx, "rc_in_dk", in->dep_is_key, NDin, mem) };
    }
    const uint8_t allowed = state ? (uint8_t)(ACC_RCMD_ERASED | ACC_RCMD_HAS_DEPS | ACC_RCMD_KEEP_DEPS) : (uint8_t)ACC_RCMD_ERASED;

    // ---- 1, 2. validate; the TxnIds' dense ranks and stable sorted order
    uint64_t *g = ctx->get<uint64_t>("rc_g", 8);
    ACC_HIP(hipMemsetAsync(g, 0, 8 * sizeof(uint64_t), st));
    uint64_t *w[3] = { ctx->get<uint64_t>("rc_w0", D), ctx->get<uint64_t>("rc_w1", D), ctx->get<uint64_t>("rc_w2", D) };
    launch(ctx, "rc_validate", k_rc_validate, dim3(grid_for(D, BLOCK)), dim3(BLOCK), 0, d, allowed, g, w[0], w[1], w[2]);
    const uint64_t *words[3] = { w[0], w[1], w[2] };
    const DenseRank dr = dense_rank(ctx, "rc_dr", D, 3, words, nullptr, nullptr, true);
    uint32_t G, nkey;
    {
        ReadBack rb(ctx);
        const auto hg = rb.words((const uint64_t *)g, 2);
        const auto cnt = rb.u64(dr.count_dev);
        rb.wait();
        const uint64_t e = hg[0];
        if (e & E_KIND) fail(ACC_E_ARG, "Kind.ofOrdinal: invalid kind ordinal in TxnId flags");
        if (e & E_FLAGS)
            fail(ACC_E_ARG, state ? "flags: only ACC_RCMD_ERASED, ACC_RCMD_HAS_DEPS and ACC_RCMD_KEEP_DEPS may be set"
                                  : "flags: only ACC_RCMD_ERASED may be set");
        if (e & E_OFF) fail(ACC_E_ARG, "rng_off must start at 0, be non-decreasing and end at n_ranges");
        if (e & E_BOUND) fail(ACC_E_ARG, "range start must be below its end (Range: start >= end)");
        if (e & E_ORDER) fail(ACC_E_ARG, "ranges of an update must be sorted and deoverlapped (Ranges.ofSortedAndDeoverlapped)");
        if (e & E_STATUS) fail(ACC_E_ARG, "invalid Status ordinal");
        if (e & E_DOFF) fail(ACC_E_ARG, "dep_off must start at 0, be non-decreasing and end at n_deps");
        if (e & E_DEPS) fail(ACC_E_ARG, "deps of an update must be sorted by TxnId, dep_is_key 0 or 1, ranges with start < end");
        G = (uint32_t)(uint64_t)cnt;
        nkey = (uint32_t)hg[1];
    }

    // under a non-empty RedundantBefore map the fold sees the trimmed ranges (a store never marked launches nothing here)
    const uint64_t ntrim = store->rb && store->rb->nv ? trim_delta(ctx, store->rb, d) : 0;

    // ---- 3. groups against the stored TxnIds
    const Table s = table_of(store);
    const uint32_t n = store->n;
    uint32_t *gstart = ctx->get<uint32_t>("rc_gstart", (size_t)G + 1);
    uint32_t *pos = ctx->get<uint32_t>("rc_pos", G), *isnew = ctx->get<uint32_t>("rc_isnew", G);
    uint32_t *newx = ctx->get<uint32_t>("rc_newx", (size_t)G + 1);
    uint64_t *bound = ctx->get<uint64_t>("rc_bound", G), *boff = ctx->get<uint64_t>("rc_boff", (size_t)G + 1);
    launch(ctx, "rc_gstart", k_rc_gstart, dim3(grid_for(D, BLOCK)), dim3(BLOCK), 0, D, G, dr.perm, (const uint32_t *)dr.rank, gstart);
    launch(ctx, "rc_locate", k_rc_locate, dim3(grid_for(G, BLOCK)), dim3(BLOCK), 0, G, d, s, (const uint32_t *)dr.first, dr.perm,
           (const uint32_t *)gstart, pos, isnew, bound);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, isnew, newx, G, true, newx + G);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, bound, boff, G, true, boff + G);
    uint32_t nnew;
    uint64_t B;
    {
        ReadBack rb(ctx);
        const auto a = rb.u32(newx + G);
        const auto b = rb.u64(boff + G);
        rb.wait();
        nnew = a; B = b;
    }
    if ((uint64_t)n + nnew >= 0xFFFFFFFFull) fail(ACC_E_CAP, "range-command store too large (commands >= 2^32 - 1)");
    const uint32_t n2 = n + nnew;
    if (n2 == 0) {   // an empty store and key-domain TxnIds only
        ctx->stat("rcmd.skipped_key_domain", nkey);
        ctx->stat("rcmd.update_ranges_trimmed", ntrim);
        return;
    }

    // ---- 4. the fold
    uint64_t *scr_s = ctx->get<uint64_t>("rc_scr_s", 2 * B), *scr_e = ctx->get<uint64_t>("rc_scr_e", 2 * B);
    uint32_t *grow = ctx->get<uint32_t>("rc_grow", n2);
    ACC_HIP(hipMemsetAsync(grow, 0xFF, (size_t)n2 * sizeof(uint32_t), st));
    Folded f{ ctx->get<uint32_t>("rc_f_row", G), ctx->get<uint32_t>("rc_f_cnt", G), ctx->get<uint8_t>("rc_f_erased", G),
              ctx->get<const uint64_t *>("rc_f_ps", G), ctx->get<const uint64_t *>("rc_f_pe", G),
              ctx->get<uint32_t>("rc_f_ssrc", G), ctx->get<uint32_t>("rc_f_dsrc", G) };
    launch(ctx, "rc_fold", k_rc_fold, dim3(grid_for(G, BLOCK)), dim3(BLOCK), 0, G, d, s, dr.perm, (const uint32_t *)gstart,
           (const uint32_t *)pos, (const uint32_t *)isnew, (const uint32_t *)newx, (const uint64_t *)boff, scr_s, scr_e, grow, f, g + 4);

    // ---- 5. row counts -> rng_off; every column once
    uint32_t *insf = ctx->get<uint32_t>("rc_insf", n2), *insx = ctx->get<uint32_t>("rc_insx", (size_t)n2 + 1);
    uint64_t *cnt = ctx->get<uint64_t>("rc_cnt", n2), *off = ctx->get<uint64_t>("rc_off", (size_t)n2 + 1);
    launch(ctx, "rc_insflag", k_rc_insflag, dim3(grid_for(n2, BLOCK)), dim3(BLOCK), 0, n2, (const uint32_t *)grow,
           (const uint32_t *)isnew, insf);
    scan<uint32_t, OpAdd<uint32_t>>(ctx, insf, insx, n2, true, insx + n2);
    // deps are counted and scanned only when a command holds some, before or after (a store fed by acc_rcmd_update alone
    // runs the launches it always ran)
    const bool deps = state || store->ND > 0;
    uint64_t *dcnt = deps ? ctx->get<uint64_t>("rc_dcnt", n2) : nullptr;
    uint64_t *doff = deps ? ctx->get<uint64_t>("rc_doff", (size_t)n2 + 1) : nullptr;
    launch(ctx, "rc_counts", k_rc_counts, dim3(grid_for(n2, BLOCK)), dim3(BLOCK), 0, n2, d, s, (const uint32_t *)grow,
           (const uint32_t *)insx, (const uint32_t *)isnew, f, cnt, dcnt);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, cnt, off, n2, true, off + n2);
    if (deps) scan<uint64_t, OpAdd<uint64_t>>(ctx, dcnt, doff, n2, true, doff + n2);
    uint64_t R2, ND2 = 0;
    {
        ReadBack rb(ctx);
        const auto a = rb.u64(off + n2);
        ReadBack::Word<uint64_t> b;
        if (deps) b = rb.u64(doff + n2);
        rb.wait();
        R2 = a; ND2 = b;
    }
    if (R2 >= 0xFFFFFFFFull) fail(ACC_E_CAP, "range-command store too large (ranges >= 2^32 - 1)");
    if (ND2 >= 0xFFFFFFFFull) fail(ACC_E_CAP, "range-command store too large (deps >= 2^32 - 1)");
    const TableOut o = table_out(ctx, n2, R2, ND2);
    RdBuild b = index_inputs(ctx, store, n2, R2);
    launch(ctx, "rc_write", k_rc_write, dim3(grid_for(n2, BLOCK)), dim3(BLOCK), 0, n2, d, s, (const uint32_t *)dr.first,
           (const uint32_t *)grow, (const uint32_t *)insx, (const uint32_t *)isnew, f, (const uint64_t *)off, (const uint64_t *)doff, o, b.tinfo, b.rowner,
           b.eflag, g);

    // ---- 6. the index from the new table; the store adopts both
    const Finished fin = finish_table(ctx, store, o, b, n2, R2, ND2, g);
    const uint64_t n_ign = fin.w[0], n_upd = fin.w[1];
    ctx->stat("rcmd.inserted", nnew);
    ctx->stat("rcmd.updated", n_upd);
    ctx->stat("rcmd.skipped_key_domain", nkey);
    ctx->stat("rcmd.erased_ignored", n_ign);
    ctx->stat("rcmd.entries", fin.NE);
    ctx->stat("rcmd.stored_ranges", fin.n_dict);
    ctx->stat("rcmd.update_ranges_trimmed", ntrim);
}

void rcmd_update(acc_ctx *ctx, acc_rcmd *store, const acc_rcmd_updates *in)
{
    if (!store || !in) fail(ACC_E_ARG, "null argument");
    acc_rcmd_cmd_updates u{};
    u.n_upd = in->n_upd; u.mem = in->mem; u.n_ranges = in->n_ranges; u.txn_id = in->txn_id; u.flags = in->flags;
    u.rng_off = in->rng_off; u.rng_start = in->rng_start; u.rng_end = in->rng_end;
    rcmd_update_impl(ctx, store, &u, false);
}

void rcmd_update_cmds(acc_ctx *ctx, acc_rcmd *store, const acc_rcmd_cmd_updates *in)
{
    if (!store || !in) fail(ACC_E_ARG, "null argument");
    rcmd_update_impl(ctx, store, in, true);
}

// InMemoryCommandStore.markShardDurable (:346-370) for the resident table, once per distinct bound of the input: the
// map merged first (RedundantBefore.merge), then every non-erased command below a bound loses the input ranges that
// hold a bound above it, and leaves when none of its ranges is left.
void rcmd_redundant_before(acc_ctx *ctx, acc_rcmd *store, const acc_cfk_redundant_in *in)
{
    if (!store || !in) fail(ACC_E_ARG, "null argument");
    if (in->mem != ACC_MEM_HOST && in->mem != ACC_MEM_DEVICE) fail(ACC_E_ARG, "mem must be ACC_MEM_HOST or ACC_MEM_DEVICE");
    if (in->end_inclusive > 1) fail(ACC_E_ARG, "end_inclusive must be 0 (StartInclusive) or 1 (EndInclusive)");
    if (in->end_inclusive != store->end_inclusive) fail(ACC_E_ARG, "end_inclusive differs from the store's Range bound type");
    for (const char *z : { "rcmd.redundant_cmds_cut", "rcmd.redundant_cmds_dropped", "rcmd.redundant_prune_us", "rcmd.redundant_index_us" })
        ctx->stat(z, 0);
    ctx->stat("rcmd.redundant_ranges_before", store->R);
    ctx->stat("rcmd.redundant_ranges_after", store->R);
    if (in->n_ranges == 0) return;
    hipStream_t st = ctx->stream;
    const RbInput ri = rb_stage_ranges(ctx, in);
    if (!store->rb) store->rb = mc_new(store->device, store->end_inclusive);   // (the ranges have passed)
    rb_merge_staged(ctx, store->rb, ri);
    store->u.valid = false;   // the map may have changed: the partial call's union index names its intervals
    const uint32_t n = store->n, R = store->R, m = ri.n;
    if (n == 0) { ctx->sync(); return; }   // an empty store records the map
    hipEvent_t ev[3] = { ctx->take_event(), ctx->take_event(), ctx->take_event() };
    struct Give {
        acc_ctx *c; hipEvent_t *e;
        ~Give() { for (int i = 0; i < 3; ++i) c->event_pool.push_back(e[i]); }
    } give{ ctx, ev };
    ACC_HIP(hipEventRecord(ev[0], st));

    // ---- count: lim per input range, the pieces of every stored range, keep and the counts of every row
    const Table s = table_of(store);
    uint64_t *g = ctx->get<uint64_t>("rc_g", 8);
    ACC_HIP(hipMemsetAsync(g, 0, 8 * sizeof(uint64_t), st));
    uint32_t *lim = ctx->get<uint32_t>("rp_lim", m);
    launch(ctx, "rp_lim", k_rp_lim, dim3(grid_for(m, BLOCK)), dim3(BLOCK), 0, m, ri.bm, ri.bl, ri.bn, s, lim, g);
    uint32_t *rown = ctx->get<uint32_t>("rp_rowner", R), *chg = ctx->get<uint32_t>("rp_chg", n);
    ACC_HIP(hipMemsetAsync(chg, 0, (size_t)n * sizeof(uint32_t), st));
    launch(ctx, "rp_rowner", k_rp_rowner, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, n, s.rng_off, rown);
    const Bounds bnd{ m, ri.rs, ri.re, lim };
    uint64_t *cnt = ctx->get<uint64_t>("rp_cnt", R), *poff = ctx->get<uint64_t>("rp_poff", (size_t)R + 1);
    launch(ctx, "rp_count", k_rp_cut<false>, dim3(grid_for(R, BLOCK)), dim3(BLOCK), 0, R, s, (const uint32_t *)rown, bnd, cnt, chg,
           Pruned{}, g);
    scan<uint64_t, OpAdd<uint64_t>>(ctx, cnt, poff, R, true, poff + R);
    uint64_t *keep = ctx->get<uint64_t>("rp_keep", n), *kcnt = ctx->get<uint64_t>("rp_kcnt", n), *kdep = ctx->get<uint64_t>("rp_kdep", n);
    uint64_t *cutf = ctx->get<uint64_t>("rp_cutf", n);
    uint64_t *kidx = ctx->get<uint64_t>("rp_kidx", (size_t)n + 1), *roff = ctx->get<uint64_t>("rp_roff", (size_t)n + 1);
    uint64_t *doff = ctx->get<uint64_t>("rp_doff", (size_t)n + 1), *cidx = ctx->get<uint64_t>("rp_cidx", (size_t)n + 1);
    launch(ctx, "rp_rows", k_rp_rows, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, s, (const uint64_t *)poff, (const uint32_t *)chg, keep,
           kcnt, kdep, cutf, (const uint64_t *)g);
    {
        const uint64_t *in4[4] = { keep, kcnt, kdep, cutf };
        uint64_t *out4[4] = { kidx, roff, doff, cidx }, *tot4[4] = { kidx + n, roff + n, doff + n, cidx + n };
        const size_t n4[4] = { n, n, n, n };
        scan_multi<uint64_t, OpAdd<uint64_t>>(ctx, 4, in4, out4, n4, true, tot4);
    }
    // ---- the one read-back: the new sizes and the rows cut (rows dropped = n - n2)
    uint64_t ncut, ndrop, n2, R2, ND2;
    {
        ReadBack rb(ctx);
        const auto a = rb.u64(kidx + n);
        const auto b = rb.u64(roff + n);
        const auto c = rb.u64(doff + n);
        const auto d = rb.u64(cidx + n);
        rb.wait();
        n2 = a; R2 = b; ND2 = c; ncut = d;
    }
    if (n2 > n || ND2 > store->ND) fail(ACC_E_STATE, "internal: a prune grew the range-command table");
    ndrop = n - n2;
    ctx->stat("rcmd.redundant_cmds_cut", ncut);
    ctx->stat("rcmd.redundant_cmds_dropped", ndrop);
    if (ncut == 0 && ndrop == 0) return;   // no array is rewritten, every view stays valid
    if (R2 >= 0xFFFFFFFFull) fail(ACC_E_CAP, "range-command store too large (ranges >= 2^32 - 1)");

    // ---- emit: every column once, the index's inputs with them
    const TableOut o = table_out(ctx, (uint32_t)n2, R2, ND2);
    RdBuild b = index_inputs(ctx, store, (uint32_t)n2, R2);
    uint32_t *dsrc = ctx->get<uint32_t>("rp_dsrc", n2);
    launch(ctx, "rp_write", k_rp_write, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, s, (const uint64_t *)keep, (const uint64_t *)kidx,
           (const uint64_t *)roff, (const uint64_t *)doff, o, b.tinfo, dsrc);
    launch(ctx, "rp_cut", k_rp_cut<true>, dim3(grid_for(R, BLOCK)), dim3(BLOCK), 0, R, s, (const uint32_t *)rown, bnd, (uint64_t *)nullptr,
           (uint32_t *)nullptr, Pruned{ poff, kidx, roff, o.rs, o.re, b.rowner, b.eflag }, g);
    rb::Cols dc{};
    dc.s64[0] = s.dep.m; dc.s64[1] = s.dep.l; dc.s64[2] = s.dep.s; dc.s64[3] = s.dep.e;
    dc.d64[0] = o.dm; dc.d64[1] = o.dl; dc.d64[2] = o.ds; dc.d64[3] = o.de;
    dc.s32[0] = s.dep.n; dc.d32[0] = o.dn;
    dc.s8 = s.dep.k; dc.d8 = o.dk;
    dc.n64 = 4; dc.n32 = 1;
    rb_segcopy(ctx, "rp_copy_deps", dc, ND2, o.dep_off + n2, (uint32_t)n2, o.dep_off, dsrc);
    ACC_HIP(hipEventRecord(ev[1], st));
    const uint32_t R0 = R;
    finish_table(ctx, store, o, b, (uint32_t)n2, R2, ND2, g);
    ACC_HIP(hipEventRecord(ev[2], st));
    ctx->sync();
    float ms_p = 0, ms_i = 0;
    ACC_HIP(hipEventElapsedTime(&ms_p, ev[0], ev[1]));
    ACC_HIP(hipEventElapsedTime(&ms_i, ev[1], ev[2]));
    ctx->stat("rcmd.redundant_prune_us", (uint64_t)(ms_p * 1000.0f));
    ctx->stat("rcmd.redundant_index_us", (uint64_t)(ms_i * 1000.0f));
    ctx->stat("rcmd.redundant_ranges_before", R0);
    ctx->stat("rcmd.redundant_ranges_after", R2);
}

void rcmd_redundant_view(acc_rcmd *store, acc_cfk_redundant_map *out)
{
    if (!store || !out) fail(ACC_E_ARG, "null argument");
    *out = acc_cfk_redundant_map{};
    out->end_inclusive = store->end_inclusive;
    if (const acc_maxconflicts *m = store->rb) {
        out->n = m->nv;
        out->st = m->st; out->en = m->en;
        out->bound = acc_ts_cols{ m->vm, m->vl, m->vn };
    }
}

static void rcmd_check_query_errors(uint64_t e)
{
    if (e & E_Q_KIND_ARG) fail(ACC_E_ARG, "Kind.ofOrdinal: invalid kind ordinal in TxnId flags");
    if (e & E_Q_KIND_STATE) fail(ACC_E_STATE, "Kind.witnesses(): LocalOnly has no witnessed kinds");
    if (e & E_Q_KOFF) fail(ACC_E_ARG, "query key_off must start at 0, be non-decreasing and end at n_pairs");
    if (e & E_Q_ROFF) fail(ACC_E_ARG, "query rng_off must start at 0, be non-decreasing and end at n_ranges");
    if (e & E_Q_RKEYS) fail(ACC_E_ARG, "a range-domain query lists keys (TxnId.domain())");
    if (e & E_Q_KRANGES) fail(ACC_E_ARG, "a key-domain query lists ranges (TxnId.domain())");
    if (e & E_Q_KEYS) fail(ACC_E_ARG, "keys of a query must be sorted and unique (Keys.ofSortedUnique)");
    if (e & E_BOUND) fail(ACC_E_ARG, "range start must be below its end (Range: start >= end)");
    if (e & E_ORDER) fail(ACC_E_ARG, "ranges of a query must be sorted and deoverlapped (Ranges.ofSortedAndDeoverlapped)");
}

// ---- the front end and the tail acc_rcmd_rangedeps and acc_rcmd_map_reduce_full share: what differs between them (the
// prep kernel's instantiation, the recovery route's kind errors, mirror and filter, the stats) stays in the entries

static void check_query_bounds(const acc_rcmd *store, uint32_t end_inclusive, uint64_t n_pairs, uint64_t n_ranges)
{
    if (end_inclusive > 1) fail(ACC_E_ARG, "end_inclusive must be 0 (StartInclusive) or 1 (EndInclusive)");
    if (end_inclusive != store->end_inclusive) fail(ACC_E_ARG, "end_inclusive differs from the store's Range bound type");
    if (n_pairs + n_ranges >= 0xFFFFFFFFull || n_pairs >= 0xFFFFFFFFull || n_ranges >= 0xFFFFFFFFull)
        fail(ACC_E_ARG, "n_pairs + n_ranges must be < 2^32");
}

// the build record of nq queries over the store's table, sized, with its three offset buffers; no query admits no
// participants
static RdBuild begin_query(acc_ctx *ctx, const acc_rcmd *store, uint32_t nq, uint64_t n_pairs, uint64_t n_ranges)
{
    ctx->rd_valid = false;
    RdBuild b;
    b.n = nq;
    b.npos = store->n;
    b.P = (size_t)n_pairs;
    b.R = (size_t)n_ranges;
    b.Q = (uint32_t)(b.P + b.R);
    b.end_inclusive = (int)store->end_inclusive;
    b.arena_off = ctx->get<uint64_t>("rd_arena_off", (size_t)nq + 1);
    b.rd_off = ctx->get<uint64_t>("rd_rd_off", (size_t)nq + 1);
    b.u_off = ctx->get<uint64_t>("rd_u_off", (size_t)nq + 1);
    if (nq == 0 && b.P) fail(ACC_E_ARG, "query key_off must start at 0, be non-decreasing and end at n_pairs");
    if (nq == 0 && b.R) fail(ACC_E_ARG, "query rng_off must start at 0, be non-decreasing and end at n_ranges");
    return b;
}

// the view of a call that stabs nothing: every query empty, the store's dictionary (placeholders while it has none).
// The caller records its stats and syncs.
static void publish_empty(acc_ctx *ctx, const acc_rcmd *store, const RdBuild &b, acc_rangedeps_view *view)
{
    hipStream_t st = ctx->stream;
    const uint32_t nq = b.n;
    const uint64_t *dict_s = store->dict_s ? store->dict_s : ctx->get<uint64_t>("rc_dict0", 2);
    const uint64_t *dict_e = store->dict_e ? store->dict_e : ctx->get<uint64_t>("rc_dict0", 2);
    ACC_HIP(hipMemsetAsync(b.arena_off, 0, ((size_t)nq + 1) * 8, st));
    ACC_HIP(hipMemsetAsync(b.rd_off, 0, ((size_t)nq + 1) * 8, st));
    ACC_HIP(hipMemsetAsync(b.u_off, 0, ((size_t)nq + 1) * 8, st));
    *view = acc_rangedeps_view{ nq, store->n_dict, 0, 0, 0, 0, dict_s, dict_e, b.arena_off, ctx->get<int32_t>("rd_arena", 1),
                                b.rd_off, ctx->get<uint32_t>("rd_range_id", 1), b.u_off, ctx->get<uint32_t>("rd_dep_txn", 1) };
    ctx->rd_view = *view;
    ctx->rd_valid = true;
}

// stages the queries of `in` (ids their TxnIds, execute_at their bounds or null: the TxnIds) and allocates what the prep
// kernel writes: b.tinfo, owner, b.rowner and the zeroed words g ([0] errors, [1] low-bound mask, from [4] the entry's)
template <class In>
static Queries stage_queries(acc_ctx *ctx, RdBuild &b, const In *in, const acc_ts_cols &ids, const acc_ts_cols *execute_at,
                             uint32_t *&owner, uint64_t *&g)
{
    const uint32_t nq = b.n, mem = in->mem;
    Queries Q{};
    Q.nq = nq; Q.P = (uint32_t)b.P; Q.R = (uint32_t)b.R;
    Q.tm = stage_in(ctx, "rc_q_tm", ids.msb, nq, mem);
    Q.tl = stage_in(ctx, "rc_q_tl", ids.lsb, nq, mem);
    Q.tn = stage_in(ctx, "rc_q_tn", ids.node, nq, mem);
    if (execute_at && execute_at->msb) {
        Q.xm = stage_in(ctx, "rc_q_xm", execute_at->msb, nq, mem);
        Q.xl = stage_in(ctx, "rc_q_xl", execute_at->lsb, nq, mem);
        Q.xn = stage_in(ctx, "rc_q_xn", execute_at->node, nq, mem);
    } else {
        Q.xm = Q.tm; Q.xl = Q.tl; Q.xn = Q.tn;
    }
    Q.key_off = stage_in(ctx, "rc_q_koff", in->key_off, (size_t)nq + 1, mem);
    Q.key = stage_in(ctx, "rc_q_key", in->key_code, b.P, mem);
    Q.rng_off = stage_in(ctx, "rc_q_roff", in->rng_off, (size_t)nq + 1, mem);
    Q.rs = stage_in(ctx, "rc_q_rs", in->rng_start, b.R, mem);
    Q.re = stage_in(ctx, "rc_q_re", in->rng_end, b.R, mem);
    g = ctx->get<uint64_t>("rc_g", 8);
    ACC_HIP(hipMemsetAsync(g, 0, 8 * sizeof(uint64_t), ctx->stream));
    b.tinfo = ctx->get<uint4>("rd_tinfo", nq);
    owner = ctx->get<uint32_t>("owner", b.P);
    b.rowner = ctx->get<uint32_t>("rd_rowner", b.R);
    return Q;
}

// the prep kernel's words: the low-bound mask into b; returns the error bits
static uint64_t read_prep(acc_ctx *ctx, const uint64_t *g, RdBuild &b)
{
    ReadBack rb(ctx);
    const auto hg = rb.words(g, 2);
    rb.wait();
    b.mask_lo = hg[1];
    return hg[0];
}

// the reused stages (rd_stab_queries, rd_build_txns) read the staged queries and the store's index
static void bind_store_index(RdBuild &b, const acc_rcmd *store, const Queries &Q, const uint32_t *owner)
{
    b.key_off = Q.key_off; b.rng_off = Q.rng_off;
    b.key_code = Q.key; b.rs = Q.rs; b.re = Q.re;
    b.tl = Q.tl;
    b.owner = owner;
    b.dict.batch_sorted = true;   // tpos is the table index: no txn_of_tpos
    b.NE = store->NE;
    b.dict_s = store->dict_s; b.dict_e = store->dict_e; b.dincl = store->dincl;
    b.cs_s = store->cs_s; b.cs_e = store->cs_e; b.cs_info = store->cs_info; b.cs_kind = store->cs_kind;
    b.class_off = store->cls + (rd::NCLS + 1);
}

static void publish_view(acc_ctx *ctx, const RdBuild &b, acc_rangedeps_view *view)
{
    *view = acc_rangedeps_view{ b.n, b.n_dict, b.tot_arena, b.tot_rd, b.tot_u, b.tot_arena - b.tot_rd, b.dict_s, b.dict_e, b.arena_off,
                                b.o.arena, b.rd_off, b.o.range_id, b.u_off, b.o.dep_txn };
    ctx->rd_view = *view;
    ctx->rd_valid = true;
}

RdBuild rcmd_begin_rangedeps(acc_ctx *ctx, const acc_rcmd *store, const acc_cfk_mixed_queries *in)
{
    if (in->mem != ACC_MEM_HOST && in->mem != ACC_MEM_DEVICE) fail(ACC_E_ARG, "mem must be ACC_MEM_HOST or ACC_MEM_DEVICE");
    check_query_bounds(store, in->end_inclusive, in->n_pairs, in->n_ranges);
    return begin_query(ctx, store, in->n_query, in->n_pairs, in->n_ranges);
}

Queries rcmd_prep_rangedeps(acc_ctx *ctx, const acc_rcmd *store, const acc_cfk_mixed_queries *in, RdBuild &b, uint32_t *&owner)
{
    uint64_t *g = nullptr;
    const Queries Q = stage_queries(ctx, b, in, in->txn_id, &in->execute_at, owner, g);
    launch(ctx, "rc_qprep", k_rc_qprep<false>, dim3(grid_for(b.n, BLOCK)), dim3(BLOCK), 0, Q, table_of(store), 0, 0u, b.tinfo, owner,
           b.rowner, g);
    rcmd_check_query_errors(read_prep(ctx, g, b));
    return Q;
}

void rcmd_bind_store_index(RdBuild &b, const acc_rcmd *store, const Queries &Q, const uint32_t *owner)
{
    bind_store_index(b, store, Q, owner);
}

void rcmd_rangedeps_stats(acc_ctx *ctx, const acc_rcmd *store, const RdBuild &b, bool stabbed)
{
    ctx->stat("rangedeps.entries", store->NE);
    ctx->stat("rangedeps.stored_ranges", store->n_dict);
    ctx->stat("rangedeps.queries", b.Q);
    ctx->stat("rangedeps.raw_entries", stabbed ? b.E : 0);
    if (!stabbed) return;
    ctx->stat("rangedeps.stab_passes", b.stab_passes);
    ctx->stat("rangedeps.s16_txns", b.tier_txns[1]);
    ctx->stat("rangedeps.s32_txns", b.tier_txns[11]);
    ctx->stat("rangedeps.s64_txns", b.tier_txns[2]);
    ctx->stat("rangedeps.block_txns", b.block_txns);
    ctx->stat("rangedeps.global_txns", b.tier_txns[10]);
}

void rcmd_publish_view(acc_ctx *ctx, const RdBuild &b, acc_rangedeps_view *view) { publish_view(ctx, b, view); }

void rcmd_rangedeps(acc_ctx *ctx, acc_rcmd *store, const acc_cfk_mixed_queries *in, acc_rangedeps_view *view)
{
    if (!store || !in || !view) fail(ACC_E_ARG, "null argument");
    RdBuild b = rcmd_begin_rangedeps(ctx, store, in);
    auto empty = [&] {
        publish_empty(ctx, store, b, view);
        rcmd_rangedeps_stats(ctx, store, b, false);
        ctx->sync();
    };
    if (in->n_query == 0) return empty();

    // ---- stage and validate; the per-query rows
    uint32_t *owner = nullptr;
    const Queries Q = rcmd_prep_rangedeps(ctx, store, in, b, owner);
    if (store->NE == 0) return empty();   // nothing to stab: no commands, or none with ranges that is not erased

    // ---- the reused stages over the store's index
    bind_store_index(b, store, Q, owner);
    rd_stab_queries(ctx, b);
    rd_build_txns(ctx, b);
    rcmd_rangedeps_stats(ctx, store, b, true);
    ctx->sync();
    publish_view(ctx, b, view);
}

void rcmd_map_reduce_full(acc_ctx *ctx, acc_rcmd *store, const acc_cfk_recovery_in *in, acc_rangedeps_view *view)
{
    if (!store || !in || !view) fail(ACC_E_ARG, "null argument");
    if (in->mem != ACC_MEM_HOST && in->mem != ACC_MEM_DEVICE) fail(ACC_E_ARG, "mem must be ACC_MEM_HOST or ACC_MEM_DEVICE");
    const RcParams prm = recovery_params(in->started_at, in->test_dep, in->test_status, in->flags, in->test_kinds);
    check_query_bounds(store, in->end_inclusive, in->n_pairs, in->n_ranges);
    const uint64_t wl0 = ctx->wave_launches;
    const uint32_t nq = in->n_query, n = store->n;
    RdBuild b = begin_query(ctx, store, nq, in->n_pairs, in->n_ranges);
    auto stats = [&](uint64_t raw, uint64_t kept, uint64_t probes) {
        ctx->stat("rcr.queries", b.Q);
        ctx->stat("rcr.raw_entries", raw);
        ctx->stat("rcr.kept_entries", kept);
        ctx->stat("rcr.dep_probes", probes);
        ctx->stat("rcr.wave_launches", ctx->wave_launches - wl0);
    };
    auto empty = [&] { publish_empty(ctx, store, b, view); stats(0, 0, 0); ctx->sync(); };
    if (nq == 0) return empty();

    // ---- stage and validate; the per-query rows
    uint32_t *owner = nullptr;
    uint64_t *g = nullptr;
    const Queries Q = stage_queries(ctx, b, in, in->test_txn, nullptr, owner, g);
    launch(ctx, "rcr_qprep", k_rc_qprep<true>, dim3(grid_for(nq, BLOCK)), dim3(BLOCK), 0, Q, table_of(store), (int)prm.test_kinds,
           prm.started_at, b.tinfo, owner, b.rowner, g);
    const uint64_t e = read_prep(ctx, g, b);
    if (e & E_Q_KIND_STATE) fail(ACC_E_STATE, "Kind.witnessedBy(): unhandled kind LocalOnly (AssertionError)");
    if (e & E_Q_KIND_ARG) fail(ACC_E_ARG, "Kind.ofOrdinal: invalid kind ordinal in a testTxnId");
    rcmd_check_query_errors(e);
    if (store->NE == 0 || b.Q == 0) return empty();   // nothing to stab, or nothing to stab with

    // ---- the stabbing pass as it is, over the store's index (STARTED_AFTER: positions counted from the top)
    bind_store_index(b, store, Q, owner);
    const bool mirror = prm.started_at == ACC_STARTED_AFTER;
    if (mirror) {
        uint2 *mi = ctx->get<uint2>("rcr_info", store->NE);
        launch(ctx, "rcr_mirror", k_rcr_mirror, dim3(grid_for(store->NE, BLOCK)), dim3(BLOCK), 0, store->NE, n,
               (const uint2 *)store->cs_info, mi);
        b.cs_info = mi;
    }
    rd_stab_queries(ctx, b);

    // ---- the command tests on the candidates alone
    const StateCols c{ store->tm, store->tl, store->em, store->el, store->tn, store->en, store->status, store->flags, store->rng_off,
                       store->rs, store->re, store->dep_off, store->dm, store->dl, store->dn, store->ds, store->de, store->dk,
                       store->end_inclusive };
    uint64_t *fst = g + 4;   // zeroed with g; the prep kernel writes g[0], g[1]
    if (b.E)
        launch_waves(ctx, "rcr_filter", k_rcr_filter, (uint64_t)b.Q, (uint64_t)b.Q, (uint32_t)b.P, (const uint32_t *)owner,
                     (const uint32_t *)b.rowner, c, Q.tm, Q.tl, Q.tn, (const uint4 *)b.tinfo, prm, mirror ? n : 0u, b.v.q_out, b.v.ent, fst);
    rd_build_txns(ctx, b);
    ReadBack rb(ctx);
    const auto hs = rb.words((const uint64_t *)fst, 2);
    rb.wait();
    stats(b.E, hs[0], hs[1]);
    publish_view(ctx, b, view);
}

}  // namespace acc
