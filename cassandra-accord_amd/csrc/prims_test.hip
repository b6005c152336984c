// prims_test.hip — a test shim over prims.hpp and search.hpp (libaccord_prims_test.so): NOT part of the product ABI, nothing here is
// declared in include/accord_amd.h. Each entry point runs one primitive on an acc_ctx made by the main library's
// acc_create (acc_ctx is header-only; both libraries are built with the same flags, so the layout is the same), takes
// HOST arrays in and out, and returns after a sync: the Python side (tests/test_prims_gpu.py, tests/test_search_gpu.py)
// needs numpy and ctypes only.
// Every device output buffer is filled with FILL bytes before the primitive runs and copied back whole, one guard
// element included, so a store the primitive should not have made shows in the result.
#include "prims.hpp"
#include "search.hpp"

#include <map>

using namespace acc;

namespace {

constexpr int FILL = 0xA5;

template <class T>
T *upload(acc_ctx *ctx, const char *name, const T *host, size_t n)
{
    T *d = ctx->get<T>(name, n);
    if (n) ACC_HIP(hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return d;
}

template <class T>
T *filled(acc_ctx *ctx, const char *name, size_t n)
{
    T *d = ctx->get<T>(name, n);
    if (n) ACC_HIP(hipMemsetAsync(d, FILL, n * sizeof(T), ctx->stream));
    return d;
}

template <class T>
void download(acc_ctx *ctx, T *host, const T *dev, size_t n)
{
    if (n) ACC_HIP(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
}

// total modes of a scanned array
enum { TOT_NONE = 0, TOT_WORD = 1, TOT_CSR = 2 };   // no total / a separate word / out + n (the callers' CSR idiom)

// k arrays through scan_multi (or scan(), k == 1 && single): in[i] holds n[i] elements, out[i] n[i] + 1 (the last one is
// the total in TOT_CSR mode and stays FILL otherwise), totals k elements (FILL where no separate word was asked for).
template <class T, class Op>
void run_scans(acc_ctx *ctx, int k, const void *const *in, void *const *out, const uint64_t *n, int exclusive,
               const int *tot_mode, void *totals, int side_lane, bool single)
{
    std::vector<const T *> din(k);
    std::vector<T *> dout(k), dtot(k);
    std::vector<size_t> dn(k);
    T *tw = filled<T>(ctx, "pt_tot", (size_t)k);
    char name[32];
    bool any_total = false;
    for (int i = 0; i < k; ++i) {
        snprintf(name, sizeof name, "pt_in%d", i);
        din[i] = upload(ctx, name, static_cast<const T *>(in[i]), (size_t)n[i]);
        snprintf(name, sizeof name, "pt_out%d", i);
        dout[i] = filled<T>(ctx, name, (size_t)n[i] + 1);
        dn[i] = (size_t)n[i];
        dtot[i] = tot_mode[i] == TOT_WORD ? tw + i : tot_mode[i] == TOT_CSR ? dout[i] + n[i] : nullptr;
        any_total |= dtot[i] != nullptr;
    }
    if (side_lane) {   // the staging above is on the main stream: the fork orders the lane behind it
        ctx->lane_fork();
        ctx->launch_stream = ctx->aux[0];
    }
    if (single) scan<T, Op>(ctx, din[0], dout[0], dn[0], exclusive != 0, dtot[0]);
    else scan_multi<T, Op>(ctx, k, din.data(), dout.data(), dn.data(), exclusive != 0,
                           any_total ? dtot.data() : (T *const *)nullptr);   // (callers without totals pass no array)
    if (side_lane) ctx->lane_join();
    for (int i = 0; i < k; ++i) download(ctx, static_cast<T *>(out[i]), dout[i], (size_t)n[i] + 1);
    download(ctx, static_cast<T *>(totals), tw, (size_t)k);
    ctx->sync();
}

// type: 0 u32 add, 1 u32 max, 2 u64 add, 3 u64 max
void run_scans_typed(acc_ctx *ctx, int type, int k, const void *const *in, void *const *out, const uint64_t *n, int exclusive,
                     const int *tot_mode, void *totals, int side_lane, bool single)
{
    switch (type) {
    case 0: run_scans<uint32_t, OpAdd<uint32_t>>(ctx, k, in, out, n, exclusive, tot_mode, totals, side_lane, single); break;
    case 1: run_scans<uint32_t, OpMax<uint32_t>>(ctx, k, in, out, n, exclusive, tot_mode, totals, side_lane, single); break;
    case 2: run_scans<uint64_t, OpAdd<uint64_t>>(ctx, k, in, out, n, exclusive, tot_mode, totals, side_lane, single); break;
    case 3: run_scans<uint64_t, OpMax<uint64_t>>(ctx, k, in, out, n, exclusive, tot_mode, totals, side_lane, single); break;
    default: fail(ACC_E_ARG, "prims_test: scan type");
    }
}

// the last result of each (context, tag): read again by acct_sort_result after other tags have sorted
struct SortResult {
    Sorted s;
    size_t n;
};
std::map<std::pair<acc_ctx *, std::string>, SortResult> g_sorted;

void sort_download(acc_ctx *ctx, const SortResult &r, uint64_t *keys_out, uint32_t *vals_out)
{
    download(ctx, keys_out, r.s.keys, r.n);
    if (vals_out) download(ctx, vals_out, r.s.vals, r.n);
    ctx->sync();
}

// ---------------------------------------------------------------- block and wave primitives, one per kernel

template <class T, class Op>
__global__ __launch_bounds__(BLOCK) void k_t_block_exclusive(const T *__restrict__ in, T *__restrict__ out, T *__restrict__ totals)
{
    __shared__ T lds[4];
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    T total;
    out[i] = block_exclusive<T, Op, 4>(in[i], Op(), lds, total);
    if (threadIdx.x == BLOCK - 1) totals[blockIdx.x] = total;   // (every thread holds it; the last one reports)
}

template <class T>
__global__ __launch_bounds__(BLOCK) void k_t_bitonic_reg(const T *__restrict__ in, T *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    out[i] = bitonic_reg<T>(in[i]);
}

// block b sorts a[b * n2, (b + 1) * n2): in LDS (n2 <= LDS_MAX) or in place in global memory
constexpr uint32_t BB_LDS_MAX = 8192;
template <class T, bool LDS>
__global__ __launch_bounds__(BLOCK) void k_t_block_bitonic(T *__restrict__ a, uint32_t n2)
{
    T *mine = a + (size_t)blockIdx.x * n2;
    if constexpr (LDS) {
        __shared__ T s[BB_LDS_MAX];
        for (uint32_t i = threadIdx.x; i < n2; i += BLOCK) s[i] = mine[i];
        __syncthreads();
        block_bitonic<T>(s, n2);
        for (uint32_t i = threadIdx.x; i < n2; i += BLOCK) mine[i] = s[i];
    } else {
        block_bitonic<T>(mine, n2);
    }
}

// one workgroup walks the chunks of [off[0], off[nt]) as the library's copy loops do: own_out[c * CH + p] = own[p] of
// chunk c, carry_out[c] = the carry after it
template <int PT>
__global__ __launch_bounds__(BLOCK) void k_t_chunk_owners(uint32_t nt, const uint64_t *__restrict__ off_g,
                                                        uint32_t *__restrict__ own_out, uint32_t *__restrict__ carry_out)
{
    constexpr uint32_t CH = (uint32_t)PT * BLOCK;
    __shared__ uint64_t off[BLOCK + 1];
    __shared__ uint32_t own[CH], red[WAVES];
    const uint32_t tid = threadIdx.x;
    if (tid <= nt) off[tid] = off_g[tid];
    if (tid == 0) off[nt] = off_g[nt];
    __syncthreads();
    const uint64_t j1 = off[nt];
    uint32_t carry = 0, c = 0;
    for (uint64_t c0 = off[0]; c0 < j1; c0 += CH, ++c) {
        chunk_owners<PT>(nt, off, c0, own, red, carry);
        for (uint32_t p = tid; p < CH; p += BLOCK) own_out[(size_t)c * CH + p] = own[p];
        if (tid == 0) carry_out[c] = carry;
    }
}

__global__ __launch_bounds__(BLOCK) void k_t_pext_runs(size_t n, const uint64_t *__restrict__ w, Runs r, uint64_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = pext_runs(w[i], r);
}

// ---------------------------------------------------------------- search.hpp, one kernel per helper, a thread per query

template <class T, class I, bool UPPER>
__global__ __launch_bounds__(BLOCK) void k_t_bound(const T *__restrict__ a, const uint64_t *__restrict__ lo,
                                                   const uint64_t *__restrict__ hi, const uint64_t *__restrict__ v, uint32_t nq,
                                                   uint64_t *__restrict__ out)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= nq) return;
    out[q] = UPPER ? upper_bound(a, (I)lo[q], (I)hi[q], (T)v[q]) : lower_bound(a, (I)lo[q], (I)hi[q], (T)v[q]);
}

__global__ __launch_bounds__(BLOCK) void k_t_seg_of(const uint32_t *__restrict__ off, uint32_t n, const uint32_t *__restrict__ v,
                                                    uint32_t nq, uint32_t *__restrict__ out)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q < nq) out[q] = seg_of(off, n, v[q]);
}

__global__ __launch_bounds__(BLOCK) void k_t_find_sorted(const uint64_t *__restrict__ a, uint32_t n, const uint64_t *__restrict__ v,
                                                         uint32_t nq, uint32_t *__restrict__ out)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q < nq) out[q] = find_sorted(a, n, v[q]);
}

struct TsCols {
    const uint64_t *m, *l;
    const int32_t *n;
};
template <bool UPPER>
__global__ __launch_bounds__(BLOCK) void k_t_ts_bound(TsCols a, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, TsCols v,
                                                      uint32_t nq, uint32_t *__restrict__ out)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= nq) return;
    const Ts t = ts_at(v.m, v.l, v.n, q);
    out[q] = UPPER ? upper_bound_ts(a.m, a.l, a.n, lo[q], hi[q], t) : lower_bound_ts(a.m, a.l, a.n, lo[q], hi[q], t);
}

// a wave per query; every lane reports the (wave-uniform) result: out[64 q + lane]
__global__ __launch_bounds__(BLOCK) void k_t_wave_search(const uint64_t *__restrict__ a, const uint32_t *__restrict__ lo,
                                                         const uint32_t *__restrict__ hi, const uint64_t *__restrict__ v, int upper,
                                                         uint32_t nq, uint32_t *__restrict__ out)
{
    const uint32_t q = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (q < nq) out[(size_t)q * 64 + lane_id()] = wave_search(a, lo[q], hi[q], v[q], upper != 0);
}

}  // namespace

extern "C" {

// one array through scan(): out holds n + 1 elements, *total one
int acct_scan(acc_ctx *ctx, int type, const void *in, void *out, uint64_t n, int exclusive, int tot_mode, void *total,
              int side_lane)
{
    return acc_guard(ctx, [&] {
        run_scans_typed(ctx, type, 1, &in, &out, &n, exclusive, &tot_mode, total, side_lane, true);
    });
}

// k arrays through scan_multi() (k outside 1 .. SCAN_MAXA is refused by scan_multi itself: ACC_E_STATE)
int acct_scan_multi(acc_ctx *ctx, int type, int k, const void *const *in, void *const *out, const uint64_t *n, int exclusive,
                    const int *tot_mode, void *totals, int side_lane)
{
    return acc_guard(ctx, [&] {
        if (k < 0 || k > 16) fail(ACC_E_ARG, "prims_test: array count");
        run_scans_typed(ctx, type, k, in, out, n, exclusive, tot_mode, totals, side_lane, false);
    });
}

int acct_sum_u32(acc_ctx *ctx, const uint32_t *in, uint64_t n, uint64_t *out)
{
    return acc_guard(ctx, [&] {
        const uint32_t *d = upload(ctx, "pt_in0", in, (size_t)n);
        uint64_t *t = filled<uint64_t>(ctx, "pt_tot", 2);
        sum_u32(ctx, d, (size_t)n, t);
        download(ctx, out, t, 2);   // out[1] is the guard word
        ctx->sync();
    });
}

// radix_sort (three_launch == 0) or radix_sort_3launch behind radix_sort's own early returns; vals may be null (iota);
// keys_out / vals_out hold n elements
int acct_radix_sort(acc_ctx *ctx, const char *tag, const uint64_t *keys, const uint32_t *vals, uint64_t n, int bits,
                    int three_launch, uint64_t *keys_out, uint32_t *vals_out)
{
    return acc_guard(ctx, [&] {
        const uint64_t *dk = upload(ctx, "pt_keys", keys, (size_t)n);
        const uint32_t *dv = vals ? upload(ctx, "pt_vals", vals, (size_t)n) : nullptr;
        const int passes = (bits + 7) / 8;
        SortResult r;
        r.n = (size_t)n;
        if (three_launch && n && passes) {
            char nk0[40], nk1[40], nv0[40], nv1[40];
            snprintf(nk0, sizeof nk0, "%s_k0", tag); snprintf(nk1, sizeof nk1, "%s_k1", tag);
            snprintf(nv0, sizeof nv0, "%s_v0", tag); snprintf(nv1, sizeof nv1, "%s_v1", tag);
            uint64_t *k[2] = { ctx->get<uint64_t>(nk0, (size_t)n), ctx->get<uint64_t>(nk1, (size_t)n) };
            uint32_t *v[2] = { ctx->get<uint32_t>(nv0, (size_t)n), ctx->get<uint32_t>(nv1, (size_t)n) };
            r.s = radix_sort_3launch(ctx, tag, dk, dv, (size_t)n, passes, k, v);
        } else {
            r.s = radix_sort(ctx, tag, dk, dv, (size_t)n, bits);
        }
        g_sorted[{ ctx, tag }] = r;
        sort_download(ctx, r, keys_out, vals_out);
    });
}

int acct_radix_sort_keys(acc_ctx *ctx, const char *tag, const uint64_t *keys, uint64_t n, int lo, int bits, uint64_t *keys_out)
{
    return acc_guard(ctx, [&] {
        const uint64_t *dk = upload(ctx, "pt_keys", keys, (size_t)n);
        SortResult r;
        r.n = (size_t)n;
        r.s = Sorted{ radix_sort_keys(ctx, tag, dk, (size_t)n, lo, bits), nullptr };
        g_sorted[{ ctx, tag }] = r;
        sort_download(ctx, r, keys_out, nullptr);
    });
}

// the tag's last result again ("valid until the next sort with the same tag"); *n_out its size
int acct_sort_result(acc_ctx *ctx, const char *tag, uint64_t cap, uint64_t *keys_out, uint32_t *vals_out, uint64_t *n_out)
{
    return acc_guard(ctx, [&] {
        auto it = g_sorted.find({ ctx, tag });
        if (it == g_sorted.end()) fail(ACC_E_STATE, "prims_test: no sort with this tag");
        *n_out = it->second.n;
        if (it->second.n > cap) fail(ACC_E_CAP, "prims_test: result larger than the arrays given");
        sort_download(ctx, it->second, keys_out, it->second.s.vals ? vals_out : nullptr);
    });
}

// forget a context's results (before acc_destroy)
void acct_forget(acc_ctx *ctx)
{
    for (auto it = g_sorted.begin(); it != g_sorted.end();) it = it->first.first == ctx ? g_sorted.erase(it) : std::next(it);
}

// nblocks blocks of BLOCK values each: out the exclusive prefixes, totals one per block. type as acct_scan.
int acct_block_exclusive(acc_ctx *ctx, int type, const void *in, uint32_t nblocks, void *out, void *totals)
{
    return acc_guard(ctx, [&] {
        const size_t n = (size_t)nblocks * BLOCK;
        auto run = [&](auto tv, auto opv) {
            using T = decltype(tv);
            using Op = decltype(opv);
            const T *d = upload(ctx, "pt_in0", static_cast<const T *>(in), n);
            T *o = filled<T>(ctx, "pt_out0", n), *t = filled<T>(ctx, "pt_tot", nblocks);
            launch(ctx, "t_block_exclusive", k_t_block_exclusive<T, Op>, dim3(nblocks), dim3(BLOCK), 0, d, o, t);
            download(ctx, static_cast<T *>(out), o, n);
            download(ctx, static_cast<T *>(totals), t, (size_t)nblocks);
        };
        switch (type) {
        case 0: run(uint32_t(), OpAdd<uint32_t>()); break;
        case 1: run(uint32_t(), OpMax<uint32_t>()); break;
        case 2: run(uint64_t(), OpAdd<uint64_t>()); break;
        case 3: run(uint64_t(), OpMax<uint64_t>()); break;
        default: fail(ACC_E_ARG, "prims_test: scan type");
        }
        ctx->sync();
    });
}

// nwaves (a multiple of WAVES: bitonic_reg needs whole waves) waves of 64 values, each sorted on its own
int acct_bitonic_reg(acc_ctx *ctx, int is64, const void *in, uint32_t nwaves, void *out)
{
    return acc_guard(ctx, [&] {
        if (nwaves % WAVES) fail(ACC_E_ARG, "prims_test: bitonic_reg takes whole blocks");
        const size_t n = (size_t)nwaves * 64;
        if (is64) {
            const uint64_t *d = upload(ctx, "pt_in0", static_cast<const uint64_t *>(in), n);
            uint64_t *o = filled<uint64_t>(ctx, "pt_out0", n);
            launch(ctx, "t_bitonic_reg", k_t_bitonic_reg<uint64_t>, dim3(nwaves / WAVES), dim3(BLOCK), 0, d, o);
            download(ctx, static_cast<uint64_t *>(out), o, n);
        } else {
            const uint32_t *d = upload(ctx, "pt_in0", static_cast<const uint32_t *>(in), n);
            uint32_t *o = filled<uint32_t>(ctx, "pt_out0", n);
            launch(ctx, "t_bitonic_reg", k_t_bitonic_reg<uint32_t>, dim3(nwaves / WAVES), dim3(BLOCK), 0, d, o);
            download(ctx, static_cast<uint32_t *>(out), o, n);
        }
        ctx->sync();
    });
}

// nblocks arrays of n2 (a power of two, 2 .. 8192) values, each sorted by one workgroup: in LDS (u32 only, as the
// library's caller) or in global memory (u32 or u64). out holds nblocks * n2 + 1 values (a guard element).
int acct_block_bitonic(acc_ctx *ctx, int is64, int in_lds, const void *in, uint32_t n2, uint32_t nblocks, void *out)
{
    return acc_guard(ctx, [&] {
        if (n2 < 2 || n2 > BB_LDS_MAX || (n2 & (n2 - 1))) fail(ACC_E_ARG, "prims_test: block_bitonic size");
        if (is64 && in_lds) fail(ACC_E_ARG, "prims_test: block_bitonic in LDS sorts u32");
        const size_t n = (size_t)nblocks * n2;
        auto run = [&](auto tv) {
            using T = decltype(tv);
            T *a = filled<T>(ctx, "pt_out0", n + 1);
            if (n) ACC_HIP(hipMemcpyAsync(a, in, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
            if constexpr (sizeof(T) == 4) {
                if (in_lds) launch(ctx, "t_block_bitonic", k_t_block_bitonic<T, true>, dim3(nblocks), dim3(BLOCK), 0, a, n2);
                else launch(ctx, "t_block_bitonic", k_t_block_bitonic<T, false>, dim3(nblocks), dim3(BLOCK), 0, a, n2);
            } else {
                launch(ctx, "t_block_bitonic", k_t_block_bitonic<T, false>, dim3(nblocks), dim3(BLOCK), 0, a, n2);
            }
            download(ctx, static_cast<T *>(out), a, n + 1);
        };
        if (is64) run(uint64_t()); else run(uint32_t());
        ctx->sync();
    });
}

// chunk_owners<8> (the only PT the library instantiates) over the nt runs off[0 .. nt], nt <= BLOCK: own_out holds
// nchunks * 8 * BLOCK owners (nchunks = ceil((off[nt] - off[0]) / (8 * BLOCK))), carry_out nchunks carries
int acct_chunk_owners(acc_ctx *ctx, uint32_t nt, const uint64_t *off, uint32_t *own_out, uint32_t *carry_out)
{
    return acc_guard(ctx, [&] {
        constexpr int PT = 8;
        constexpr uint64_t CH = (uint64_t)PT * BLOCK;
        if (nt < 1 || nt > (uint32_t)BLOCK) fail(ACC_E_ARG, "prims_test: chunk_owners run count");
        for (uint32_t i = 0; i < nt; ++i)
            if (off[i] > off[i + 1]) fail(ACC_E_ARG, "prims_test: chunk_owners offsets must ascend");
        const uint64_t nch = (off[nt] - off[0] + CH - 1) / CH;
        if (nch > 4096) fail(ACC_E_ARG, "prims_test: chunk_owners range");
        const uint64_t *d = upload(ctx, "pt_in0", off, (size_t)nt + 1);
        uint32_t *o = filled<uint32_t>(ctx, "pt_out0", (size_t)(nch * CH));
        uint32_t *c = filled<uint32_t>(ctx, "pt_out1", (size_t)nch);
        launch(ctx, "t_chunk_owners", k_t_chunk_owners<PT>, dim3(1), dim3(BLOCK), 0, nt, d, o, c);
        download(ctx, own_out, o, (size_t)(nch * CH));
        download(ctx, carry_out, c, (size_t)nch);
        ctx->sync();
    });
}

// out[i] = pext_runs(w[i], make_runs(mask)); *bits_out = Runs.bits, *nruns_out = Runs.n
int acct_pext_runs(acc_ctx *ctx, uint64_t mask, const uint64_t *w, uint64_t n, uint64_t *out, int *bits_out, int *nruns_out)
{
    return acc_guard(ctx, [&] {
        const Runs r = make_runs(mask);
        *bits_out = r.bits;
        *nruns_out = r.n;
        const uint64_t *d = upload(ctx, "pt_in0", w, (size_t)n);
        uint64_t *o = filled<uint64_t>(ctx, "pt_out0", (size_t)n);
        launch(ctx, "t_pext_runs", k_t_pext_runs, dim3(grid_for((size_t)n, BLOCK)), dim3(BLOCK), 0, (size_t)n, d, r, o);
        download(ctx, out, o, (size_t)n);
        ctx->sync();
    });
}

// lower_bound (upper == 0) / upper_bound over a[0, n) of u32 (elem64 == 0) or u64 elements, with a u32 (idx64 == 0) or u64
// index type: query q searches the window [lo[q], hi[q]) for v[q]. out holds nq + 1 values (a guard element).
int acct_search_bound(acc_ctx *ctx, int elem64, int idx64, int upper, const void *a, uint64_t n, const uint64_t *lo,
                      const uint64_t *hi, const uint64_t *v, uint32_t nq, uint64_t *out)
{
    return acc_guard(ctx, [&] {
        for (uint32_t q = 0; q < nq; ++q)
            if (lo[q] > hi[q] || hi[q] > n) fail(ACC_E_ARG, "prims_test: search window outside the array");
        const uint64_t *dlo = upload(ctx, "pt_lo", lo, nq), *dhi = upload(ctx, "pt_hi", hi, nq), *dv = upload(ctx, "pt_v", v, nq);
        uint64_t *o = filled<uint64_t>(ctx, "pt_out0", (size_t)nq + 1);
        auto run = [&](auto tv, auto iv) {
            using T = decltype(tv);
            using I = decltype(iv);
            const T *d = upload(ctx, "pt_in0", static_cast<const T *>(a), (size_t)n);
            if (!nq) return;
            if (upper) launch(ctx, "t_bound", k_t_bound<T, I, true>, dim3(grid_for(nq, BLOCK)), dim3(BLOCK), 0, d, dlo, dhi, dv, nq, o);
            else launch(ctx, "t_bound", k_t_bound<T, I, false>, dim3(grid_for(nq, BLOCK)), dim3(BLOCK), 0, d, dlo, dhi, dv, nq, o);
        };
        if (elem64) { if (idx64) run(uint64_t(), uint64_t()); else run(uint64_t(), uint32_t()); }
        else { if (idx64) run(uint32_t(), uint64_t()); else run(uint32_t(), uint32_t()); }
        download(ctx, out, o, (size_t)nq + 1);
        ctx->sync();
    });
}

// out[q] = seg_of(off, n, v[q]) over the n offsets off[0, n); out holds nq + 1 values
int acct_seg_of(acc_ctx *ctx, const uint32_t *off, uint32_t n, const uint32_t *v, uint32_t nq, uint32_t *out)
{
    return acc_guard(ctx, [&] {
        const uint32_t *d = upload(ctx, "pt_in0", off, n), *dv = upload(ctx, "pt_v", v, nq);
        uint32_t *o = filled<uint32_t>(ctx, "pt_out0", (size_t)nq + 1);
        if (nq) launch(ctx, "t_seg_of", k_t_seg_of, dim3(grid_for(nq, BLOCK)), dim3(BLOCK), 0, d, n, dv, nq, o);
        download(ctx, out, o, (size_t)nq + 1);
        ctx->sync();
    });
}

// out[q] = find_sorted(a, n, v[q]); out holds nq + 1 values
int acct_find_sorted(acc_ctx *ctx, const uint64_t *a, uint32_t n, const uint64_t *v, uint32_t nq, uint32_t *out)
{
    return acc_guard(ctx, [&] {
        const uint64_t *d = upload(ctx, "pt_in0", a, n), *dv = upload(ctx, "pt_v", v, nq);
        uint32_t *o = filled<uint32_t>(ctx, "pt_out0", (size_t)nq + 1);
        if (nq) launch(ctx, "t_find_sorted", k_t_find_sorted, dim3(grid_for(nq, BLOCK)), dim3(BLOCK), 0, d, n, dv, nq, o);
        download(ctx, out, o, (size_t)nq + 1);
        ctx->sync();
    });
}

// lower_bound_ts (upper == 0) / upper_bound_ts over the column triple (m, l, nd)[0, n): query q searches [lo[q], hi[q]) for
// (qm, ql, qn)[q]; out holds nq + 1 values
int acct_ts_bound(acc_ctx *ctx, int upper, const uint64_t *m, const uint64_t *l, const int32_t *nd, uint32_t n, const uint32_t *lo,
                  const uint32_t *hi, const uint64_t *qm, const uint64_t *ql, const int32_t *qn, uint32_t nq, uint32_t *out)
{
    return acc_guard(ctx, [&] {
        for (uint32_t q = 0; q < nq; ++q)
            if (lo[q] > hi[q] || hi[q] > n) fail(ACC_E_ARG, "prims_test: search window outside the array");
        const TsCols a{ upload(ctx, "pt_am", m, n), upload(ctx, "pt_al", l, n), upload(ctx, "pt_an", nd, n) };
        const TsCols v{ upload(ctx, "pt_qm", qm, nq), upload(ctx, "pt_ql", ql, nq), upload(ctx, "pt_qn", qn, nq) };
        const uint32_t *dlo = upload(ctx, "pt_lo", lo, nq), *dhi = upload(ctx, "pt_hi", hi, nq);
        uint32_t *o = filled<uint32_t>(ctx, "pt_out0", (size_t)nq + 1);
        if (nq && upper) launch(ctx, "t_ts_bound", k_t_ts_bound<true>, dim3(grid_for(nq, BLOCK)), dim3(BLOCK), 0, a, dlo, dhi, v, nq, o);
        else if (nq) launch(ctx, "t_ts_bound", k_t_ts_bound<false>, dim3(grid_for(nq, BLOCK)), dim3(BLOCK), 0, a, dlo, dhi, v, nq, o);
        download(ctx, out, o, (size_t)nq + 1);
        ctx->sync();
    });
}

// wave_search over a[0, n), one wave per query window [lo[q], hi[q]); out holds 64 * nq + 1 values: every lane's result
int acct_wave_search(acc_ctx *ctx, const uint64_t *a, uint32_t n, const uint32_t *lo, const uint32_t *hi, const uint64_t *v,
                     int upper, uint32_t nq, uint32_t *out)
{
    return acc_guard(ctx, [&] {
        for (uint32_t q = 0; q < nq; ++q)
            if (lo[q] > hi[q] || hi[q] > n) fail(ACC_E_ARG, "prims_test: search window outside the array");
        const uint64_t *d = upload(ctx, "pt_in0", a, n), *dv = upload(ctx, "pt_v", v, nq);
        const uint32_t *dlo = upload(ctx, "pt_lo32", lo, nq), *dhi = upload(ctx, "pt_hi32", hi, nq);
        uint32_t *o = filled<uint32_t>(ctx, "pt_out0", (size_t)nq * 64 + 1);
        if (nq) launch(ctx, "t_wave_search", k_t_wave_search, dim3((nq + WAVES - 1) / WAVES), dim3(BLOCK), 0, d, dlo, dhi, dv, upper, nq, o);
        download(ctx, out, o, (size_t)nq * 64 + 1);
        ctx->sync();
    });
}

}  // extern "C"
