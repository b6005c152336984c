// search.hpp — the one set of searches over sorted device arrays: the bisection every lower / upper bound goes through,
// the segment lookup over an offsets array, the key lookup of the resident stores, and the 64-ary search by one wave.
// The Java-shaped three-way searches (Arrays.binarySearch's -(lo + 1)) stay where they are used (cfkdeps.hip,
// keydeps.hpp). tests/test_search_gpu.py runs each of these on its own through prims_test.hip.
#pragma once

#include "prims.hpp"
#include "ts.hpp"

#include <type_traits>

namespace acc {

// first index i of [lo, hi) with !below(i), hi if none; below must be true on a prefix of the window and false after it
template <class I, class Below>
__device__ __forceinline__ I partition_point(I lo, I hi, Below below)
{
    while (lo < hi) { const I m = (lo + hi) >> 1; if (below(m)) lo = m + 1; else hi = m; }
    return lo;
}

// first index of the sorted a[lo, hi) with a[i] >= v (lower) or a[i] > v (upper); the index type is that of hi
template <class T, class I>
__device__ __forceinline__ I lower_bound(const T *a, std::common_type_t<I> lo, I hi, std::common_type_t<T> v)
{
    return partition_point(lo, hi, [&](I m) { return a[m] < v; });
}
template <class T, class I>
__device__ __forceinline__ I upper_bound(const T *a, std::common_type_t<I> lo, I hi, std::common_type_t<T> v)
{
    return partition_point(lo, hi, [&](I m) { return a[m] <= v; });
}

// the same over a Timestamp column triple, in Timestamp order
__device__ __forceinline__ uint32_t lower_bound_ts(const uint64_t *m, const uint64_t *l, const int32_t *n, uint32_t lo, uint32_t hi, const Ts &t)
{
    return partition_point(lo, hi, [&](uint32_t i) { return cmp(ts_at(m, l, n, i), t) < 0; });
}
__device__ __forceinline__ uint32_t upper_bound_ts(const uint64_t *m, const uint64_t *l, const int32_t *n, uint32_t lo, uint32_t hi, const Ts &t)
{
    return partition_point(lo, hi, [&](uint32_t i) { return cmp(ts_at(m, l, n, i), t) <= 0; });
}

// last index i of off[0, n) with off[i] <= v: the one non-empty segment of the offsets off[0 .. n] that holds element v
// (off[0] <= v; 0 for n == 0). Its own loop: through partition_point it is an instruction longer per step.
template <class T>
__device__ __forceinline__ uint32_t seg_of(const T *off, uint32_t n, std::common_type_t<T> v)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (off[m] <= v) lo = m; else hi = m; }
    return lo;
}

// the index of v in the sorted, duplicate-free a[0, n), or NOT_FOUND: a key's slot in a resident store
constexpr uint32_t NOT_FOUND = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t find_sorted(const uint64_t *a, uint32_t n, uint64_t v)
{
    const uint32_t i = lower_bound(a, 0, n, v);
    return i < n && a[i] == v ? i : NOT_FOUND;
}

// 64-ary search by one wave: first index in [lo, hi) whose value is >= v (upper = false) or > v (upper = true).
// Each round is one parallel probe of 64 positions, so a 1M-entry class takes 4 dependent loads, not 20.
__device__ __forceinline__ uint32_t wave_search(const uint64_t *a, uint32_t lo, uint32_t hi, uint64_t v, bool upper)
{
    const uint32_t lane = lane_id();
    while (hi - lo > 64) {
        const uint32_t step = (hi - lo + 63) / 64;
        const uint32_t p = lo + lane * step;
        const bool below = p < hi && (upper ? a[p] <= v : a[p] < v);
        const uint32_t c = (uint32_t)__popcll(__ballot(below));
        if (c == 0) return lo;
        const uint32_t base = lo + (c - 1) * step;   // a[base] is below v, the answer is in (base, base + step]
        lo = base + 1;
        hi = min(base + step + 1, hi);
    }
    const uint32_t p = lo + lane;
    const bool below = p < hi && (upper ? a[p] <= v : a[p] < v);
    return lo + (uint32_t)__popcll(__ballot(below));
}

}  // namespace acc
