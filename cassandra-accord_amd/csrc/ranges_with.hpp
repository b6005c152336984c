// ranges_with.hpp — Ranges.with (AbstractRanges.union(MERGE_OVERLAPPING), primitives/AbstractRanges.java:439-585) once,
// for the host (ranges.hpp: acc_ranges_with, acc_ranges_contains_all) and for the device (rcmd.hip: the fold of a range
// command's updates). The algorithm is templated over how its two inputs are read and where its result goes:
//   In    size() and operator[](size_t) -> Rg, a sorted, deoverlapped Ranges;
//   Sink  push(Rg), appended to in order.
// Nothing here allocates, and the method is replayed step by step: with() has a superset short-cut and absorbs touching
// ranges only inside a group that a strict overlap opened, so it is no interval union and its result depends on the
// order of a fold.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ACC_RG_HD __host__ __device__ inline
#else
#define ACC_RG_HD inline
#endif

namespace acc {
namespace rg {

struct Rg {
    uint64_t s, e;
    bool operator==(const Rg &o) const { return s == o.s && e == o.e; }
};

ACC_RG_HD int cmpu(uint64_t a, uint64_t b) { return a < b ? -1 : a > b ? 1 : 0; }

// Range.compareIntersecting (Range.java:296-305)
ACC_RG_HD int cmp_intersecting(const Rg &a, const Rg &b)
{
    if (a.s >= b.e) return 1;
    if (a.e <= b.s) return -1;
    return 0;
}

// AbstractRanges.supersetLinearMerge (AbstractRanges.java:439-484): (ai, bi) = how far `as` covers a prefix of `bs`
template <class In>
ACC_RG_HD void superset_linear_merge_of(const In &as, const In &bs, size_t &ai_out, size_t &bi_out)
{
    size_t ai = 0, bi = 0;
    const size_t an = as.size(), bn = bs.size();
    while (ai < an && bi < bn) {
        Rg a = as[ai];
        const Rg b = bs[bi];
        int c = cmp_intersecting(a, b);
        if (c < 0) { ai++; continue; }
        if (c > 0) break;
        if (b.s < a.s) break;
        if ((c = cmpu(b.e, a.e)) <= 0) {
            bi++;
            if (c == 0) ai++;
            continue;
        }
        // a run of touching `as` ranges must reach b's end, else stop at the start of the run
        size_t t = ai;
        bool broke = false;
        do {
            if (++t == an) { broke = true; break; }
            const Rg nx = as[t];
            if (a.e != nx.s) { broke = true; break; }
            a = nx;
        } while (a.e < b.e);
        if (broke) break;
        bi++;
        ai = t;
    }
    ai_out = ai;
    bi_out = bi;
}

// where the result of with_of is: the left input itself, the right input itself (the method returns the object it was
// given), or the sink
enum WithResult { WITH_LEFT = 0, WITH_RIGHT = 1, WITH_SINK = 2 };

// AbstractRanges.union(MERGE_OVERLAPPING, left, right) (AbstractRanges.java:496-585) = Ranges.with (Ranges.java:119-127).
// The sink receives at most left.size() + right.size() ranges, and none unless WITH_SINK is returned.
template <class In, class Sink>
ACC_RG_HD WithResult with_of(const In &left, const In &right, Sink &out)
{
    if (right.size() == 0) return WITH_LEFT;
    if (left.size() == 0) return WITH_RIGHT;
    bool swapped = false;
    {
        const int c = cmpu(left[0].s, right[0].s);
        if (c > 0 || (c == 0 && left[left.size() - 1].e < right[right.size() - 1].e)) swapped = true;
    }
    const In &as = swapped ? right : left, &bs = swapped ? left : right;
    const size_t an = as.size(), bn = bs.size();
    size_t ai, bi;
    superset_linear_merge_of(as, bs, ai, bi);
    if (bi == bn) return swapped ? WITH_RIGHT : WITH_LEFT;
    for (size_t i = 0; i < ai; ++i) out.push(as[i]);
    while (ai < an && bi < bn) {
        const Rg a = as[ai], b = bs[bi];
        const int c = cmp_intersecting(a, b);
        if (c < 0) { out.push(a); ai++; }
        else if (c > 0) { out.push(b); bi++; }
        else {
            const uint64_t start = a.s <= b.s ? a.s : b.s;
            uint64_t end = a.e >= b.e ? a.e : b.e;
            ai++; bi++;
            while (ai < an || bi < bn) {
                bool from_a;
                if (ai == an) from_a = false;
                else if (bi == bn) from_a = true;
                else from_a = as[ai].s < bs[bi].s;
                const Rg mn = from_a ? as[ai] : bs[bi];
                if (mn.s > end) break;
                if (mn.e > end) end = mn.e;
                if (from_a) ai++; else bi++;
            }
            out.push(Rg{ start, end });
        }
    }
    while (ai < an) out.push(as[ai++]);
    while (bi < bn) out.push(bs[bi++]);
    return WITH_SINK;
}

}  // namespace rg
}  // namespace acc
