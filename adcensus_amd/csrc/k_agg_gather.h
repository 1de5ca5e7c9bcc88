// k_agg_gather.h -- the per-pixel arithmetic of the GATHER form of the sparse small-ring aggregation launches (k_agg_gather,
// k_aggregate.hip).  A sparse launch changes only the pixels whose own record makes a pass change them (adc_rec_changes_pixel);
// the gather form computes exactly those, each from the input vectors inside its own arm span (a pass pair: inside the arm spans
// of the pixels of its span), instead of marching over the whole volume.  Same sums as the marching form (AGG_EMIT / AGG_EMIT2,
// cross_aggregator.cpp:327-394): every value is the sequential f32 sum from +0.0f in the order -arm .. +arm, the dividing pass
// divided by the support count with plain IEEE division (x / 1 is skipped, as there); no sliding sums, no reassociation.
//
// Compiled a second time for the CPU with RR_EMUL defined (tests/emul/emul_gather.cpp, V = float, one disparity at a time).
#pragma once

#ifndef RR_EMUL
#define GG_FN __device__ __forceinline__
#else
#include <cstdint>
#define GG_FN static inline
#endif

#define GG_BATCH 4 // loads of a span issued together (indices past the span repeat its last entry and are not added)

// First-pass value of the element whose vector starts at pq, from its own record rq = {lo, hi << 8, count << 16}; neighbouring
// elements of the line lie fstep floats apart.
template <typename V, bool DIVIDE>
GG_FN V agg_gather_first(const float* pq, long long fstep, uint32_t rq)
{
    const int lo = (int)(rq & 255u), hi = (int)((rq >> 8) & 255u);
    V acc = (V)(0.0f);
    for (int u = -lo; u <= hi; u += GG_BATCH) {
        V v[GG_BATCH];
#pragma unroll
        for (int k = 0; k < GG_BATCH; k++) v[k] = *reinterpret_cast<const V*>(pq + (long long)(u + k < hi ? u + k : hi) * fstep);
#pragma unroll
        for (int k = 0; k < GG_BATCH; k++)
            if (u + k <= hi) acc = acc + v[k];
    }
    if (DIVIDE) {
        const uint32_t c = rq >> 16;
        if (c != 1u) acc = acc / (float)c;
    }
    return acc;
}

// Output of a launch at the changed pixel whose input vector starts at ps and whose record is rs.  Single pass: its first-pass value.
// PAIR (dividing pass + the following non-dividing pass along the same line): the ordered sum over the pixel's own span of the
// first-pass values of the span's pixels, each with ITS record -- rec_at(t) = record of the pixel t places along the line.
template <typename V, bool DIVIDE, bool PAIR, class RecAt>
GG_FN V agg_gather_pixel(const float* ps, long long fstep, uint32_t rs, RecAt rec_at)
{
    if constexpr (!PAIR) return agg_gather_first<V, DIVIDE>(ps, fstep, rs);
    const int lo = (int)(rs & 255u), hi = (int)((rs >> 8) & 255u);
    V acc2 = (V)(0.0f);
    for (int t = -lo; t <= hi; t++) acc2 = acc2 + agg_gather_first<V, true>(ps + (long long)t * fstep, fstep, t == 0 ? rs : rec_at(t));
    return acc2;
}
