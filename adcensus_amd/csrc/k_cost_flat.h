// k_cost_flat.h -- the per-pixel arithmetic of k_cost_agg_flat (k_cost.hip): the FIRST aggregation pass of the short-arm plan
// (horizontal, non-dividing, matching cost computed inside the pass) as an element-wise kernel.  An output is the ordered f32 sum
// from +0.0f over t = -arm_lo .. +arm_hi of the matching cost of (x + t, y, d) (cross_aggregator.cpp:327-394 over
// cost_computor.cpp:82-121) -- the sum k_agg_march<.., COSTIN> forms by marching; on a short-arm image the span is {x} for almost
// every pixel, so the flat form evaluates each span where it stands: no ring, no window, no hand-counted wait.  The cost expression
// is AGG_COST's (k_aggregate.hip), bit for bit: v_sad_u8 of the packed colours, two popcounts of the census xor,
// A[min(ad, 765)] - C[hm & 63], 1.0f for the out-of-image marker, 0.0f in padding lanes.
//
// Compiled a second time for the CPU with RR_EMUL defined (tests/emul/emul_cost_flat.cpp, one disparity at a time).
#pragma once

#ifndef RR_EMUL
#define CF_FN __device__ __forceinline__
#define CF_SAD_U8(A, B) __builtin_amdgcn_sad_u8((A), (B), 0u)
#define CF_POPC(X) ((uint32_t)__popc(X))
#else
#include <cstdint>
#define CF_FN static inline
static inline uint32_t cf_sad_u8(uint32_t a, uint32_t b) // v_sad_u8 with a zero accumulator: sum of the four byte differences
{
    uint32_t s = 0;
    for (int k = 0; k < 4; k++) {
        const int x = (int)((a >> (8 * k)) & 255u), y = (int)((b >> (8 * k)) & 255u);
        s += (uint32_t)(x > y ? x - y : y - x);
    }
    return s;
}
#define CF_SAD_U8(A, B) cf_sad_u8((A), (B))
#define CF_POPC(X) ((uint32_t)__builtin_popcount(X))
#endif

#define CF_MARKER 0xFFFFFFFFu // bgrx of a right-image column outside the image (k_cost_records)

struct CfRec { uint32_t b, c0, c1; }; // a pixel record {B | G<<8 | R<<16, census lo, census hi}

// matching cost of a left pixel against a right pixel; `pad`: the disparity lies beyond the range (d >= D)
CF_FN float cost_flat_term(const CfRec& r, const CfRec& l, const float* lutA, const float* lutC, bool pad)
{
    const uint32_t ad = CF_SAD_U8(r.b, l.b);
    const uint32_t hm = CF_POPC(r.c0 ^ l.c0) + CF_POPC(r.c1 ^ l.c1);
    float cv = lutA[ad < 766u ? ad : 765u] - lutC[hm & 63u]; // == ((1 - ea) + 1) - ec, cost_computor.cpp:117
    cv = r.b == CF_MARKER ? 1.0f : cv;                        // right pixel outside the image (:101-104)
    return pad ? 0.0f : cv;
}

// The arms of a horizontal record {lo, hi << 8, ..} of column x as the pass may use them: clipped at the row's ends (as k_agg_gather
// clips: changes no valid record) and at `cap`, the longest arm the launch was made for (the gate lets no image with a longer one
// through; the cap keeps every read of a damaged record inside what the launch staged).
CF_FN void cost_flat_arms(uint32_t rec, int x, int W, int cap, int* lo, int* hi)
{
    const int a = (int)(rec & 255u), b = (int)((rec >> 8) & 255u);
    const int la = a < x ? a : x, hb = b < W - 1 - x ? b : W - 1 - x;
    *lo = la < cap ? la : cap;
    *hi = hb < cap ? hb : cap;
}

// out[k] = the pass's value for NV disparities of one pixel: left_at(t) = record of the left pixel t columns along the row,
// right_at(t, k) = record of the right pixel that disparity k of the left pixel x + t is matched against.
// Arms 0 / 0 (almost every pixel of a short-arm image): the value is the pixel's own cost c, without the addition -- exact, because
// 0.0f + c differs from c only for c == -0.0f, and c is 1.0f, 0.0f or a difference A - C of two table entries that are never -0.0f
// (in round-to-nearest x - y is -0.0f only for x == -0.0f).  PAD = false: the caller knows that no disparity lies beyond the range.
template <int NV, bool PAD, class LeftAt, class RightAt>
CF_FN void cost_flat_span(int lo, int hi, LeftAt left_at, RightAt right_at, const float* lutA, const float* lutC, const bool* pad,
                          float* out)
{
    if (lo == 0 && hi == 0) {
        const CfRec l = left_at(0);
        for (int k = 0; k < NV; k++) out[k] = cost_flat_term(right_at(0, k), l, lutA, lutC, PAD && pad[k]);
        return;
    }
    float acc[NV];
    for (int k = 0; k < NV; k++) acc[k] = 0.0f;
    for (int t = -lo; t <= hi; t++) {
        const CfRec l = left_at(t);
        for (int k = 0; k < NV; k++) acc[k] = acc[k] + cost_flat_term(right_at(t, k), l, lutA, lutC, PAD && pad[k]);
    }
    for (int k = 0; k < NV; k++) out[k] = acc[k];
}
