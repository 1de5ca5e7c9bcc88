// CPU build of the gather form of the sparse small-ring aggregation launches: the per-pixel arithmetic is the device's own
// (adcensus_amd/csrc/k_agg_gather.h, compiled here with RR_EMUL and V = float, one disparity at a time); the walk around it restates
// k_agg_gather / k_agg_apply (k_aggregate.hip): waves of 64 consecutive records of the direction's line-major record set, the
// launch's predicate, the 64-record window around a changed pixel with clamped indices, records clipped to the line, stores into the
// OTHER volume and the copy back.  Test infrastructure (tests/test_emul_gather.py); shares no code with the oracle.
#define RR_EMUL
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>
#include <algorithm>
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
#include "../../adcensus_amd/csrc/adc_device_fn.h"
#include "../../adcensus_amd/csrc/k_agg_gather.h"

template <bool DIVIDE, bool PAIR>
static long gather_launch(const float* src, float* dst, const uint32_t* rec, int W, int H, int D, bool vert)
{
    const long long P = (long long)W * H;
    const int N = vert ? H : W;
    const long long fstep = (vert ? (long long)W : 1LL) * D;
    long changed = 0;
    for (long long i0 = 0; i0 < P; i0 += 64) { // one wave
        uint32_t mine[64];
        unsigned long long todo = 0;
        for (int lane = 0; lane < 64; lane++) {
            const long long i = i0 + lane;
            mine[lane] = rec[i < P ? i : 0];
            if (i < P && adc_rec_changes_pixel(mine[lane], DIVIDE || PAIR)) todo |= 1ull << lane;
        }
        while (todo) {
            const int b = __builtin_ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const long long r = i0 + b;
            const long long line = r / N;
            const int s = (int)(r - line * N);
            auto clip = [&](uint32_t q, int pos) -> uint32_t {
                const uint32_t lo = std::min((int)(q & 255u), pos), hi = std::min((int)((q >> 8) & 255u), N - 1 - pos);
                return (q & 0xFFFF0000u) | (hi << 8) | lo;
            };
            const uint32_t rs = clip(mine[b], s);
            uint32_t win[64];
            for (int lane = 0; lane < 64; lane++) {
                const long long wi = r - 32 + lane;
                win[lane] = rec[wi < 0 ? 0 : (wi >= P ? P - 1 : wi)];
            }
            auto rec_at = [&](int t) -> uint32_t {
                if (t >= -32 && t < 32) return clip(win[t + 32], s + t);
                return clip(rec[r + t], s + t);
            };
            const long long pix = vert ? (long long)s * W + line : r;
            for (int d = 0; d < D; d++) // (the device: two disparities per lane, Dp / 128 chunks per pixel)
                dst[pix * D + d] = agg_gather_pixel<float, DIVIDE, PAIR>(src + pix * D + d, fstep, rs, rec_at);
            changed++;
        }
    }
    return changed;
}

// k_agg_apply: the stored pixels go back into the volume the launch read
static void apply_launch(const float* from, float* to, const uint32_t* rec, int W, int H, int D, bool vert, bool divide)
{
    const long long P = (long long)W * H;
    for (long long r = 0; r < P; r++) {
        if (!adc_rec_changes_pixel(rec[r], divide)) continue;
        const long long pix = vert ? (r % H) * W + r / H : r;
        memcpy(to + pix * D, from + pix * D, sizeof(float) * D);
    }
}

// One sparse launch in its gather form + k_agg_apply.  vol: [H][W][D] floats, holds the input and then the result; other: the second
// volume (poisoned here: nothing the launch did not store may be copied back).  `sup` = the divisor map of the direction's dividing
// pass (the count field of its records, as k_make_records packs them).  Returns the number of pixels the launch computed.
extern "C" long emul_gather_launch(float* vol, float* other, const uint8_t* arms, const uint16_t* sup, int W, int H, int D, int vert,
                                   int divide, int pair)
{
    const size_t P = (size_t)W * H;
    std::vector<uint32_t> rec(P);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            const uint8_t* a = arms + p * 4;
            if (vert) rec[(size_t)x * H + y] = (uint32_t)a[2] | ((uint32_t)a[3] << 8) | ((uint32_t)sup[p] << 16);
            else rec[p] = (uint32_t)a[0] | ((uint32_t)a[1] << 8) | ((uint32_t)sup[p] << 16);
        }
    for (size_t k = 0; k < P * D; k++) other[k] = NAN;
    long n;
    if (pair) n = gather_launch<true, true>(vol, other, rec.data(), W, H, D, vert != 0);
    else if (divide) n = gather_launch<true, false>(vol, other, rec.data(), W, H, D, vert != 0);
    else n = gather_launch<false, false>(vol, other, rec.data(), W, H, D, vert != 0);
    apply_launch(other, vol, rec.data(), W, H, D, vert != 0, divide || pair);
    return n;
}
