// CPU build of the element-wise first aggregation pass (k_cost_agg_flat, k_cost.hip): the per-pixel arithmetic is the device's own
// (adcensus_amd/csrc/k_cost_flat.h, compiled here with RR_EMUL, one disparity at a time); the walk around it restates the kernel --
// packed pixel records with marker-padded right rows (k_cost_records), the host-built tables (upload_tables, capi.hip), a workgroup's
// tile with the right columns it stages (clamped indices), a wave's 64 left / arm records with clamped columns picked by lane number,
// two disparities per lane and 128-float chunks.  Test infrastructure (tests/test_emul_cost_flat.py); shares no code with the oracle.
#define RR_EMUL
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>
#include <algorithm>
#include "../../adcensus_amd/csrc/k_cost_flat.h"

#define CF_PW 32
#define CF_HALO 16
#define CF_TX (4 * CF_PW)

struct Rec4 { uint32_t x, y, z, w; };

// vol: [H][W][Dp] floats (poisoned by the caller).  arms: the oracle's [H][W][4] = left, right, up, down.  cap: the depth the launch
// is made for (the longest horizontal arm or more).  Returns 0, or 1 when an index left what the kernel staged.
extern "C" int emul_cost_flat_launch(float* vol, const uint8_t* img_l, const uint8_t* img_r, const uint64_t* census_l,
                                     const uint64_t* census_r, const uint8_t* arms, int W, int H, int dmin, int D, int Dp, int cap,
                                     int lambda_ad, int lambda_census)
{
    if (Dp % 128 != 0 || D > Dp || cap < 0) return 2;
    // tables (upload_tables)
    float A[768], Ct[64];
    memset(A, 0, sizeof(A));
    for (int k = 0; k <= 765; k++) {
        const float cost_ad = (float)k / 3.0f;
        const float ea = expf(-cost_ad / (float)lambda_ad);
        A[k] = (1.0f - ea) + 1.0f;
    }
    for (int hm = 0; hm < 64; hm++) Ct[hm] = expf(-(float)hm / (float)lambda_census);
    // records (adc_create, k_cost_records)
    const int padl = (dmin + Dp - 1 > 0 ? dmin + Dp - 1 : 0) + 1;
    const int pitch = padl + W + (dmin < 0 ? -dmin : 0) + 1;
    std::vector<Rec4> rrec((size_t)H * pitch), lrec((size_t)H * W);
    std::vector<uint32_t> rec((size_t)H * W);
    for (int y = 0; y < H; y++) {
        for (int i = 0; i < pitch; i++) {
            const int c = i - padl;
            Rec4 r = {0xFFFFFFFFu, 0u, 0u, 0u};
            if (c >= 0 && c < W) {
                const size_t p = (size_t)y * W + c;
                r = {(uint32_t)img_r[3 * p] | ((uint32_t)img_r[3 * p + 1] << 8) | ((uint32_t)img_r[3 * p + 2] << 16), (uint32_t)census_r[p],
                     (uint32_t)(census_r[p] >> 32), 0u};
            }
            rrec[(size_t)y * pitch + i] = r;
        }
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            lrec[p] = {(uint32_t)img_l[3 * p] | ((uint32_t)img_l[3 * p + 1] << 8) | ((uint32_t)img_l[3 * p + 2] << 16), (uint32_t)census_l[p],
                       (uint32_t)(census_l[p] >> 32), 0u};
            rec[p] = (uint32_t)arms[p * 4] | ((uint32_t)arms[p * 4 + 1] << 8) | (1u << 16); // (the count is not read by this pass)
        }
    }
    int bad = 0;
    const int tiles = (W + CF_TX - 1) / CF_TX;
    const int n = CF_TX + Dp - 1 + 2 * cap;
    std::vector<uint32_t> sB(n), sC0(n), sC1(n);
    for (int blk = 0; blk < tiles * H; blk++) {
        const int y = blk / tiles, x0 = (blk - y * tiles) * CF_TX;
        const int col_lo = x0 - cap - dmin - (Dp - 1);
        const Rec4* rrow = rrec.data() + (size_t)y * pitch;
        for (int i = 0; i < n; i++) {
            int gi = padl + col_lo + i;
            gi = gi < 0 ? 0 : (gi >= pitch ? pitch - 1 : gi);
            sB[i] = rrow[gi].x; sC0[i] = rrow[gi].y; sC1[i] = rrow[gi].z;
        }
        for (int wave = 0; wave < 4; wave++) {
            const int xw = x0 + wave * CF_PW;
            if (xw >= W) continue;
            Rec4 lr[64];
            uint32_t myrec[64];
            for (int lane = 0; lane < 64; lane++) {
                const int xl = std::max(0, std::min(W - 1, xw - CF_HALO + lane));
                lr[lane] = lrec[(size_t)y * W + xl];
                myrec[lane] = rec[(size_t)y * W + xl];
            }
            const int npx = std::min(CF_PW, W - xw);
            for (int p = 0; p < npx; p++) {
                const int x = xw + p, li = CF_HALO + p;
                int lo, hi;
                cost_flat_arms(myrec[li], x, W, cap, &lo, &hi);
                auto left_at = [&](int t) -> CfRec {
                    if (li + t >= 0 && li + t < 64) return CfRec{lr[li + t].x, lr[li + t].y, lr[li + t].z};
                    if (x + t < 0 || x + t >= W) { bad = 1; return CfRec{0, 0, 0}; }
                    const Rec4 q = lrec[(size_t)y * W + x + t]; // (the device: a load of its own beyond the wave's window)
                    return CfRec{q.x, q.y, q.z};
                };
                for (int c = 0; c < Dp; c += 128)
                    for (int lane = 0; lane < 64; lane++)
                        for (int k = 0; k < 2; k++) { // (the device: both disparities of a lane in one call)
                            const int d = c + 2 * lane;
                            const int i0 = (x - x0) + cap + (Dp - 1) - d;
                            const bool pad[1] = {d + k >= D};
                            auto right_at = [&](int t, int) -> CfRec {
                                const int i = i0 + t - k;
                                if (i < 0 || i >= n) { bad = 1; return CfRec{0, 0, 0}; }
                                return CfRec{sB[i], sC0[i], sC1[i]};
                            };
                            float out[1];
                            if (D == Dp) cost_flat_span<1, false>(lo, hi, left_at, right_at, A, Ct, pad, out); // (the launcher's choice)
                            else cost_flat_span<1, true>(lo, hi, left_at, right_at, A, Ct, pad, out);
                            vol[((size_t)y * W + x) * Dp + d + k] = out[0];
                        }
            }
        }
    }
    return bad;
}
