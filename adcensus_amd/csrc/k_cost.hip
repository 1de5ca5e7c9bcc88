// k_cost.hip -- K1 gray + 9x7 census, K2 AD-census cost volume.
//
// Replaces CostComputor::{ComputeGray, CensusTransform, ComputeCost} (cost_computor.cpp:58-121)
// and adcensus_util::{census_transform_9x7, Hamming64} (adcensus_util.cpp:10-53).
//
// K2 is a pure streaming write of the volume (algorithmic bytes: V = 4*W*H*Dp written once,
// inputs 2*(3+8)*W*H): lanes = disparities, one wave-store of Dp floats per pixel (256/512/1024 B
// contiguous), the right image row segment and its census strings staged in LDS, the two
// exponentials replaced by host-built tables (A[766], C[64]) so the result is bit-identical to
// glibc expf on the host.
#include "adc_internal.h"
#include "adc_device_fn.h"
#include "k_aggregate_rr.h"  // agg_gate_skip
#include "k_aggregate_rr2.h" // AggCostIn
#include "k_cost_flat.h"

// ------------------------------------------------------------------------------------------- K1
#define CT_W 32
#define CT_H 8
#define CT_LW (CT_W + 6)
#define CT_LH (CT_H + 8)

__global__ __launch_bounds__(CT_W* CT_H) void k_gray_census(const uint8_t* __restrict__ img_l,
                                                             const uint8_t* __restrict__ img_r,
                                                             uint8_t* __restrict__ gray_l, uint8_t* __restrict__ gray_r,
                                                             uint64_t* __restrict__ census_l,
                                                             uint64_t* __restrict__ census_r, int W, int H, int census5)
{
    __shared__ uint8_t tile[CT_LH][CT_LW + 2];
    const uint8_t* img = blockIdx.z == 0 ? img_l : img_r;
    uint8_t* gray = blockIdx.z == 0 ? gray_l : gray_r;
    uint64_t* census = blockIdx.z == 0 ? census_l : census_r;
    const int x0 = blockIdx.x * CT_W, y0 = blockIdx.y * CT_H;
    const int tid = threadIdx.y * CT_W + threadIdx.x;
    for (int i = tid; i < CT_LH * CT_LW; i += CT_W * CT_H) {
        const int ly = i / CT_LW, lx = i % CT_LW;
        const int gx = x0 + lx - 3, gy = y0 + ly - 4;
        uint8_t g = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const uint8_t* p = img + ((size_t)gy * W + gx) * 3;
            g = adc_gray(p[0], p[1], p[2]);
        }
        tile[ly][lx] = g;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int lx = threadIdx.x + 3, ly = threadIdx.y + 4;
    const uint8_t c = tile[ly][lx];
    gray[(size_t)y * W + x] = c;
    uint64_t v = 0;
    // interior only, whole transform skipped for tiny images (adcensus_util.cpp:12,17-18); others stay 0
    if (census5) { // opt-in paper mode (k_paper.hip): 5x5 window, same conventions -- 25 bits, MSB first, interior only
        if (W > 5 && H > 5 && y >= 2 && y < H - 2 && x >= 2 && x < W - 2) {
#pragma unroll
            for (int r = -2; r <= 2; r++)
#pragma unroll
                for (int cc = -2; cc <= 2; cc++) {
                    v <<= 1;
                    v += (tile[ly + r][lx + cc] < c) ? 1u : 0u;
                }
        }
    } else if (W > 9 && H > 7 && y >= 4 && y < H - 4 && x >= 3 && x < W - 3) {
#pragma unroll
        for (int r = -4; r <= 4; r++)
#pragma unroll
            for (int cc = -3; cc <= 3; cc++) {
                v <<= 1;
                v += (tile[ly + r][lx + cc] < c) ? 1u : 0u;
            }
    }
    census[(size_t)y * W + x] = v;
}

hipError_t adc_launch_gray_census(adc_handle* h)
{
    const AdcParams& p = h->p;
    dim3 grid((p.W + CT_W - 1) / CT_W, (p.H + CT_H - 1) / CT_H, 2), block(CT_W, CT_H, 1);
    hipLaunchKernelGGL(k_gray_census, grid, block, 0, h->heavy, h->img_l, h->img_r, h->gray_l, h->gray_r, h->census_l,
                       h->census_r, p.W, p.H, (h->paper & ADC_PAPER_CENSUS5X5) ? 1 : 0);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------- K1, pipeline form
// One pass over both images (grid z = image) in place of k_gray_census, k_pack_bgr, k_color_diffs and k_cost_records: a workgroup
// loads its tile plus the census halo as packed B | G<<8 | R<<16 into LDS once, derives the gray tile from it (adc_gray, the unfused
// f64 form) and writes per pixel the gray value, the 9x7 census (same interior rule, same skip for W <= 9 or H <= 7), the colour
// steps dh / dv against the left / upper neighbour in the tile (0 at x = 0 / y = 0), the cost record {bgr, census lo, census hi, 0}
// and -- left image -- the packed pixel.  The marker columns of the right records are not written here: they never change for a
// handle (k_rrec_markers, once behind the allocation).  Same values in the same buffers as the four kernels.
__global__ __launch_bounds__(CT_W* CT_H) void k_front(const uint8_t* __restrict__ img_l, const uint8_t* __restrict__ img_r,
                                                       uint8_t* __restrict__ gray_l, uint8_t* __restrict__ gray_r,
                                                       uint64_t* __restrict__ census_l, uint64_t* __restrict__ census_r,
                                                       uint32_t* __restrict__ bgrx_l, uint8_t* __restrict__ lh, uint8_t* __restrict__ lv,
                                                       uint8_t* __restrict__ rh, uint8_t* __restrict__ rv, uint4* __restrict__ lrec,
                                                       uint4* __restrict__ rrec, int W, int H, int pitch, int padl)
{
    __shared__ uint8_t tile[CT_LH][CT_LW + 2];
    __shared__ uint32_t sbgr[CT_LH][CT_LW];
    const bool left = blockIdx.z == 0;
    const uint8_t* img = left ? img_l : img_r;
    const int x0 = blockIdx.x * CT_W, y0 = blockIdx.y * CT_H;
    const int tid = threadIdx.y * CT_W + threadIdx.x;
    for (int i = tid; i < CT_LH * CT_LW; i += CT_W * CT_H) {
        const int ly = i / CT_LW, lx = i % CT_LW;
        const int gx = x0 + lx - 3, gy = y0 + ly - 4;
        uint8_t g = 0;
        uint32_t c = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const uint8_t* p = img + ((size_t)gy * W + gx) * 3;
            c = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
            g = adc_gray(p[0], p[1], p[2]);
        }
        tile[ly][lx] = g;
        sbgr[ly][lx] = c;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int lx = threadIdx.x + 3, ly = threadIdx.y + 4;
    const size_t p = (size_t)y * W + x;
    const uint8_t c = tile[ly][lx];
    (left ? gray_l : gray_r)[p] = c;
    uint64_t v = 0;
    if (W > 9 && H > 7 && y >= 4 && y < H - 4 && x >= 3 && x < W - 3) { // interior only (adcensus_util.cpp:12,17-18); others stay 0
#pragma unroll
        for (int r = -4; r <= 4; r++)
#pragma unroll
            for (int cc = -3; cc <= 3; cc++) {
                v <<= 1;
                v += (tile[ly + r][lx + cc] < c) ? 1u : 0u;
            }
    }
    (left ? census_l : census_r)[p] = v;
    const uint32_t me = sbgr[ly][lx];
    (left ? lh : rh)[p] = x > 0 ? (uint8_t)adc_color_dist_max_u32(me, sbgr[ly][lx - 1]) : 0;
    (left ? lv : rv)[p] = y > 0 ? (uint8_t)adc_color_dist_max_u32(me, sbgr[ly - 1][lx]) : 0;
    const uint4 rec = make_uint4(me, (uint32_t)v, (uint32_t)(v >> 32), 0u);
    if (left) {
        bgrx_l[p] = me;
        lrec[p] = rec;
    } else {
        rrec[(size_t)y * pitch + padl + x] = rec;
    }
}

hipError_t adc_launch_front(adc_handle* h)
{
    const AdcParams& p = h->p;
    dim3 grid((p.W + CT_W - 1) / CT_W, (p.H + CT_H - 1) / CT_H, 2), block(CT_W, CT_H, 1);
    hipLaunchKernelGGL(k_front, grid, block, 0, h->heavy, h->img_l, h->img_r, h->gray_l, h->gray_r, h->census_l, h->census_r, h->bgrx_l,
                       h->cdiff_lh, h->cdiff_lv, h->cdiff_rh, h->cdiff_rv, reinterpret_cast<uint4*>(h->cost_lrec),
                       reinterpret_cast<uint4*>(h->cost_rrec), p.W, p.H, h->rrec_pitch, h->rrec_padl);
    h->bgrx_valid = 1;
    return hipGetLastError();
}

// The out-of-image marker columns of the right records (cost_computor.cpp:101-104: bgrx = 0xFFFFFFFF -> cost 1.0), padl to the left
// of a row and pitch - padl - W to its right.  A handle's geometry is fixed, so they are written once, behind the allocation
// (k_cost_records rewrites them with every launch; k_front leaves them alone).
__global__ __launch_bounds__(256) void k_rrec_markers(uint4* __restrict__ rrec, int W, int H, int pitch, int padl)
{
    const int y = blockIdx.y;
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pitch - W) return;
    if (i >= padl) i += W;
    rrec[(size_t)y * pitch + i] = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
}
hipError_t adc_launch_rrec_markers(adc_handle* h)
{
    const AdcParams& p = h->p;
    hipLaunchKernelGGL(k_rrec_markers, dim3((h->rrec_pitch - p.W + 255) / 256, p.H), dim3(256), 0, h->stream, reinterpret_cast<uint4*>(h->cost_rrec),
                       p.W, p.H, h->rrec_pitch, h->rrec_padl);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------- K2
#define COST_TX 32          // pixels of one row per block
#define COST_MAXSEG (COST_TX + ADC_MAX_DISP_RANGE)

template <int VPL>
__global__ __launch_bounds__(256) void k_cost(const uint8_t* __restrict__ img_l, const uint8_t* __restrict__ img_r,
                                              const uint64_t* __restrict__ census_l,
                                              const uint64_t* __restrict__ census_r, const float* __restrict__ lut_ad,
                                              const float* __restrict__ lut_census, float* __restrict__ vol, int W,
                                              int H, int dmin, int D)
{
    constexpr int Dp = 64 * VPL;
    __shared__ float sA[768];
    __shared__ float sC[64];
    __shared__ uint32_t sBgr[COST_MAXSEG];
    __shared__ uint64_t sCen[COST_MAXSEG];

    const int y = blockIdx.y;
    const int x0 = blockIdx.x * COST_TX;
    const int tid = threadIdx.x;
    for (int i = tid; i < 766; i += 256) sA[i] = lut_ad[i];
    if (tid < 64) sC[tid] = lut_census[tid];
    // right-image columns needed: xr = x - d, x in [x0, x0+TX), d in [dmin, dmin+D)
    const int xr_lo = x0 - (dmin + D - 1);
    const int nseg = COST_TX + D - 1;
    for (int i = tid; i < nseg; i += 256) {
        const int xr = xr_lo + i;
        uint32_t c = 0xFFFFFFFFu; // out-of-image marker (cost_computor.cpp:101-104)
        uint64_t cs = 0;
        if (xr >= 0 && xr < W) {
            const uint8_t* pr = img_r + ((size_t)y * W + xr) * 3;
            c = (uint32_t)pr[0] | ((uint32_t)pr[1] << 8) | ((uint32_t)pr[2] << 16);
            cs = census_r[(size_t)y * W + xr];
        }
        sBgr[i] = c;
        sCen[i] = cs;
    }
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    for (int px = wave; px < COST_TX; px += 4) {
        const int x = x0 + px;
        if (x >= W) break;
        const uint8_t* pl = img_l + ((size_t)y * W + x) * 3;
        const int bl = pl[0], gl = pl[1], rl = pl[2];
        const uint64_t cl = census_l[(size_t)y * W + x];
        float out[VPL];
#pragma unroll
        for (int k = 0; k < VPL; k++) {
            const int di = lane * VPL + k;
            float c = 0.0f; // padding
            if (di < D) {
                const int xr = x - (di + dmin);
                const uint32_t pr = sBgr[xr - xr_lo];
                if (pr == 0xFFFFFFFFu) {
                    c = 1.0f;
                } else {
                    const int ad = adc_iabs(bl - (int)(pr & 255u)) + adc_iabs(gl - (int)((pr >> 8) & 255u)) +
                                   adc_iabs(rl - (int)((pr >> 16) & 255u));
                    const int hm = __popcll(cl ^ sCen[xr - xr_lo]);
                    c = sA[ad] - sC[hm]; // == ((1 - ea) + 1) - ec, cost_computor.cpp:117
                }
            }
            out[k] = c;
        }
        float* dst = vol + ((size_t)y * W + x) * Dp + lane * VPL;
        if constexpr (VPL == 1) dst[0] = out[0];
        else if constexpr (VPL == 2) *reinterpret_cast<float2*>(dst) = make_float2(out[0], out[1]);
        else {
#pragma unroll
            for (int q = 0; q < VPL; q += 4) *reinterpret_cast<float4*>(dst + q) = make_float4(out[q], out[q + 1], out[q + 2], out[q + 3]);
        }
    }
}

hipError_t adc_launch_cost(adc_handle* h, float* vol_out)
{
    const AdcParams& p = h->p;
    dim3 grid((p.W + COST_TX - 1) / COST_TX, p.H, 1), block(256, 1, 1);
#define LAUNCH(V)                                                                                                     \
    hipLaunchKernelGGL(k_cost<V>, grid, block, 0, h->heavy, h->img_l, h->img_r, h->census_l, h->census_r, h->lut_ad, \
                       h->lut_census, vol_out, p.W, p.H, p.dmin, p.D)
    if (p.VPL == 1) LAUNCH(1);
    else if (p.VPL == 2) LAUNCH(2);
    else if (p.VPL == 4) LAUNCH(4);
    else if (p.VPL == 8) LAUNCH(8);
    else if (p.VPL == 16) LAUNCH(16);
    else LAUNCH(32);
#undef LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------- packed pixel records (fused cost)
// Inputs of the cost computation that is fused into the first aggregation pass (k_agg_march<.., COSTIN>):
// per pixel {B | G<<8 | R<<16, census lo, census hi, 0}.  The right-image rows are padded on both sides with
// out-of-image markers (bgrx = 0xFFFFFFFF -> cost 1.0, cost_computor.cpp:101-104), so the marching kernel needs
// no bounds logic: row pitch = padl + W + padr.
__global__ __launch_bounds__(256) void k_cost_records(const uint8_t* __restrict__ img_l, const uint8_t* __restrict__ img_r,
                                                      const uint64_t* __restrict__ census_l,
                                                      const uint64_t* __restrict__ census_r, uint4* __restrict__ lrec,
                                                      uint4* __restrict__ rrec, int W, int H, int pitch, int padl)
{
    const int y = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < pitch) {
        const int c = i - padl;
        uint4 r = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
        if (c >= 0 && c < W) {
            const size_t p = (size_t)y * W + c;
            const uint64_t cs = census_r[p];
            r = make_uint4((uint32_t)img_r[3 * p] | ((uint32_t)img_r[3 * p + 1] << 8) | ((uint32_t)img_r[3 * p + 2] << 16),
                           (uint32_t)cs, (uint32_t)(cs >> 32), 0u);
        }
        rrec[(size_t)y * pitch + i] = r;
    }
    if (i < W) {
        const size_t p = (size_t)y * W + i;
        const uint64_t cs = census_l[p];
        lrec[p] = make_uint4((uint32_t)img_l[3 * p] | ((uint32_t)img_l[3 * p + 1] << 8) | ((uint32_t)img_l[3 * p + 2] << 16),
                             (uint32_t)cs, (uint32_t)(cs >> 32), 0u);
    }
}

hipError_t adc_launch_cost_records(adc_handle* h)
{
    const AdcParams& p = h->p;
    hipLaunchKernelGGL(k_cost_records, dim3((h->rrec_pitch + 255) / 256, p.H), dim3(256), 0, h->heavy, h->img_l, h->img_r,
                       h->census_l, h->census_r, reinterpret_cast<uint4*>(h->cost_lrec), reinterpret_cast<uint4*>(h->cost_rrec),
                       p.W, p.H, h->rrec_pitch, h->rrec_padl);
    return hipGetLastError();
}

// ------------------------------------------------- first aggregation pass of the short-arm plan, element-wise
// k_cost_agg_flat runs in place of k_agg_march<false, false, true, true, false, 1> (small ring, fused cost) and writes the same
// volume: per element the ordered f32 sum from 0.0f over the pixel's own horizontal span of the matching costs (k_cost_flat.h).  On a
// short-arm image that span is the pixel itself for ~99 % of the pixels, and the march pays its ring, its DPP window and its slot
// bookkeeping for nothing; here a span is evaluated where it stands.
//   * a workgroup of 4 waves owns CF_TX consecutive pixels of one row and stages, in LDS, the right records of every column its
//     spans can reach (tile - dmin - Dp + 1 - cap .. tile + cap: the padded rows of k_cost_records need no bounds logic, indices
//     beyond the pitch repeat a marker column) and the two tables;
//   * a wave owns CF_PW of those pixels: lane l holds the left record and the arm record of column first - CF_HALO + l (one
//     coalesced load per wave), and every pixel picks what its span needs with v_readlane -- wave-uniform, like the loop over the span;
//   * a lane holds disparities 2 * lane and 2 * lane + 1 of each 128-float chunk (the layout of the VPL = 2 kernels): one 8-byte
//     store per lane, 512 contiguous bytes per wave.
// Keeps the gate of the march it replaces (agg_gate_skip with the same arguments): it skips, and raises the too-shallow flag, exactly
// when that march would.  cap = the ring depth the march would have had; no valid record of an image that passes the gate has a
// longer arm.  The arithmetic holds for any arm length (arms beyond CF_HALO cost a load of their own per span entry).
#define CF_PW 32
#define CF_HALO 16
#define CF_TX (4 * CF_PW)
#define CF_LDS_MAX (48 * 1024)
static_assert(CF_TX == LEARN_CF_TX && CF_LDS_MAX == LEARN_CF_LDS_MAX, "learn_plan.h states the LDS footprint of k_cost_agg_flat");
typedef float cf_f2 __attribute__((ext_vector_type(2)));

template <bool PAD> // PAD = false: D == Dp, no padding lanes
__global__ __launch_bounds__(256) void k_cost_agg_flat(float* __restrict__ dst, const uint32_t* __restrict__ rec, int W, int H, int Dp,
                                                       int cap, int tiles, const int* __restrict__ armmax, int small_variant,
                                                       int small_L, AggCostIn ci)
{
    if (agg_gate_skip(armmax, small_variant, small_L, false)) return;
    extern __shared__ __attribute__((aligned(16))) uint32_t cf_lds[];
    const int n = CF_TX + Dp - 1 + 2 * cap; // staged right columns
    float* lutA = reinterpret_cast<float*>(cf_lds);
    float* lutC = lutA + 768;
    uint32_t* sB = cf_lds + 768 + 64;
    uint32_t* sC0 = sB + n;
    uint32_t* sC1 = sC0 + n;
    const int tid = threadIdx.x;
    const int y = (int)blockIdx.x / tiles;
    const int x0 = ((int)blockIdx.x - y * tiles) * CF_TX;
    for (int i = tid; i < 766; i += 256) lutA[i] = ci.lut_ad[i];
    if (tid < 64) lutC[tid] = ci.lut_census[tid];
    // staged entry i = right column col_lo + i; disparity index d of pixel x + t is matched against column x + t - dmin - d
    const int col_lo = x0 - cap - ci.dmin - (Dp - 1);
    const uint4* rrow = ci.rrec + (size_t)y * ci.rpitch;
    for (int i = tid; i < n; i += 256) {
        int gi = ci.padl + col_lo + i;
        gi = gi < 0 ? 0 : (gi >= ci.rpitch ? ci.rpitch - 1 : gi); // (both ends of a padded row are marker columns; no pixel of the image needs a clamped one)
        const uint4 r = rrow[gi];
        sB[i] = r.x;
        sC0[i] = r.y;
        sC1[i] = r.z;
    }
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int xw = x0 + wave * CF_PW; // first pixel of this wave
    if (xw >= W) return;
    const int xl = adc_imax(0, adc_imin(W - 1, xw - CF_HALO + lane));
    const uint4 lr = ci.lrec[(size_t)y * W + xl];
    const uint32_t myrec = rec[(size_t)y * W + xl];
    const int npx = adc_imin(CF_PW, W - xw);
    // staged entry of (pixel, t = 0, chunk 0, first disparity of the lane) = (x - x0) + cap + (Dp - 1) - 2 * lane, in [cap + 1, n - 1 - cap];
    // entry + t - c - k is what disparity c + 2 * lane + k of pixel x + t is matched against
    const uint32_t* qB = sB + (xw - x0) + cap + (Dp - 1) - 2 * lane;
    const uint32_t* qC0 = qB + n;
    const uint32_t* qC1 = qC0 + n;
    float* pd = dst + ((size_t)y * W + xw) * Dp + 2 * lane;
    for (int p = 0; p < npx; p++, qB++, qC0++, qC1++, pd += Dp) {
        const int li = CF_HALO + p; // the lane that holds column x
        const uint32_t rq = (uint32_t)__builtin_amdgcn_readlane((int)myrec, li);
        auto left_at = [&](int t) -> CfRec { // (x + t lies inside the row: t comes from the clipped span of x)
            CfRec l;
            if (li + t >= 0 && li + t < 64) {
                l.b = (uint32_t)__builtin_amdgcn_readlane((int)lr.x, li + t);
                l.c0 = (uint32_t)__builtin_amdgcn_readlane((int)lr.y, li + t);
                l.c1 = (uint32_t)__builtin_amdgcn_readlane((int)lr.z, li + t);
            } else { // arms beyond the wave's window -- never with the small ring -- fall back to a load of their own
                const uint4 q = ci.lrec[(size_t)y * W + xw + p + t];
                l.b = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.x);
                l.c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.y);
                l.c1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.z);
            }
            return l;
        };
        int lo = 0, hi = 0;
        const bool single = (rq & 0xFFFFu) == 0u; // arms 0 / 0 (the clip changes no zero): the straight-line form of cost_flat_span
        if (!single) cost_flat_arms(rq, xw + p, W, cap, &lo, &hi);
        for (int c = 0; c < Dp; c += 128) {
            const bool pad[2] = {c + 2 * lane >= ci.D, c + 2 * lane + 1 >= ci.D};
            auto right_at = [&](int t, int k) -> CfRec {
                CfRec r;
                r.b = qB[t - c - k];
                r.c0 = qC0[t - c - k];
                r.c1 = qC1[t - c - k];
                return r;
            };
            float out[2];
            if (single) cost_flat_span<2, PAD>(0, 0, left_at, right_at, lutA, lutC, pad, out);
            else cost_flat_span<2, PAD>(lo, hi, left_at, right_at, lutA, lutC, pad, out);
            cf_f2 v;
            v.x = out[0];
            v.y = out[1];
            ADC_VOL_STORE(reinterpret_cast<cf_f2*>(pd + c), v);
        }
    }
}

static size_t cost_agg_flat_lds(const adc_handle* h, int cap)
{
    return learn_cost_flat_lds(h->p.Dp, cap);
}
bool adc_cost_agg_flat_fits(const adc_handle* h, int cap)
{
    return learn_cost_flat_fits(h->p.Dp, cap);
}
hipError_t adc_launch_cost_agg_flat(adc_handle* h, float* dst, int cap, int small_variant, int small_L)
{
    const AdcParams& p = h->p;
    if (!adc_cost_agg_flat_fits(h, cap)) return hipErrorInvalidValue;
    AggCostIn ci;
    ci.rrec = reinterpret_cast<const uint4*>(h->cost_rrec);
    ci.lrec = reinterpret_cast<const uint4*>(h->cost_lrec);
    ci.lut_ad = h->lut_ad;
    ci.lut_census = h->lut_census;
    ci.rpitch = h->rrec_pitch; ci.padl = h->rrec_padl; ci.dmin = p.dmin; ci.D = p.D;
    const int tiles = (p.W + CF_TX - 1) / CF_TX;
    if (p.D == p.Dp)
        hipLaunchKernelGGL(k_cost_agg_flat<false>, dim3((unsigned)tiles * p.H), dim3(256), cost_agg_flat_lds(h, cap), h->heavy, dst, h->rec_h,
                           p.W, p.H, p.Dp, cap, tiles, h->armmax, small_variant, small_L, ci);
    else
        hipLaunchKernelGGL(k_cost_agg_flat<true>, dim3((unsigned)tiles * p.H), dim3(256), cost_agg_flat_lds(h, cap), h->heavy, dst, h->rec_h,
                           p.W, p.H, p.Dp, cap, tiles, h->armmax, small_variant, small_L, ci);
    return hipGetLastError();
}

// ---------------------------------------------------------------------- volume pad / unpad (debug)
__global__ void k_pad_volume(const float* __restrict__ src, float* __restrict__ dst, size_t P, int D, int Dp, int to_padded)
{
    const size_t n = P * (size_t)Dp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t px = i / Dp;
        const int d = (int)(i % Dp);
        if (to_padded) dst[i] = d < D ? src[px * D + d] : 0.0f;
        else if (d < D) dst[px * D + d] = src[i];
    }
}

hipError_t adc_launch_pad_volume(adc_handle* h, const float* src_HWD, float* dst_HWDp)
{
    const AdcParams& p = h->p;
    hipLaunchKernelGGL(k_pad_volume, dim3(2048), dim3(256), 0, h->stream, src_HWD, dst_HWDp, (size_t)p.W * p.H, p.D, p.Dp, 1);
    return hipGetLastError();
}
hipError_t adc_launch_unpad_volume(adc_handle* h, const float* src_HWDp, float* dst_HWD)
{
    const AdcParams& p = h->p;
    hipLaunchKernelGGL(k_pad_volume, dim3(2048), dim3(256), 0, h->stream, src_HWDp, dst_HWD, (size_t)p.W * p.H, p.D, p.Dp, 0);
    return hipGetLastError();
}
