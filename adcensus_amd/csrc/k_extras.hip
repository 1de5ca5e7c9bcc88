// k_extras.hip -- the optional per-pixel outputs of adc_match_ex / adc_match_device_ex (include/adcensus_c_api.h).
//
// Confidence (run_heavy, behind the winner-takes-all): one read of the scanline-optimised volume vol_a.  Per pixel, c1 = the
// first minimum of the costs (lowest d among equal costs: the reference's WTA, ADCensusStereo.cpp:188-243), d1 its index,
// c2 = min { C[d] : |d - d1| >= 2 }; confidence = (c2 - c1) / c2, 0 when c2 == 0, 1 when that set is empty.
// Provenance (top of run_refine_tail, after the region voting): code = lr | fill << 2 from the LR-check labels and the voted
// map; it also sets the confidence to 0 wherever the value was not the pixel's own winner-takes-all result.
#include "adc_internal.h"
#include "adc_device_fn.h"

// ------------------------------------------------------------------------------------------------------------ confidence
// A workgroup is ONE wave and owns 64 consecutive pixels (lane = pixel).  Their cost vectors are consecutive in the volume, so
// the wave walks them in chunks of 64 disparities: 16 float4 loads per lane bring a 64 x 64 block in (each load = 4 pixels x
// 256 contiguous bytes), ds_write_b128 puts it into LDS with a row pitch of 68 floats (8 consecutive lanes of a store hit 32
// different banks), and every lane then reads its own pixel's 64 costs back with 16 ds_read_b128 (16 lanes of a read start on
// 16 different 4-bank groups: conflict-free).  The loads of chunk k + 1 are in flight while chunk k is scanned.
//
// One pass per pixel, in increasing d, for any number of chunks (D up to 2047):
//   cur    = min C[0 .. d-1]       (strict '<' update: d1 = the index of the first minimum)
//   prev   = min C[0 .. d-2]
//   before = min C[0 .. d1-2]      (prev at the moment d1 was set)
//   after  = min C[d1+2 .. d-1]    (reset when d1 moves; the element right behind d1 is skipped)
// and c2 = min(before, after).  Padding disparities (d >= D) count as +inf: they change none of the four.
#define CONF_PITCH4 17 // 16-byte vectors per LDS row: 64 costs + 4 floats of padding
typedef float conf_f4 __attribute__((ext_vector_type(4))); // (the nontemporal builtin takes native vector types only)

__global__ __launch_bounds__(64) void k_confidence(const float* __restrict__ vol, float* __restrict__ conf, int P, int D, int Dp)
{
    __shared__ conf_f4 blk[64 * CONF_PITCH4];
    const int lane = threadIdx.x;
    const int pix0 = (int)blockIdx.x * 64;
    const int lp = lane >> 4, lq = lane & 15; // loads: pixel 4 * j + lp of the block, float4 lq of its 64-cost chunk
    const conf_f4* src[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int pix = min(pix0 + 4 * j + lp, P - 1); // (the last block: clamped, loads stay in bounds; its results are not stored)
        src[j] = reinterpret_cast<const conf_f4*>(vol + (size_t)pix * Dp) + lq;
    }
    conf_f4 buf[16];
#pragma unroll
    for (int j = 0; j < 16; j++) buf[j] = __builtin_nontemporal_load(src[j]);
    const float INF = __builtin_inff();
    float cur = INF, prev = INF, before = INF, after = INF;
    bool skip = false; // the element right behind d1
    const int nchunk = Dp >> 6;
    for (int k = 0; k < nchunk; k++) {
        if (k) __syncthreads(); // (every lane has read the previous chunk)
#pragma unroll
        for (int j = 0; j < 16; j++) blk[(4 * j + lp) * CONF_PITCH4 + lq] = buf[j];
        if (k + 1 < nchunk) {
#pragma unroll
            for (int j = 0; j < 16; j++) buf[j] = __builtin_nontemporal_load(src[j] + 16 * (k + 1));
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; m++) {
            const conf_f4 q = blk[lane * CONF_PITCH4 + m];
            const float qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int d = 64 * k + 4 * m + c;
                const float v = d < D ? qv[c] : INF;
                const bool lt = v < cur;
                const float aft = (skip || !(v < after)) ? after : v;
                before = lt ? prev : before;
                after = lt ? INF : aft;
                skip = lt;
                prev = cur;
                cur = lt ? v : cur;
            }
        }
    }
    const float c2 = before < after ? before : after;
    float out;
    if (c2 == INF) out = 1.0f;       // no disparity at least two steps away from d1 (D <= 3)
    else if (c2 == 0.0f) out = 0.0f; // (then c1 == 0 too)
    else out = (c2 - cur) / c2;
    if (pix0 + lane < P) conf[pix0 + lane] = out;
}

hipError_t adc_launch_confidence(adc_handle* h)
{
    const AdcParams& p = h->p;
    const int P = p.W * p.H; // (adc_create: W * H <= 2^30)
    hipLaunchKernelGGL(k_confidence, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, h->heavy, h->vol_a, h->fly.req.conf, P, p.D, p.Dp);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------ provenance
// Elementwise.  At the top of run_refine_tail disp_l holds the map the voting left: the WTA value where the LR check passed,
// the voted value or +inf (Invalid_Float) at the outliers.  Idempotent: adc_wait's redo paths run it again.
__global__ __launch_bounds__(256) void k_provenance(const uint8_t* __restrict__ label, const float* __restrict__ disp,
                                                    uint8_t* __restrict__ prov, float* __restrict__ conf, int P, int filling)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= P) return;
    const int lr = label[i];
    const bool finite = __builtin_isfinite(disp[i]);
    int fill;
    if (lr == ADC_LR_CONSISTENT) fill = finite ? ADC_FILL_WTA : ADC_FILL_NONE; // (+inf here: no LR check, WTA at a range end)
    else if (!filling) fill = ADC_FILL_NONE;
    else fill = finite ? ADC_FILL_VOTING : ADC_FILL_INTERPOLATION;
    if (prov) prov[i] = (uint8_t)(lr | (fill << ADC_PROV_FILL_SHIFT));
    if (conf && fill != ADC_FILL_WTA) conf[i] = 0.0f;
}

hipError_t adc_launch_provenance(adc_handle* h)
{
    const AdcParams& p = h->p;
    const int P = p.W * p.H;
    const int filling = p.opt.do_lr_check && p.opt.do_filling;
    hipLaunchKernelGGL(k_provenance, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, h->label, h->disp_l, h->fly.req.prov, h->fly.req.conf, P,
                       filling);
    return hipGetLastError();
}
