// k_eval.hip -- evaluation of a disparity map against ground truth (include/adcensus_c_api.h: adc_set_ground_truth,
// adc_evaluate_device; the definition is tests/eval_ref.py, which these kernels match bit for bit).
//
//   k_eval_gt<FMT>   once per side and set call: the caller's raw array (row pitch in bytes) -> g float32 [P], unknown = +inf
//   k_eval_occ       once per set call: the occlusion byte map (1 = known and non-occluded) from the right-view ground truth (a
//                    gather within the pixel's own row) or from the caller's mask
//   k_eval_measure   per evaluation: one pass over d, g, the occlusion byte and optionally provenance and confidence; writes err
//                    and class if asked, and adds the report's counters to the report words in HBM
//
// k_eval_measure follows k_outputs.hip: a wave owns chunks of 64 consecutive pixels; every count is a __ballot / __popcll into a
// wave-uniform register (the fill classes too: four more ballot groups, no LDS conflict at all), the eq sums are per-lane 64-bit
// accumulators reduced across the wave at the end.  Only the histograms (error bins of both masks, confidence bins) are per-pixel
// LDS integer atomics.  The waves add their totals into the workgroup's LDS image of the report; the image is flushed with one
// 64-bit integer atomic per NONZERO word.  The grid is a fixed multiple of the CU count with a grid-stride loop over the tiles, so
// the number of flushes does not grow with the image (k_outputs.hip records what thousands of atomics on one word cost).
// Everything accumulated is an integer: the order of arrival cannot change a bit.  No float atomics, plain vector stores only.
//
// Arithmetic: IEEE binary32, one rounding per operation (-ffp-contract=off, pragma in adc_device_fn.h), correctly rounded division.
#include "adc_internal.h"
#include "adc_device_fn.h"

#define EV_WG 256
#define EV_WAVES (EV_WG / ADC_WAVE)
#define EV_PER_WAVE 4                               // chunks of 64 consecutive pixels a wave owns per tile
#define EV_TILE (EV_WG * EV_PER_WAVE)               // pixels per workgroup and grid-stride step
#define EV_GRID_PER_CU 2                            // workgroups per CU (8 waves with 4 chunks of loads in flight each)
#define EV_NT ADC_EVAL_MAX_THRESHOLDS

// Word offsets of adc_eval_report (uint64 each): the two mask blocks, the fill classes, the speckle count, the confidence bins
#define EV_MASK_WORDS (4 + EV_NT + ADC_EVAL_ERR_BINS) // pixels, invalid, bad[], sum_err_q, sum_sq_err_q, err_hist[]
#define EV_MASK_SCAL (4 + EV_NT)
#define EV_FILL_WORDS (3 + EV_NT)                     // pixels, invalid, bad[], sum_err_q
#define EV_OFF_FILL (2 * EV_MASK_WORDS)
#define EV_OFF_SPECKLE (EV_OFF_FILL + 4 * EV_FILL_WORDS)
#define EV_OFF_CONF (EV_OFF_SPECKLE + 1)
#define EV_WORDS (EV_OFF_CONF + 2 * ADC_EVAL_CONF_BINS)
#define EV_SCAL (2 * EV_MASK_SCAL + 4 * EV_FILL_WORDS + 1) // the words that are not histogram bins
static_assert(EV_WORDS * 8 == offsetof(adc_eval_report, thresholds), "the report words are the head of adc_eval_report");
static_assert(EV_OFF_FILL * 8 == offsetof(adc_eval_report, by_fill) && EV_OFF_CONF * 8 == offsetof(adc_eval_report, conf_pixels), "layout");

struct EvalArgs {
    const float* d;
    const float* g;
    const uint8_t* occ;
    const uint8_t* prov;  // may be null
    const float* conf;    // may be null (never without prov)
    float* err;           // may be null
    uint8_t* cls;         // may be null
    unsigned long long* rep;
    float t[EV_NT];       // unused thresholds: +inf (nothing is above it)
    int P, ntiles;
    int has_occ;
};

template <int FMT>
__global__ __launch_bounds__(256) void k_eval_gt(const uint8_t* __restrict__ raw, int pitch, float scale, float* __restrict__ g, int W, int P)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x); // (P <= 2^30: adc_create)
    if (i >= P) return;
    const int y = i / W, x = i - y * W;
    const uint8_t* row = raw + (size_t)y * (size_t)pitch;
    float v;
    bool zero = false;
    if (FMT == ADC_GT_U8) { const uint8_t u = row[x]; zero = u == 0; v = (float)u; }
    else if (FMT == ADC_GT_U16) { const uint16_t u = (uint16_t)(row[2 * x] | (row[2 * x + 1] << 8)); zero = u == 0; v = (float)u; } // (any pitch: bytes)
    else { const uint8_t* p = row + 4 * (size_t)x; v = __uint_as_float((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)); }
    const float q = v / scale;
    g[i] = (!zero && __builtin_isfinite(q)) ? q : ADC_INVALID_FLOAT;
}

// mode 1: cross-check with the right-view ground truth gr; mode 2: the caller's mask (nonzero = non-occluded)
__global__ __launch_bounds__(256) void k_eval_occ(const float* __restrict__ g, const float* __restrict__ gr, const uint8_t* __restrict__ mask,
                                                  float occ_thres, uint8_t* __restrict__ occ, int W, int P, int mode)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P) return;
    const int y = i / W, x = i - y * W;
    const float gl = g[i];
    bool ok = __builtin_isfinite(gl);
    if (ok && mode == 1) {
        const float r = rintf(gl); // ties to even
        ok = __builtin_fabsf(r) <= 1073741824.0f;
        if (ok) {
            const int xr = x - (int)r;
            ok = xr >= 0 && xr < W;
            if (ok) {
                const float v = gr[(size_t)y * W + xr];
                ok = __builtin_isfinite(v) && __builtin_fabsf(v - gl) <= occ_thres;
            }
        }
    } else if (ok) {
        ok = mask[i] != 0;
    }
    occ[i] = ok ? 1 : 0;
}

__device__ __forceinline__ uint32_t ev_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

__device__ __forceinline__ unsigned long long ev_wave_sum(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, ADC_WAVE);
    return v;
}

__global__ __launch_bounds__(EV_WG) void k_eval_measure(const EvalArgs a)
{
    __shared__ uint32_t s_hist[4][256];            // error bins of `all`, of `nonocc`, confidence pixels, confidence bad
    __shared__ unsigned long long s_scal[EV_SCAL]; // [0, 8) all, [8, 16) nonocc, then 4 x 7 fill words, the speckle count
    for (int j = (int)threadIdx.x; j < 4 * 256; j += EV_WG) (&s_hist[0][0])[j] = 0;
    for (int j = (int)threadIdx.x; j < EV_SCAL; j += EV_WG) s_scal[j] = 0;
    __syncthreads();
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    uint32_t c_all[2 + EV_NT] = {0}, c_non[2 + EV_NT] = {0}, c_fill[4][2 + EV_NT] = {{0}}, c_spk = 0; // wave-uniform counts
    unsigned long long sum_all = 0, sq_all = 0, sum_non = 0, sq_non = 0, sum_fill[4] = {0, 0, 0, 0};  // per lane
    for (int tile = (int)blockIdx.x; tile < a.ntiles; tile += (int)gridDim.x) {
        const int base = tile * EV_TILE + wave * (ADC_WAVE * EV_PER_WAVE);
#pragma unroll
        for (int k = 0; k < EV_PER_WAVE; k++) {
            const int i = base + k * ADC_WAVE + lane;
            const bool in = i < a.P;
            const float d = in ? a.d[i] : ADC_INVALID_FLOAT;
            const float g = in ? a.g[i] : ADC_INVALID_FLOAT;
            const bool known = __builtin_isfinite(g);
            const bool valid = __builtin_isfinite(d);
            const bool kv = known && valid;
            const bool non = known && a.occ[in ? i : 0] != 0;
            const bool nv = non && valid;
            const float e = kv ? __builtin_fabsf(d - g) : ADC_INVALID_FLOAT;
            const uint32_t eq = kv ? (uint32_t)rintf(fminf(e, 2048.0f) * 1024.0f) : 0u;
            const unsigned long long eq2 = (unsigned long long)eq * eq;
            bool bad[EV_NT];
#pragma unroll
            for (int t = 0; t < EV_NT; t++) bad[t] = kv && e > a.t[t];
            c_all[0] += ev_count(known);
            c_all[1] += ev_count(known && !valid);
            c_non[0] += ev_count(non);
            c_non[1] += ev_count(non && !valid);
#pragma unroll
            for (int t = 0; t < EV_NT; t++) {
                c_all[2 + t] += ev_count(bad[t]);
                c_non[2 + t] += ev_count(non && bad[t]);
            }
            if (kv) {
                const uint32_t bin = (eq >> 8) < 255u ? (eq >> 8) : 255u;
                sum_all += eq;
                sq_all += eq2;
                atomicAdd(&s_hist[0][bin], 1u);
                if (nv) {
                    sum_non += eq;
                    sq_non += eq2;
                    atomicAdd(&s_hist[1][bin], 1u);
                }
            }
            if (a.prov) {
                const uint32_t code = in ? a.prov[i] : 0u;
                const uint32_t fill = (code >> ADC_PROV_FILL_SHIFT) & 3u;
#pragma unroll
                for (uint32_t f = 0; f < 4; f++) {
                    const bool m = known && fill == f;
                    c_fill[f][0] += ev_count(m);
                    c_fill[f][1] += ev_count(m && !valid);
#pragma unroll
                    for (int t = 0; t < EV_NT; t++) c_fill[f][2 + t] += ev_count(m && bad[t]);
                    sum_fill[f] += (m && valid) ? eq : 0u;
                }
                c_spk += ev_count(known && (code & ADC_PROV_SPECKLE) != 0);
                if (a.conf && kv && fill == ADC_FILL_WTA) {
                    const float c = a.conf[i] * 256.0f;
                    const uint32_t b = !(c >= 0.0f) ? 0u : (c >= 255.0f ? 255u : (uint32_t)(int)c);
                    atomicAdd(&s_hist[2][b], 1u);
                    if (bad[0]) atomicAdd(&s_hist[3][b], 1u);
                }
            }
            if (in) {
                if (a.err) a.err[i] = e;
                if (a.cls)
                    a.cls[i] = (uint8_t)((known ? ADC_EVAL_KNOWN : 0) | (valid ? ADC_EVAL_VALID : 0) | (bad[0] ? ADC_EVAL_BAD : 0) |
                                         ((known && a.has_occ && !non) ? ADC_EVAL_OCCLUDED : 0));
            }
        }
    }
    // the wave's totals -> the workgroup's LDS image (64-bit LDS integer atomics, one lane)
    sum_all = ev_wave_sum(sum_all); sq_all = ev_wave_sum(sq_all);
    sum_non = ev_wave_sum(sum_non); sq_non = ev_wave_sum(sq_non);
    if (a.prov) {
#pragma unroll
        for (int f = 0; f < 4; f++) sum_fill[f] = ev_wave_sum(sum_fill[f]);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 2 + EV_NT; j++) {
            if (c_all[j]) atomicAdd(&s_scal[j], (unsigned long long)c_all[j]);
            if (c_non[j]) atomicAdd(&s_scal[EV_MASK_SCAL + j], (unsigned long long)c_non[j]);
        }
        if (sum_all) atomicAdd(&s_scal[2 + EV_NT], sum_all);
        if (sq_all) atomicAdd(&s_scal[3 + EV_NT], sq_all);
        if (sum_non) atomicAdd(&s_scal[EV_MASK_SCAL + 2 + EV_NT], sum_non);
        if (sq_non) atomicAdd(&s_scal[EV_MASK_SCAL + 3 + EV_NT], sq_non);
        if (a.prov) {
#pragma unroll
            for (int f = 0; f < 4; f++) {
#pragma unroll
                for (int j = 0; j < 2 + EV_NT; j++)
                    if (c_fill[f][j]) atomicAdd(&s_scal[2 * EV_MASK_SCAL + f * EV_FILL_WORDS + j], (unsigned long long)c_fill[f][j]);
                if (sum_fill[f]) atomicAdd(&s_scal[2 * EV_MASK_SCAL + f * EV_FILL_WORDS + 2 + EV_NT], sum_fill[f]);
            }
            if (c_spk) atomicAdd(&s_scal[2 * EV_MASK_SCAL + 4 * EV_FILL_WORDS], (unsigned long long)c_spk);
        }
    }
    __syncthreads();
    // the image -> the report words: one 64-bit atomic per nonzero word
    for (int j = (int)threadIdx.x; j < EV_WORDS; j += EV_WG) {
        unsigned long long v;
        if (j < EV_OFF_FILL) {
            const int m = j >= EV_MASK_WORDS ? 1 : 0, r = j - m * EV_MASK_WORDS;
            v = r < EV_MASK_SCAL ? s_scal[m * EV_MASK_SCAL + r] : (unsigned long long)s_hist[m][r - EV_MASK_SCAL];
        } else if (j < EV_OFF_CONF) {
            v = s_scal[2 * EV_MASK_SCAL + (j - EV_OFF_FILL)];
        } else {
            v = (unsigned long long)(&s_hist[2][0])[j - EV_OFF_CONF];
        }
        if (v) atomicAdd(&a.rep[j], v);
    }
}

size_t adc_eval_report_words(void) { return EV_WORDS; }

hipError_t adc_launch_eval_gt(adc_handle* h, int side, int format, int pitch, float scale)
{
    const int W = h->p.W, P = h->p.W * h->p.H;
    const dim3 grid((unsigned)((P + 255) / 256));
    if (format == ADC_GT_U8) hipLaunchKernelGGL(k_eval_gt<ADC_GT_U8>, grid, dim3(256), 0, h->stream, h->ev_raw, pitch, scale, h->ev_g[side], W, P);
    else if (format == ADC_GT_U16) hipLaunchKernelGGL(k_eval_gt<ADC_GT_U16>, grid, dim3(256), 0, h->stream, h->ev_raw, pitch, scale, h->ev_g[side], W, P);
    else hipLaunchKernelGGL(k_eval_gt<ADC_GT_F32>, grid, dim3(256), 0, h->stream, h->ev_raw, pitch, scale, h->ev_g[side], W, P);
    return hipGetLastError();
}

hipError_t adc_launch_eval_occ(adc_handle* h, int mode, float occ_thres)
{
    const int W = h->p.W, P = h->p.W * h->p.H;
    hipLaunchKernelGGL(k_eval_occ, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, h->ev_g[0], h->ev_g[1], h->ev_raw, occ_thres,
                       h->ev_occ, W, P, mode);
    return hipGetLastError();
}

hipError_t adc_launch_eval_measure(adc_handle* h, const float* disp, const uint8_t* prov, const float* conf, const float* thresholds, float* err,
                                   uint8_t* cls)
{
    EvalArgs a;
    a.d = disp; a.g = h->ev_g[0]; a.occ = h->ev_occ; a.prov = prov; a.conf = conf; a.err = err; a.cls = cls;
    a.rep = reinterpret_cast<unsigned long long*>(h->ev_rep);
    for (int t = 0; t < EV_NT; t++) a.t[t] = thresholds[t];
    a.P = h->p.W * h->p.H;
    a.ntiles = (a.P + EV_TILE - 1) / EV_TILE;
    a.has_occ = (h->ev_has_right || h->ev_has_mask) ? 1 : 0;
    const int cap = EV_GRID_PER_CU * (h->ev_cus > 0 ? h->ev_cus : 256);
    hipLaunchKernelGGL(k_eval_measure, dim3((unsigned)(a.ntiles < cap ? a.ntiles : cap)), dim3(EV_WG), 0, h->stream, a);
    return hipGetLastError();
}
