// k_outputs.hip -- the outputs that are functions of the final left-view disparity map (include/adcensus_c_api.h: adc_outputs):
// the min-max normalised 8-bit image of the reference's SaveDisparityMap (main.cpp:180-206), metric depth Z = f * B / (|d| + doffs),
// and the point list of SaveDisparityCloud (main.cpp:212-230), one 16-byte point per valid pixel IN RASTER ORDER.
//
// Three launches on the object stream behind the median, none of which depends on another workgroup of its own launch:
//   k_out_measure   reads the map once: depth (elementwise), min / max of |d| for the image, valid pixels per tile for the cloud
//   k_out_scan      one workgroup: exclusive scan of the tile counts (a few thousand) in place, total -> the count words
//   k_out_emit      reads the map again: the 8-bit image from the finished min / max, the points behind their tile's base
// Only what was asked for runs: depth alone is the first launch, the image alone the first and the third.
// A fourth kernel, k_disp16, is independent of the three: the map in 16-bit fixed point (adc_products.disp16).
//
// Arithmetic: IEEE binary32, one rounding per operation (-ffp-contract=off, pragma in adc_device_fn.h), correctly rounded
// divisions.  a = |d|.  The min / max use that for non-negative floats (and +inf is excluded, a >= +0) the unsigned order of
// the bit pattern is the float order: integer atomics on the bits are exact and independent of the order of arrival.  Both
// words start at 0 (one hipMemsetAsync): word 0 holds max(~bits(a)), i.e. the minimum, word 1 max(bits(a)).  The definition's
// start values mn = float(W), mx = -float(W) are applied when the words are decoded: the maximum of at least one a >= 0 and -W is
// that of the a alone, and with no a at all both forms give !(mx > mn).
#include "adc_internal.h"
#include "adc_device_fn.h"

#define OUT_WG 256
#define OUT_WAVES (OUT_WG / ADC_WAVE)
#define OUT_PER_WAVE 4                                // chunks of 64 consecutive pixels a wave owns
#define OUT_TILE (OUT_WG * OUT_PER_WAVE)              // pixels per workgroup: wave w owns [w * 256, w * 256 + 256) of the tile

struct OutArgs {
    const float* disp;
    const uint8_t* img;   // left image, B,G,R per pixel (cloud only)
    float* depth;         // may be null
    uint4* cloud;         // may be null
    uint8_t* disp8;       // may be null
    uint32_t* words;      // [0] max(~bits(a)), [1] max(bits(a)), [2] count, [4 ...] tile counts -> tile bases
    uint32_t* count_out;  // the caller's device word, may be null
    uint32_t capacity;
    int P, W;
    int calibrated;
    float fb, focal, cx, cy, doffs;
};

// validity and Z of one pixel for the calibrated outputs: valid <=> a finite and s = a + doffs > 0; Z = fb / s
__device__ __forceinline__ bool out_depth(const OutArgs& g, float a, float* z)
{
    const float s = a + g.doffs;
    const bool ok = __builtin_isfinite(a) && s > 0.0f;
    *z = ok ? g.fb / s : ADC_INVALID_FLOAT;
    return ok;
}

__device__ __forceinline__ bool out_cloud_valid(const OutArgs& g, float a)
{
    if (!g.calibrated) return a != ADC_INVALID_FLOAT;
    return __builtin_isfinite(a) && a + g.doffs > 0.0f;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)v, o, ADC_WAVE);
        v = t > v ? t : v;
    }
    return v;
}

__global__ __launch_bounds__(OUT_WG) void k_out_measure(const OutArgs g)
{
    __shared__ uint32_t s_cnt[OUT_WAVES], s_min[OUT_WAVES], s_max[OUT_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const int base = (int)blockIdx.x * OUT_TILE + wave * (ADC_WAVE * OUT_PER_WAVE);
    uint32_t nmin = 0, nmax = 0, cnt = 0;
#pragma unroll
    for (int k = 0; k < OUT_PER_WAVE; k++) {
        const int i = base + k * ADC_WAVE + lane;
        bool valid = false;
        if (i < g.P) {
            const float a = __builtin_fabsf(g.disp[i]);
            if (g.depth) {
                float z;
                out_depth(g, a, &z);
                g.depth[i] = z;
            }
            if (g.disp8 && a != ADC_INVALID_FLOAT) {
                const uint32_t b = __float_as_uint(a);
                nmin = ~b > nmin ? ~b : nmin;
                nmax = b > nmax ? b : nmax;
            }
            valid = g.cloud && out_cloud_valid(g, a);
        }
        cnt += (uint32_t)__popcll(__ballot(valid));
    }
    if (!g.disp8 && !g.cloud) return;
    if (g.disp8) {
        nmin = wave_max_u32(nmin);
        nmax = wave_max_u32(nmax);
    }
    if (lane == 0) { s_cnt[wave] = cnt; s_min[wave] = nmin; s_max[wave] = nmax; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (g.cloud) {
        uint32_t t = 0;
        for (int w = 0; w < OUT_WAVES; w++) t += s_cnt[w];
        g.words[4 + blockIdx.x] = t;
    }
    if (g.disp8) {
        for (int w = 1; w < OUT_WAVES; w++) { nmin = s_min[w] > nmin ? s_min[w] : nmin; nmax = s_max[w] > nmax ? s_max[w] : nmax; }
        // One atomic per word and workgroup at most, and only where it can still raise the word: thousands of atomics on one
        // address serialise in the L2 (measured: 0.19 ms at 1080p with one pair per wave).  The word only grows, so a value read
        // here that is already out of date costs an atomic that changes nothing, never a missed maximum.
        if (nmin > __hip_atomic_load(&g.words[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&g.words[0], nmin);
        if (nmax > __hip_atomic_load(&g.words[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&g.words[1], nmax);
    }
}

// One workgroup of 1024: tile counts -> exclusive prefix sums in place, chunk by chunk with a carry; the total goes to the
// handle's count word (read back by the launcher) and to the caller's device word.
__global__ __launch_bounds__(1024) void k_out_scan(uint32_t* __restrict__ words, int ntiles, uint32_t* __restrict__ count_out)
{
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_carry;
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    uint32_t* tiles = words + 4;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int c = 0; c < ntiles; c += 1024) {
        const int i = c + (int)threadIdx.x;
        const uint32_t v = i < ntiles ? tiles[i] : 0u;
        uint32_t incl = v;
        for (int o = 1; o < ADC_WAVE; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, o, ADC_WAVE);
            if (lane >= o) incl += t;
        }
        if (lane == ADC_WAVE - 1) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = s_carry, total = 0;
        for (int w = 0; w < 16; w++) {
            const uint32_t t = s_wave[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < ntiles) tiles[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 0) s_carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        words[2] = s_carry;
        if (count_out) *count_out = s_carry;
    }
}

__global__ __launch_bounds__(OUT_WG) void k_out_emit(const OutArgs g)
{
    __shared__ uint32_t s_cnt[OUT_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const int base = (int)blockIdx.x * OUT_TILE + wave * (ADC_WAVE * OUT_PER_WAVE);
    float mn = 0.f, range = 0.f;
    bool spread = false;
    if (g.disp8) {
        const uint32_t w0 = g.words[0], w1 = g.words[1];
        const float fw = (float)g.W;
        float lo = fw;
        if (w0) { const float m = __uint_as_float(~w0); lo = m < fw ? m : fw; }
        const float hi = __uint_as_float(w1); // (0 = +0.0f: nothing above zero was seen; the definition's -W then loses to no a or to an a of 0 alike)
        mn = lo;
        spread = w0 != 0 && hi > lo;
        range = hi - lo;
    }
    float a[OUT_PER_WAVE];
    unsigned long long mask[OUT_PER_WAVE];
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < OUT_PER_WAVE; k++) {
        const int i = base + k * ADC_WAVE + lane;
        bool valid = false;
        a[k] = ADC_INVALID_FLOAT;
        if (i < g.P) {
            a[k] = __builtin_fabsf(g.disp[i]);
            if (g.disp8) {
                uint8_t v = 0;
                if (spread && a[k] != ADC_INVALID_FLOAT) v = (uint8_t)((a[k] - mn) / range * 255.0f);
                g.disp8[i] = v;
            }
            valid = g.cloud && out_cloud_valid(g, a[k]);
        }
        mask[k] = __ballot(valid);
        cnt += (uint32_t)__popcll(mask[k]);
    }
    if (!g.cloud) return;
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    uint32_t pos = g.words[4 + blockIdx.x]; // the tile's base: valid pixels of all tiles before it
    for (int w = 0; w < wave; w++) pos += s_cnt[w];
#pragma unroll
    for (int k = 0; k < OUT_PER_WAVE; k++) {
        const int i = base + k * ADC_WAVE + lane;
        const unsigned long long m = mask[k];
        // lanes of this chunk that are valid and below this lane (v_mbcnt_lo / _hi)
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        const uint32_t at = pos + below;
        if (((m >> lane) & 1ull) && at < g.capacity) {
            const int y = i / g.W, x = i - y * g.W;
            float px = (float)x, py = (float)y, pz = a[k];
            if (g.calibrated) {
                out_depth(g, a[k], &pz);
                px = ((px - g.cx) * pz) / g.focal;
                py = ((py - g.cy) * pz) / g.focal;
            }
            const uint8_t* c = g.img + (size_t)i * 3;
            uint4 pt;
            pt.x = __float_as_uint(px);
            pt.y = __float_as_uint(py);
            pt.z = __float_as_uint(pz);
            pt.w = (uint32_t)c[2] | ((uint32_t)c[1] << 8) | ((uint32_t)c[0] << 16); // r, g, b, pad = 0
            g.cloud[at] = pt;
        }
        pos += (uint32_t)__popcll(m);
    }
}

// The 16-bit fixed-point map (include/adcensus_c_api.h: adc_products.disp16): a = |d|; not finite -> 0; otherwise
// (uint16_t)fminf(fmaxf(a * scale, 1.0f), 65535.0f) -- one multiply, one rounding; an overflowing product is +inf and saturates.
// A streaming kernel of its own: 4 bytes in, 2 bytes out per pixel, nothing shared between lanes.
__device__ __forceinline__ uint16_t disp16_pixel(float d, float scale)
{
    const float a = __builtin_fabsf(d);
    if (!__builtin_isfinite(a)) return 0;
    const float p = a * scale;
    return (uint16_t)fminf(fmaxf(p, 1.0f), 65535.0f);
}

typedef float disp16_f4 __attribute__((ext_vector_type(4)));
typedef unsigned short disp16_u4 __attribute__((ext_vector_type(4)));
#define DISP16_WG 256
#define DISP16_PER_LANE 4

// vec (uniform): disp is 16-byte and out 8-byte aligned -- a lane owns 4 consecutive pixels, one 16-byte load and one 8-byte store;
// the lane that holds the end of the map walks its pixels one by one.  Otherwise the element-wise form: lane l of a workgroup
// owns pixels base + l, base + 256 + l, ... of the workgroup's 1024.
__global__ __launch_bounds__(DISP16_WG) void k_disp16(const float* __restrict__ disp, uint16_t* __restrict__ out, int P, float scale, int vec)
{
    const int base = (int)blockIdx.x * (DISP16_WG * DISP16_PER_LANE);
    if (vec) {
        const int i = base + (int)threadIdx.x * DISP16_PER_LANE;
        if (i + DISP16_PER_LANE <= P) {
            const disp16_f4 v = *reinterpret_cast<const disp16_f4*>(disp + i);
            disp16_u4 r;
            r.x = disp16_pixel(v.x, scale);
            r.y = disp16_pixel(v.y, scale);
            r.z = disp16_pixel(v.z, scale);
            r.w = disp16_pixel(v.w, scale);
            *reinterpret_cast<disp16_u4*>(out + i) = r;
        } else {
            for (int k = i; k < P; k++) out[k] = disp16_pixel(disp[k], scale);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < DISP16_PER_LANE; k++) {
        const int i = base + k * DISP16_WG + (int)threadIdx.x;
        if (i < P) out[i] = disp16_pixel(disp[i], scale);
    }
}

hipError_t adc_launch_disp16(adc_handle* h, const float* disp, float scale, uint16_t* out)
{
    const int P = h->p.W * h->p.H;
    const int vec = (((uintptr_t)disp & 15u) == 0 && ((uintptr_t)out & 7u) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_disp16, dim3((unsigned)((P + DISP16_WG * DISP16_PER_LANE - 1) / (DISP16_WG * DISP16_PER_LANE))), dim3(DISP16_WG), 0, h->stream,
                       disp, out, P, scale, vec);
    return hipGetLastError();
}

size_t adc_outputs_scratch_bytes(int W, int H)
{
    const size_t P = (size_t)W * H;
    return (4 + (P + OUT_TILE - 1) / OUT_TILE) * sizeof(uint32_t);
}

// The three launchers: disp is any device-resident map of the handle's geometry, img the left image; what h->fly.req.out asks for decides
// what a kernel does.  capi.hip (enqueue_outputs) orders them and owns every other HIP call of the path.
static OutArgs out_args(adc_handle* h, const float* disp, const uint8_t* img, bool with_cloud)
{
    const AdcOutReq& r = h->fly.req.out;
    OutArgs g;
    g.disp = disp;
    g.img = img;
    g.depth = r.depth;
    g.cloud = with_cloud ? static_cast<uint4*>(r.cloud) : nullptr;
    g.disp8 = r.disp8;
    g.words = h->out_words;
    g.count_out = r.cloud_count;
    g.capacity = r.capacity;
    g.P = h->p.W * h->p.H;
    g.W = h->p.W;
    g.calibrated = r.calibrated;
    g.fb = r.fb; g.focal = r.calib.focal_px; g.cx = r.calib.cx; g.cy = r.calib.cy; g.doffs = r.calib.doffs;
    return g;
}

hipError_t adc_launch_out_measure(adc_handle* h, const float* disp, const uint8_t* img, bool with_cloud)
{
    const OutArgs g = out_args(h, disp, img, with_cloud);
    hipLaunchKernelGGL(k_out_measure, dim3((unsigned)((g.P + OUT_TILE - 1) / OUT_TILE)), dim3(OUT_WG), 0, h->stream, g);
    return hipGetLastError();
}

hipError_t adc_launch_out_scan(adc_handle* h)
{
    const int P = h->p.W * h->p.H;
    hipLaunchKernelGGL(k_out_scan, dim3(1), dim3(1024), 0, h->stream, h->out_words, (P + OUT_TILE - 1) / OUT_TILE, h->fly.req.out.cloud_count);
    return hipGetLastError();
}

hipError_t adc_launch_out_emit(adc_handle* h, const float* disp, const uint8_t* img, bool with_cloud)
{
    const OutArgs g = out_args(h, disp, img, with_cloud);
    hipLaunchKernelGGL(k_out_emit, dim3((unsigned)((g.P + OUT_TILE - 1) / OUT_TILE)), dim3(OUT_WG), 0, h->stream, g);
    return hipGetLastError();
}
