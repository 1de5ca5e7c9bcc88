// k_register.hip -- registration of depth into a second camera (include/adcensus_c_api.h: adc_set_register_target,
// adc_register_depth_device, adc_align_color_device; the arithmetic is reg_project.h, the definition in numpy tests/register_ref.py,
// which these kernels match bit for bit).
//
//   k_reg_scatter   reads the source map once; every pixel with a non-empty footprint sends its 64-bit key {bits(Zc), raster index}
//                   to the z-buffer words of its footprint with one unsigned 64-bit atomic minimum each (global_atomic_umin_x2, no
//                   compare-and-swap loop).  The minimum of a set does not depend on the order of arrival: the nearest surface wins,
//                   among equal depths the lowest raster index.  The two source counts are ballots reduced per wave, added per
//                   workgroup.
//   k_reg_resolve   z-buffer -> depth, index, the count of filled pixels: a plain streaming kernel, 8 bytes in, 8 out per target pixel
//   k_reg_align     the other direction: a gather of three bytes per source pixel through the centre projection
// Stream order separates scatter and resolve (the z-buffer is set to all ones by a hipMemsetAsync in front of the scatter, capi.hip);
// no kernel waits on another workgroup of its own launch.  Both counting kernels run on a grid that is a fixed multiple of the CU
// count with a grid-stride loop, so the atomics on the three report words do not grow with the image (k_outputs.hip records what
// thousands of atomics on one word cost).
//
// Lanes of a wave hold consecutive source pixels; step (di, dj) of the footprint loop therefore sends keys to (mostly) consecutive
// z-buffer words.  PRETEST (ADC_REG_PRETEST, kept for measurement): look at the word with a relaxed agent-scope load first and skip the
// atomic when the key cannot win.  The word only decreases, so a stale value costs a useless atomic, never a lost minimum.  Measured
// (profiles/register_timing.md): issuing every atomic is as fast or faster on three of four shapes (1080p -> 2160p, structured: 0.089
// against 0.097 ms), the pre-test wins by 1.4 % on one (1080p -> 2160p, noise); the default issues every atomic.
//
// Bounds: reg_footprint / reg_align_tap return integer pixel ranges clipped to the target AFTER the |u|, |v| < 32768 test; no float
// reaches an address.  Target pixel numbers go up to 32767 * 32767 < 2^31 and are widened before they are scaled to bytes.
#include "adc_internal.h"
#include "adc_device_fn.h"
#include "reg_project.h"

#define REG_WG 256
#define REG_WAVES (REG_WG / ADC_WAVE)
#define REG_GRID_PER_CU 4 // workgroups per CU of the two counting kernels

struct RegArgs {
    RegSource s;
    adc_reg_target t;
    const float* map;
    unsigned long long* zbuf;
    uint32_t* rep;            // [0] src_valid, [1] src_projected, [2] dst_filled
    int W, P;
    int splat;
};

__device__ __forceinline__ uint32_t reg_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

template <bool PRETEST>
__global__ __launch_bounds__(REG_WG) void k_reg_scatter(const RegArgs g)
{
    __shared__ uint32_t s_cnt[2][REG_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    uint32_t n_valid = 0, n_proj = 0; // wave-uniform
    for (long long base = (long long)blockIdx.x * REG_WG; base < g.P; base += (long long)gridDim.x * REG_WG) {
        const int i = (int)base + (int)threadIdx.x; // (P <= 2^30: adc_create)
        const bool in = i < g.P;
        float Z = 0.0f;
        const bool valid = in && reg_source_z(g.s, g.map[i], &Z);
        RegFoot f;
        bool proj = false;
        int x = 0, y = 0;
        if (valid) {
            y = i / g.W;
            x = i - y * g.W;
            proj = reg_footprint(g.s, g.t, x, y, Z, g.splat != 0, &f);
        }
        n_valid += reg_count(valid);
        n_proj += reg_count(proj);
        if (proj) {
            const unsigned long long key = reg_key(f.zc, g.W, x, y);
            for (int ti = f.i0; ti <= f.i1; ti++) {
                unsigned long long* row = g.zbuf + (size_t)ti * (size_t)g.t.width;
                for (int tj = f.j0; tj <= f.j1; tj++) {
                    if (PRETEST && !(key < __hip_atomic_load(row + tj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) continue;
                    (void)__hip_atomic_fetch_min(row + tj, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
    if (lane == 0) { s_cnt[0][wave] = n_valid; s_cnt[1][wave] = n_proj; }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t t = 0;
        for (int w = 0; w < REG_WAVES; w++) t += s_cnt[threadIdx.x][w];
        if (t) atomicAdd(&g.rep[threadIdx.x], t);
    }
}

__global__ __launch_bounds__(REG_WG) void k_reg_resolve(const unsigned long long* __restrict__ zbuf, float* __restrict__ depth, int32_t* __restrict__ index,
                                                        uint32_t* __restrict__ rep, long long Pt)
{
    __shared__ uint32_t s_cnt[REG_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    uint32_t filled = 0; // wave-uniform
    for (long long base = (long long)blockIdx.x * REG_WG; base < Pt; base += (long long)gridDim.x * REG_WG) {
        const long long i = base + (long long)threadIdx.x;
        bool hit = false;
        if (i < Pt) {
            const unsigned long long key = zbuf[i];
            hit = key != REG_KEY_EMPTY;
            if (depth) depth[i] = hit ? reg_bits_float((uint32_t)(key >> 32)) : ADC_INVALID_FLOAT;
            if (index) index[i] = hit ? (int32_t)(uint32_t)key : -1;
        }
        filled += reg_count(hit);
    }
    if (lane == 0) s_cnt[wave] = filled;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < REG_WAVES; w++) t += s_cnt[w];
        if (t) atomicAdd(&rep[2], t);
    }
}

__global__ __launch_bounds__(REG_WG) void k_reg_align(const RegSource s, const adc_reg_target t, const float* __restrict__ map, const uint8_t* __restrict__ tbgr,
                                                      uint8_t* __restrict__ out, uint8_t* __restrict__ valid, int W, int P)
{
    const int i = (int)(blockIdx.x * REG_WG + threadIdx.x); // (P <= 2^30: adc_create)
    if (i >= P) return;
    const int y = i / W, x = i - y * W;
    int ti, tj;
    const bool ok = reg_align_tap(s, t, x, y, map[i], &ti, &tj);
    uint8_t b = 0, gch = 0, r = 0;
    if (ok) {
        const uint8_t* c = tbgr + ((size_t)ti * (size_t)t.width + (size_t)tj) * 3;
        b = c[0]; gch = c[1]; r = c[2];
    }
    uint8_t* o = out + (size_t)i * 3;
    o[0] = b; o[1] = gch; o[2] = r;
    if (valid) valid[i] = ok ? 1 : 0;
}

static RegSource reg_source(int kind, const adc_calib& c)
{
    RegSource s;
    s.kind = kind;
    s.fb = c.focal_px * c.baseline;
    s.focal = c.focal_px; s.cx = c.cx; s.cy = c.cy; s.doffs = c.doffs;
    return s;
}

static unsigned reg_grid(const adc_handle* h, long long n)
{
    const long long tiles = (n + REG_WG - 1) / REG_WG, cap = (long long)REG_GRID_PER_CU * (h->reg_cus > 0 ? h->reg_cus : 256);
    return (unsigned)(tiles < cap ? tiles : cap);
}

hipError_t adc_launch_reg_scatter(adc_handle* h, const float* map, int kind, const adc_calib* calib, uint32_t flags)
{
    RegArgs g;
    g.s = reg_source(kind, *calib);
    g.t = h->reg_target;
    g.map = map;
    g.zbuf = reinterpret_cast<unsigned long long*>(h->reg_zbuf);
    g.rep = h->reg_rep;
    g.W = h->p.W;
    g.P = h->p.W * h->p.H;
    g.splat = (flags & ADC_REG_NO_SPLAT) ? 0 : 1;
    const dim3 grid(reg_grid(h, g.P));
    if (flags & ADC_REG_PRETEST) hipLaunchKernelGGL(k_reg_scatter<true>, grid, dim3(REG_WG), 0, h->stream, g);
    else hipLaunchKernelGGL(k_reg_scatter<false>, grid, dim3(REG_WG), 0, h->stream, g);
    return hipGetLastError();
}

hipError_t adc_launch_reg_resolve(adc_handle* h, float* depth, int32_t* index)
{
    const long long Pt = (long long)h->reg_target.width * h->reg_target.height;
    hipLaunchKernelGGL(k_reg_resolve, dim3(reg_grid(h, Pt)), dim3(REG_WG), 0, h->stream, reinterpret_cast<const unsigned long long*>(h->reg_zbuf), depth, index,
                       h->reg_rep, Pt);
    return hipGetLastError();
}

hipError_t adc_launch_reg_align(adc_handle* h, const float* map, int kind, const adc_calib* calib, const uint8_t* tbgr, uint8_t* out, uint8_t* valid)
{
    const int P = h->p.W * h->p.H;
    hipLaunchKernelGGL(k_reg_align, dim3((unsigned)((P + REG_WG - 1) / REG_WG)), dim3(REG_WG), 0, h->stream, reg_source(kind, *calib), h->reg_target, map, tbgr, out,
                       valid, h->p.W, P);
    return hipGetLastError();
}
