// k_tsdf_raycast.hip -- the TSDF volume seen from a camera pose (include/adcensus_c_api.h: adc_tsdf_raycast_device; the ray rule is
// tsdf_ray.h, shared with the serial programs of the tests).
//
//   k_tsdf_raycast  A lane owns a ray, a wave an 8 x 8 block of pixels (neighbouring rays gather from the same lines of the volume),
//                   a workgroup of four waves 16 x 16 pixels.  The march is a wave loop that runs until the ballot of the live rays
//                   is empty; a ray takes at most max_steps samples, so the loop ends whatever the floats do.  A sample looks at its
//                   nearest voxel first: saturated free space costs one load and advances by `skip`; everything else costs the
//                   eight corner loads of the cell (the compiler joins each x-pair into one 8-byte load).  Measured and not kept
//                   (profiles/tsdf_raycast_timing.md): the eight corners first -- the same time within 3 % either way; a branch
//                   on the parity of i around explicit 8-byte loads of the x-pairs -- 9 to 30 % slower.  The volume is only read
//                   (L2 / Infinity Cache); no LDS beyond the per-wave partial sums of the report.  A pixel's outputs are plain vector stores behind the loop.  Per workgroup one
//                   integer atomic per status count that is not zero and one 64-bit add for the samples.
// No float reaches an address (tsdf_ray_cell clips the cell in integers before any load); every count is an integer and every ray
// has one owner: no result depends on the order of the waves.
#include "adc_internal.h"
#include "tsdf_ray.h"

#define TSDF_RAY_WG 256
#define TSDF_RAY_WAVES (TSDF_RAY_WG / ADC_WAVE)
#define TSDF_RAY_TILE 16 // pixels of a workgroup per axis: 2 x 2 waves of 8 x 8
static_assert(ADC_WAVE == 64 && TSDF_RAY_WAVES == 4, "a wave is 8 x 8 pixels, a workgroup 2 x 2 waves");

struct TsdfRayArgs {
    TsdfVol vol;
    TsdfRayView view;
    const uint32_t* tsdf;
    const uint32_t* color;  // null unless bgr is asked for
    float* depth;           // each may be null
    float4* normals;
    uint8_t* bgr;
    uint8_t* status;
    uint32_t* rep;          // the words of adc_tsdf_raycast_report: [0] rays [1..5] per status [6, 7] samples (64-bit)
};

__global__ __launch_bounds__(TSDF_RAY_WG) void k_tsdf_raycast(const TsdfRayArgs g)
{
    __shared__ uint32_t s_cnt[6][TSDF_RAY_WAVES]; // [0..4] rays per status, [5] samples
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const int x = (int)blockIdx.x * TSDF_RAY_TILE + (wave & 1) * 8 + (lane & 7);
    const int y = (int)blockIdx.y * TSDF_RAY_TILE + (wave >> 1) * 8 + (lane >> 3);
    const bool in = x < g.view.W && y < g.view.H;
    TsdfRay r = {};
    TsdfRayState s = {};
    s.status = ADC_TSDF_RAY_MISS; // (a lane without a pixel: never live, never counted)
    if (in) {
        r = tsdf_ray_setup(g.vol, g.view, x, y);
        tsdf_ray_start(r, &s);
    }
    while (__ballot(s.status == TSDF_RAY_LIVE) != 0ull) {
        if (s.status == TSDF_RAY_LIVE) tsdf_ray_step(g.vol, g.view, r, g.tsdf, &s); // (at most max_steps + 1 turns: tsdf_ray.h)
    }
    if (in) {
        const TsdfRayPixel o = tsdf_ray_finish(g.vol, g.view, r, g.tsdf, g.color, s, g.normals != nullptr);
        const size_t at = (size_t)y * (size_t)g.view.W + (size_t)x;
        if (g.depth) g.depth[at] = o.depth;
        if (g.normals) g.normals[at] = make_float4(o.normal[0], o.normal[1], o.normal[2], o.normal[3]);
        if (g.bgr) {
            g.bgr[at * 3 + 0] = o.bgr[0];
            g.bgr[at * 3 + 1] = o.bgr[1];
            g.bgr[at * 3 + 2] = o.bgr[2];
        }
        if (g.status) g.status[at] = o.status;
    }
#pragma unroll
    for (uint32_t c = 0; c < 5; c++) {
        const uint32_t n = (uint32_t)__popcll(__ballot(in && s.status == c));
        if (lane == 0) s_cnt[c][wave] = n;
    }
    uint32_t v = s.count; // (at most 16384 per ray: a workgroup's sum stays below 2^23)
    for (int o = ADC_WAVE / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_down((int)v, o, ADC_WAVE);
    if (lane == 0) s_cnt[5][wave] = v;
    __syncthreads();
    if (threadIdx.x < 6) {
        uint32_t t = 0;
        for (int w = 0; w < TSDF_RAY_WAVES; w++) t += s_cnt[threadIdx.x][w];
        if (t && threadIdx.x < 5) atomicAdd(&g.rep[1 + threadIdx.x], t);
        if (t && threadIdx.x == 5) atomicAdd(reinterpret_cast<unsigned long long*>(g.rep + 6), (unsigned long long)t);
    }
    if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) g.rep[0] = (uint32_t)g.view.W * (uint32_t)g.view.H; // (nobody adds to this word)
}

hipError_t adc_launch_tsdf_raycast(adc_handle* h, const AdcTsdfRayReq& r)
{
    if (!h->tsdf_vol || !h->tsdf_rep || (r.bgr && !h->tsdf_col)) return hipErrorInvalidValue;
    TsdfRayArgs g;
    g.vol = tsdf_vol(h->tsdf_params);
    g.view = tsdf_ray_view(r.view, h->tsdf_params);
    g.tsdf = h->tsdf_vol;
    g.color = r.bgr ? h->tsdf_col : nullptr;
    g.depth = r.depth;
    g.normals = reinterpret_cast<float4*>(r.normals);
    g.bgr = r.bgr;
    g.status = r.status;
    g.rep = h->tsdf_rep + ADC_TSDF_REP_RAY;
    const dim3 grid((unsigned)((g.view.W + TSDF_RAY_TILE - 1) / TSDF_RAY_TILE), (unsigned)((g.view.H + TSDF_RAY_TILE - 1) / TSDF_RAY_TILE));
    hipLaunchKernelGGL(k_tsdf_raycast, grid, dim3(TSDF_RAY_WG), 0, h->stream, g);
    return hipGetLastError();
}
