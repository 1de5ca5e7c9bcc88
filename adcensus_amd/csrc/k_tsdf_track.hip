// k_tsdf_track.hip -- frame-to-model camera tracking (include/adcensus_c_api.h: adc_track_device; the rule is tsdf_track.h, shared with
// the serial programs of the tests).  An entry point enqueues `iterations` pairs of the two kernels below up front; both begin with a
// wave-uniform read of the state's `done` word and return at once when a terminal status has set it, so the surplus launches of a
// track that ended early are no-ops and the loop never returns to the host.
//
//   k_track_reduce  A lane owns a participating pixel at a time, in a grid-stride loop, and keeps the 28 int64 sums and the seven
//                   counts of its pixels in registers (plain long long: the compiler's 64-bit adds and 32 x 32 -> 64 multiplies).
//                   Behind the loop: inside the wave by shuffles (two 32-bit cross-lane moves per 64-bit value and step), across
//                   the four waves of the workgroup through LDS, then one no-return 64-bit integer atomic add per sum that is not
//                   zero and workgroup.  The grid is capped at TRACK_GRID_PER_CU workgroups per CU of the device (1024 on an MI355X), so a
//                   pass issues at most 35 * 1024 atomics there, whatever the frame's size.  The gathers into the model maps go through the
//                   caches: for small motions neighbouring lanes read neighbouring model pixels.
//   k_track_solve   One workgroup, one working lane: track_solve (binary64) on the sums, the new float pose and the iteration record
//                   into the state, the sums and counts cleared for the next pass, `done` set on a terminal status.
// No float reaches an address (track_pixel clips the model pixel in integers before any load); every sum is an integer: no result
// depends on the order of the waves.
#include "adc_internal.h"
#include "tsdf_track.h"

#define TRACK_WG 256
#define TRACK_WAVES (TRACK_WG / ADC_WAVE)
#define TRACK_GRID_PER_CU 4 // workgroups per CU of the device (h->track_cus), at most: 1024 on the 256 CUs of an MI355X
static_assert(ADC_WAVE == 64 && TRACK_WAVES == 4, "four waves of 64 lanes");
static_assert(sizeof(((AdcTrackState*)0)->sums) == TRACK_SUMS * sizeof(long long) && TRACK_COUNTS <= 8, "the state holds the sums of tsdf_track.h");

struct TrackArgs {
    TrackFrame f;
    TrackModel m;
    TrackGate g;
    TrackPose guess;         // the estimate of pass 0; later passes read the state's
    adc_track_params p;
    const float* map;
    const float* fnormals;   // may be null
    const float* mdepth;
    const float* mnormals;
    AdcTrackState* st;
    uint32_t pixels, iter;
};

__device__ __forceinline__ TrackPose track_current(const TrackArgs& a)
{
    TrackPose k = a.guess;
    if (a.iter != 0u) {
        for (int i = 0; i < 9; i++) k.R[i] = a.st->res.R[i];
        for (int i = 0; i < 3; i++) k.t[i] = a.st->res.t[i];
    }
    return k;
}

__global__ __launch_bounds__(TRACK_WG) void k_track_reduce(const TrackArgs a)
{
    __shared__ long long s_sum[TRACK_WAVES][TRACK_SUMS];
    __shared__ uint32_t s_cnt[TRACK_WAVES][8];
    if (a.st->done != 0u) return; // (one address for the whole grid: every wave takes the same way)
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const TrackPose k = track_current(a);
    long long S[TRACK_SUMS];
    uint32_t c[TRACK_COUNTS];
#pragma unroll
    for (int i = 0; i < TRACK_SUMS; i++) S[i] = 0;
#pragma unroll
    for (int i = 0; i < TRACK_COUNTS; i++) c[i] = 0u;
    for (uint32_t p = blockIdx.x * TRACK_WG + threadIdx.x; p < a.pixels; p += gridDim.x * TRACK_WG) { // (pixels <= 2^26, the grid 1024 lanes per CU: no wrap)
        int x, y, q[7];
        track_pixel_of(a.f, a.g, p, &x, &y);
        const int what = track_pixel(a.f, a.m, a.g, k, x, y, a.map, a.fnormals, a.mdepth, a.mnormals, q);
        if (what == TRACK_USED) track_accumulate(q, S);
#pragma unroll
        for (int i = 0; i < TRACK_COUNTS; i++) c[i] += what == i ? 1u : 0u;
    }
#pragma unroll
    for (int i = 0; i < TRACK_SUMS; i++) {
        long long v = S[i];
        for (int o = ADC_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, ADC_WAVE);
        if (lane == 0) s_sum[wave][i] = v;
    }
#pragma unroll
    for (int i = 0; i < TRACK_COUNTS; i++) {
        uint32_t v = c[i];
        for (int o = ADC_WAVE / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_down((int)v, o, ADC_WAVE);
        if (lane == 0) s_cnt[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < TRACK_SUMS) {
        long long t = 0;
        for (int w = 0; w < TRACK_WAVES; w++) t += s_sum[w][threadIdx.x];
        if (t != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&a.st->sums[threadIdx.x]), (unsigned long long)t); // (two's complement: the sum of the signed values)
    } else if (threadIdx.x >= ADC_WAVE && threadIdx.x < ADC_WAVE + TRACK_COUNTS) {
        const int i = (int)threadIdx.x - ADC_WAVE;
        uint32_t t = 0;
        for (int w = 0; w < TRACK_WAVES; w++) t += s_cnt[w][i];
        if (t != 0u) atomicAdd(&a.st->counts[i], t);
    }
}

__global__ __launch_bounds__(ADC_WAVE) void k_track_solve(const TrackArgs a)
{
    if (a.st->done != 0u) return;
    if (threadIdx.x != 0) return;
    const TrackPose k = track_current(a);
    long long S[TRACK_SUMS];
    uint32_t c[TRACK_COUNTS];
    for (int i = 0; i < TRACK_SUMS; i++) { S[i] = a.st->sums[i]; a.st->sums[i] = 0; }
    for (int i = 0; i < TRACK_COUNTS; i++) { c[i] = a.st->counts[i]; a.st->counts[i] = 0u; }
    if (track_solve(S, c, a.pixels, a.p, a.m, k, a.iter, &a.st->res)) a.st->done = 1u;
}

static TrackArgs track_args(adc_handle* h, const AdcTrackReq& r, uint32_t iter)
{
    TrackArgs a;
    a.f = track_frame(r.frame, h->p.W, h->p.H);
    a.m = track_model(r.model);
    a.g = track_gate(r.params);
    a.guess = track_guess(r.frame);
    a.p = r.params;
    a.map = r.map; a.fnormals = r.fnormals; a.mdepth = r.mdepth; a.mnormals = r.mnormals;
    a.st = h->track_state;
    a.pixels = track_span(h->p.W, r.params.stride) * track_span(h->p.H, r.params.stride);
    a.iter = iter;
    return a;
}

hipError_t adc_launch_track_reduce(adc_handle* h, const AdcTrackReq& r, uint32_t iter)
{
    if (!h->track_state || !r.map || !r.mdepth || !r.mnormals) return hipErrorInvalidValue;
    const TrackArgs a = track_args(h, r, iter);
    const uint32_t want = (a.pixels + TRACK_WG - 1u) / TRACK_WG;
    const uint32_t cap = (uint32_t)TRACK_GRID_PER_CU * (uint32_t)(h->track_cus > 0 ? h->track_cus : 256);
    hipLaunchKernelGGL(k_track_reduce, dim3(want < cap ? want : cap), dim3(TRACK_WG), 0, h->stream, a);
    return hipGetLastError();
}

hipError_t adc_launch_track_solve(adc_handle* h, const AdcTrackReq& r, uint32_t iter)
{
    if (!h->track_state) return hipErrorInvalidValue;
    const TrackArgs a = track_args(h, r, iter);
    hipLaunchKernelGGL(k_track_solve, dim3(1), dim3(ADC_WAVE), 0, h->stream, a);
    return hipGetLastError();
}
