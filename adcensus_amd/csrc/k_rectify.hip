// k_rectify.hip -- optional rectification of raw camera images in front of the Match (adc_set_rectify_maps / adc_set_rectify_model,
// include/adcensus_c_api.h; the definition is tests/rectify_ref.py, which these kernels match bit for bit).
//
//   k_rect_model_maps   once per set call: the float32 maps of one camera model (one rounding per operation, fixed order)
//   k_rect_pack         once per set call: float maps -> the 8-byte record of every destination pixel + the valid byte map.  The
//                       outside test and the quantisation to 1/32 pixel happen here: the hot kernel has no float operation
//   k_rect_remap<FMT>   per image: gather of four taps with integer bilinear weights, 4 destination pixels per lane, 12 packed
//                       output bytes per lane.  A wave whose records are all flagged "four taps inside" runs without bounds tests
//
// Record (uint2): .x = (xi & 0xffff) | yi << 16 (int16 each), .y = ax | ay << 8 | flags << 16.  An outside pixel gets xi = yi = -32768,
// ax = ay = 0: every tap is out of the source, so the guarded path writes the definition's zeros without a case of its own.
// No workgroup waits for another one, no atomics; all writes are plain vector stores.
#include "adc_internal.h"

#define RECT_ALL_INSIDE 1u // record flag: the four taps lie inside the source image

__global__ __launch_bounds__(256) void k_rect_model_maps(float* __restrict__ mx_out, float* __restrict__ my_out, int W, int H, adc_camera_model m)
{
    const int x = (int)(blockIdx.x * 64 + (threadIdx.x & 63)), y = (int)(blockIdx.y * 4 + (threadIdx.x >> 6));
    if (x >= W || y >= H) return;
    const float u = (float)x, v = (float)y;
    const float xn = (u - m.new_cx) / m.new_fx, yn = (v - m.new_cy) / m.new_fy;
    const float X = (m.R[0] * xn + m.R[3] * yn) + m.R[6];
    const float Y = (m.R[1] * xn + m.R[4] * yn) + m.R[7];
    const float Wc = (m.R[2] * xn + m.R[5] * yn) + m.R[8];
    const float xx = X / Wc, yy = Y / Wc;
    const float x2 = xx * xx, y2 = yy * yy, r2 = x2 + y2, xy = xx * yy;
    const float rad = 1.0f + r2 * (m.k1 + r2 * (m.k2 + r2 * m.k3));
    const float xd = (xx * rad + (2.0f * m.p1) * xy) + m.p2 * (r2 + 2.0f * x2);
    const float yd = (yy * rad + m.p1 * (r2 + 2.0f * y2)) + (2.0f * m.p2) * xy;
    const size_t i = (size_t)y * W + x;
    mx_out[i] = m.fx * xd + m.cx;
    my_out[i] = m.fy * yd + m.cy;
}

__global__ __launch_bounds__(256) void k_rect_pack(const float* __restrict__ mx, const float* __restrict__ my, uint2* __restrict__ rec,
                                                   uint8_t* __restrict__ valid, int P, int Ws, int Hs)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float fx = mx[i], fy = my[i];
    int xi = -32768, yi = -32768, ax = 0, ay = 0;
    uint32_t flags = 0;
    uint8_t ok = 0;
    if (fabsf(fx) < 32768.f && fabsf(fy) < 32768.f) { // (false for NaN)
        const int X = (int)rintf(fx * 32.f), Y = (int)rintf(fy * 32.f);
        xi = X >> 5; ax = X & 31;
        yi = Y >> 5; ay = Y & 31;
        const bool x0 = xi >= 0 && xi < Ws, x1 = xi + 1 >= 0 && xi + 1 < Ws, y0 = yi >= 0 && yi < Hs, y1 = yi + 1 >= 0 && yi + 1 < Hs;
        if (x0 && x1 && y0 && y1) flags = RECT_ALL_INSIDE;
        ok = (x0 && y0 && (ax == 0 || x1) && (ay == 0 || y1)) ? 1 : 0; // every tap with a nonzero weight is inside
    }
    rec[i] = make_uint2(((uint32_t)xi & 0xffffu) | ((uint32_t)yi << 16), (uint32_t)ax | ((uint32_t)ay << 8) | (flags << 16));
    valid[i] = ok;
}

// one tap -> B | G << 8 | R << 16 ... kept as three ints (the weights reach 1024: 255 * 1024 needs 18 bits per channel)
template <int FMT>
__device__ __forceinline__ void rect_tap(const uint8_t* __restrict__ p, int& b, int& g, int& r)
{
    if (FMT == ADC_PIX_GRAY8) { b = g = r = p[0]; }
    else if (FMT == ADC_PIX_RGB8) { r = p[0]; g = p[1]; b = p[2]; }
    else { b = p[0]; g = p[1]; r = p[2]; } // BGR8, BGRA8 (alpha ignored)
}

template <int FMT, bool GUARD>
__device__ __forceinline__ uint32_t rect_pixel(const uint8_t* __restrict__ src, uint2 rc, int Ws, int Hs, int pitch)
{
    constexpr int BPP = FMT == ADC_PIX_GRAY8 ? 1 : (FMT == ADC_PIX_BGRA8 ? 4 : 3);
    const int xi = (int)(int16_t)(rc.x & 0xffffu), yi = (int)rc.x >> 16;
    const int ax = (int)(rc.y & 0xffu), ay = (int)((rc.y >> 8) & 0xffu);
    int sb = 512, sg = 512, sr = 512;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int tx = xi + (t & 1), ty = yi + (t >> 1);
        const int w = ((t & 1) ? ax : 32 - ax) * ((t >> 1) ? ay : 32 - ay);
        if (GUARD && !(tx >= 0 && tx < Ws && ty >= 0 && ty < Hs)) continue; // constant border, per tap
        int b, g, r;
        rect_tap<FMT>(src + (size_t)ty * (size_t)pitch + (size_t)tx * BPP, b, g, r);
        sb += w * b; sg += w * g; sr += w * r;
    }
    return (uint32_t)(sb >> 10) | ((uint32_t)(sg >> 10) << 8) | ((uint32_t)(sr >> 10) << 16);
}

// Tile of a workgroup: 64 x 16 destination pixels; a wave covers 64 x 4 (16 lanes x 4 pixels along x, 4 rows), so that its source
// footprint stays within a few rows of a smooth map.  ALIGNED (W % 4 == 0, out 4-byte aligned): records as two 16-byte loads, the
// 12 output bytes as three dword stores; otherwise 8-byte record loads and byte stores (and a tail of fewer than 4 pixels).
template <int FMT, bool ALIGNED>
__global__ __launch_bounds__(256) void k_rect_remap(const uint8_t* __restrict__ src, const uint2* __restrict__ rec, uint8_t* __restrict__ out,
                                                    int W, int H, int Ws, int Hs, int pitch)
{
    const int lane_x = (int)(threadIdx.x & 15), row = (int)(threadIdx.x >> 4);
    const int x = (int)blockIdx.x * 64 + lane_x * 4, y = (int)blockIdx.y * 16 + row;
    const bool live = x < W && y < H;
    const int n = live ? (W - x < 4 ? W - x : 4) : 0;
    const size_t i = (size_t)(live ? y : 0) * W + (live ? x : 0);
    uint2 rc[4];
    if (ALIGNED) {
        if (live) {
            const uint4 a = *reinterpret_cast<const uint4*>(rec + i), b = *reinterpret_cast<const uint4*>(rec + i + 2);
            rc[0] = make_uint2(a.x, a.y); rc[1] = make_uint2(a.z, a.w); rc[2] = make_uint2(b.x, b.y); rc[3] = make_uint2(b.z, b.w);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) if (k < n) rc[k] = rec[i + k];
    }
    uint32_t all = RECT_ALL_INSIDE << 16;
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < n) all &= rc[k].y;
    uint32_t px[4] = {0, 0, 0, 0};
    if (__all(!live || all != 0)) { // (wave-uniform: every tap of every live lane is inside the source)
#pragma unroll
        for (int k = 0; k < 4; k++) if (k < n) px[k] = rect_pixel<FMT, false>(src, rc[k], Ws, Hs, pitch);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) if (k < n) px[k] = rect_pixel<FMT, true>(src, rc[k], Ws, Hs, pitch);
    }
    if (!live) return;
    uint8_t* o = out + i * 3;
    if (ALIGNED) { // (n == 4)
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
        o4[0] = px[0] | (px[1] << 24);
        o4[1] = (px[1] >> 8) | (px[2] << 16);
        o4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) { o[3 * k] = (uint8_t)px[k]; o[3 * k + 1] = (uint8_t)(px[k] >> 8); o[3 * k + 2] = (uint8_t)(px[k] >> 16); }
    }
}

// ------------------------------------------------------------------------------ launchers (capi.hip orders them and owns every
// other HIP call of the path); all on the object stream
hipError_t adc_launch_rect_model_maps(adc_handle* h, int side, const adc_camera_model* m)
{
    const AdcRectSide& s = h->rect[side];
    hipLaunchKernelGGL(k_rect_model_maps, dim3((unsigned)((h->p.W + 63) / 64), (unsigned)((h->p.H + 3) / 4)), dim3(256), 0, h->stream, s.mx, s.my, h->p.W,
                       h->p.H, *m);
    return hipGetLastError();
}

hipError_t adc_launch_rect_pack(adc_handle* h, int side)
{
    const AdcRectSide& s = h->rect[side];
    const size_t P = (size_t)h->p.W * h->p.H;
    hipLaunchKernelGGL(k_rect_pack, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, s.mx, s.my, reinterpret_cast<uint2*>(s.rec), s.valid, (int)P,
                       s.fmt.width, s.fmt.height);
    return hipGetLastError();
}

template <int FMT>
static void rect_remap_launch(adc_handle* h, const AdcRectSide& s, const uint8_t* raw, uint8_t* out)
{
    const dim3 grid((unsigned)((h->p.W + 63) / 64), (unsigned)((h->p.H + 15) / 16));
    const uint2* rec = reinterpret_cast<const uint2*>(s.rec);
    if ((h->p.W & 3) == 0 && ((uintptr_t)out & 3u) == 0)
        hipLaunchKernelGGL((k_rect_remap<FMT, true>), grid, dim3(256), 0, h->stream, raw, rec, out, h->p.W, h->p.H, s.fmt.width, s.fmt.height, s.fmt.pitch_bytes);
    else
        hipLaunchKernelGGL((k_rect_remap<FMT, false>), grid, dim3(256), 0, h->stream, raw, rec, out, h->p.W, h->p.H, s.fmt.width, s.fmt.height, s.fmt.pitch_bytes);
}

hipError_t adc_launch_rect_remap(adc_handle* h, int side, const uint8_t* raw, uint8_t* bgr_out)
{
    const AdcRectSide& s = h->rect[side];
    switch (s.fmt.format) {
    case ADC_PIX_BGR8: rect_remap_launch<ADC_PIX_BGR8>(h, s, raw, bgr_out); break;
    case ADC_PIX_RGB8: rect_remap_launch<ADC_PIX_RGB8>(h, s, raw, bgr_out); break;
    case ADC_PIX_GRAY8: rect_remap_launch<ADC_PIX_GRAY8>(h, s, raw, bgr_out); break;
    case ADC_PIX_BGRA8: rect_remap_launch<ADC_PIX_BGRA8>(h, s, raw, bgr_out); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
