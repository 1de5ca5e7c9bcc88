// k_rectify.hip -- optional rectification of raw camera images in front of the Match (adc_set_rectify_maps / adc_set_rectify_model,
// include/adcensus_c_api.h; the definition is tests/rectify_ref.py, which these kernels match bit for bit).
//
//   k_rect_model_maps   once per set call: the float32 maps of one camera model (one rounding per operation, fixed order)
//   k_rect_pack         once per set call: float maps -> the 8-byte record of every destination pixel + the valid byte map.  The
//                       outside test and the quantisation to 1/32 pixel happen here: the hot kernel has no float operation
//   k_rect_remap<FMT>   per image: gather of four taps with integer bilinear weights, 4 destination pixels per lane, 12 packed
//                       output bytes per lane.  A wave whose records are all flagged "four taps inside" runs without bounds tests
//   k_rect_remap_raw<K> the same gather for the camera layouts (16-bit gray, Bayer, YUYV / UYVY, NV12): the decode to the virtual
//                       B, G, R source image sits behind the tap.  Bayer loads the 4 x 4 window around the four taps once and
//                       demosaics the inner 2 x 2 from it; its fast path also needs the one-pixel ring inside (second record flag)
//   k_rect_convert<K>   conversion only (adc_set_input_format): the decode alone, W x H -> W x H, no records, no valid map
//
// Record (uint2): .x = (xi & 0xffff) | yi << 16 (int16 each), .y = ax | ay << 8 | flags << 16.  An outside pixel gets xi = yi = -32768,
// ax = ay = 0: every tap is out of the source, so the guarded path writes the definition's zeros without a case of its own.
// No workgroup waits for another one, no atomics; all writes are plain vector stores.
#include "adc_internal.h"

#define RECT_ALL_INSIDE 1u  // record flag: the four taps lie inside the source image
#define RECT_RING_INSIDE 2u // record flag: so does the one-pixel ring around them (the 4 x 4 window of the Bayer decode)

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
        if (x0 && x1 && y0 && y1) flags = RECT_ALL_INSIDE | ((xi >= 1 && xi + 2 < Ws && yi >= 1 && yi + 2 < Hs) ? RECT_RING_INSIDE : 0u);
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

// ------------------------------------------------------------------------------ camera layouts (include/adcensus_c_api.h has the
// formulas, tests/rawfmt_ref.py is the definition).  A kind is the decode of one or more format codes; kinds 0..3 are the codes of the
// four 8-bit layouts above.  p0 / p1: Bayer -- column / row parity of the red sites; YUV 4:2:2 -- byte offset of Y within a pixel's
// two bytes / of U within a pair's four (V two bytes behind U)
enum { RK_GRAY16 = 4, RK_BAYER8 = 5, RK_BAYER16 = 6, RK_YUV422 = 7, RK_NV12 = 8 };
struct RectSrc { int Ws, Hs, pitch, shift, p0, p1; };

__device__ __forceinline__ int rect_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int rect_s16(const uint8_t* __restrict__ p, int shift) // (p is even: pitch and base address are)
{
    const int v = (int)*reinterpret_cast<const uint16_t*>(p) >> shift;
    return v > 255 ? 255 : v;
}
__device__ __forceinline__ void rect_yuv(int Y, int U, int V, int& b, int& g, int& r) // BT.601, limited range
{
    const int c = 298 * (Y - 16) + 128, d = U - 128, e = V - 128;
    r = rect_clip8((c + 409 * e) >> 8);
    g = rect_clip8((c - 100 * d - 208 * e) >> 8);
    b = rect_clip8((c + 516 * d) >> 8);
}

// V[y][x] of every kind but Bayer; (y, x) inside the source
template <int K>
__device__ __forceinline__ void rect_decode(const uint8_t* __restrict__ src, const RectSrc& s, int y, int x, int& b, int& g, int& r)
{
    const uint8_t* row = src + (size_t)y * (size_t)s.pitch;
    if constexpr (K <= ADC_PIX_BGRA8) {
        constexpr int BPP = K == ADC_PIX_GRAY8 ? 1 : (K == ADC_PIX_BGRA8 ? 4 : 3);
        rect_tap<K>(row + (size_t)x * BPP, b, g, r);
    } else if (K == RK_GRAY16) {
        b = g = r = rect_s16(row + 2 * (size_t)x, s.shift);
    } else if (K == RK_YUV422) {
        const uint8_t* pair = row + 4 * (size_t)(x >> 1);
        rect_yuv(row[2 * (size_t)x + s.p0], pair[s.p1], pair[s.p1 + 2], b, g, r);
    } else { // RK_NV12: the chroma plane starts behind the Hs luma rows
        const uint8_t* uv = src + ((size_t)s.Hs + (size_t)(y >> 1)) * (size_t)s.pitch + 2 * (size_t)(x >> 1);
        rect_yuv(row[x], uv[0], uv[1], b, g, r);
    }
}

template <int K>
__device__ __forceinline__ int rect_bayer_s(const uint8_t* __restrict__ src, const RectSrc& s, int y, int x)
{
    const uint8_t* row = src + (size_t)y * (size_t)s.pitch;
    return K == RK_BAYER8 ? (int)row[x] : rect_s16(row + 2 * (size_t)x, s.shift);
}
// a coordinate reflected into [0, n) without repeating the edge; what lies further out than one pixel (the ring of a tap that is
// outside itself and contributes nothing) is only kept addressable
__device__ __forceinline__ int rect_reflect(int c, int n)
{
    c = c < 0 ? -c : c;
    c = c >= n ? 2 * (n - 1) - c : c;
    return c < 0 ? 0 : (c > n - 1 ? n - 1 : c);
}
// bilinear demosaic of window element (i, j), the site (y, x)
template <int R, int C>
__device__ __forceinline__ void rect_bayer_bgr(const int (&w)[R][C], int i, int j, int y, int x, const RectSrc& s, int& b, int& g, int& r)
{
    const int px = (x ^ s.p0) & 1, py = (y ^ s.p1) & 1; // 0, 0: a red site; 1, 1: a blue one
    const int own = w[i][j];
    const int hh = w[i][j - 1] + w[i][j + 1], vv = w[i - 1][j] + w[i + 1][j];
    if (px == py) {
        const int diag = (w[i - 1][j - 1] + w[i - 1][j + 1] + w[i + 1][j - 1] + w[i + 1][j + 1] + 2) >> 2;
        g = (hh + vv + 2) >> 2;
        r = px ? diag : own;
        b = px ? own : diag;
    } else { // a green site: in a red row the left / right neighbours are red
        g = own;
        r = py ? (vv + 1) >> 1 : (hh + 1) >> 1;
        b = py ? (hh + 1) >> 1 : (vv + 1) >> 1;
    }
}

template <int K, bool GUARD>
__device__ __forceinline__ uint32_t rect_pixel_raw(const uint8_t* __restrict__ src, uint2 rc, const RectSrc& s)
{
    const int xi = (int)(int16_t)(rc.x & 0xffffu), yi = (int)rc.x >> 16;
    const int ax = (int)(rc.y & 0xffu), ay = (int)((rc.y >> 8) & 0xffu);
    int sb = 512, sg = 512, sr = 512;
    int w[4][4];
    if constexpr (K == RK_BAYER8 || K == RK_BAYER16) { // rows yi - 1 .. yi + 2, columns xi - 1 .. xi + 2, once for the four taps
        int cx[4], cy[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            cx[k] = GUARD ? rect_reflect(xi - 1 + k, s.Ws) : xi - 1 + k;
            cy[k] = GUARD ? rect_reflect(yi - 1 + k, s.Hs) : yi - 1 + k;
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) w[i][j] = rect_bayer_s<K>(src, s, cy[i], cx[j]);
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int tx = xi + (t & 1), ty = yi + (t >> 1);
        const int wt = ((t & 1) ? ax : 32 - ax) * ((t >> 1) ? ay : 32 - ay);
        if (GUARD && !(tx >= 0 && tx < s.Ws && ty >= 0 && ty < s.Hs)) continue; // constant border, per tap
        int b, g, r;
        if constexpr (K == RK_BAYER8 || K == RK_BAYER16) rect_bayer_bgr<4, 4>(w, 1 + (t >> 1), 1 + (t & 1), ty, tx, s, b, g, r);
        else rect_decode<K>(src, s, ty, tx, b, g, r);
        sb += wt * b; sg += wt * g; sr += wt * r;
    }
    return (uint32_t)(sb >> 10) | ((uint32_t)(sg >> 10) << 8) | ((uint32_t)(sr >> 10) << 16);
}

// the 12 bytes of four pixels (ALIGNED), or n < 4 / unaligned ones byte by byte: shared by the two kernels below
template <bool ALIGNED>
__device__ __forceinline__ void rect_store(uint8_t* __restrict__ o, const uint32_t (&px)[4], int n)
{
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

// k_rect_remap's tile and record loads; the fast path of a Bayer kind wants both record flags
template <int K, bool ALIGNED>
__global__ __launch_bounds__(256) void k_rect_remap_raw(const uint8_t* __restrict__ src, const uint2* __restrict__ rec, uint8_t* __restrict__ out,
                                                        int W, int H, RectSrc s)
{
    constexpr uint32_t NEED = ((K == RK_BAYER8 || K == RK_BAYER16) ? (RECT_ALL_INSIDE | RECT_RING_INSIDE) : RECT_ALL_INSIDE) << 16;
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
    uint32_t all = NEED;
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < n) all &= rc[k].y;
    uint32_t px[4] = {0, 0, 0, 0};
    if (__all(!live || all == NEED)) {
#pragma unroll
        for (int k = 0; k < 4; k++) if (k < n) px[k] = rect_pixel_raw<K, false>(src, rc[k], s);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) if (k < n) px[k] = rect_pixel_raw<K, true>(src, rc[k], s);
    }
    if (!live) return;
    rect_store<ALIGNED>(out + i * 3, px, n);
}

// Conversion only: destination pixel (y, x) = V[y][x] (Ws == W, Hs == H), the same tile.  A Bayer lane loads the 3 x 6 window of its
// four pixels once, every coordinate reflected (the columns behind a tail of fewer than 4 pixels are only kept addressable)
template <int K, bool ALIGNED>
__global__ __launch_bounds__(256) void k_rect_convert(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, int W, int H, RectSrc s)
{
    const int lane_x = (int)(threadIdx.x & 15), row = (int)(threadIdx.x >> 4);
    const int x = (int)blockIdx.x * 64 + lane_x * 4, y = (int)blockIdx.y * 16 + row;
    if (!(x < W && y < H)) return;
    const int n = W - x < 4 ? W - x : 4;
    uint32_t px[4] = {0, 0, 0, 0};
    if constexpr (K == RK_BAYER8 || K == RK_BAYER16) {
        int w[3][6], cx[6], cy[3];
#pragma unroll
        for (int j = 0; j < 6; j++) cx[j] = rect_reflect(x - 1 + j, W);
#pragma unroll
        for (int i = 0; i < 3; i++) cy[i] = rect_reflect(y - 1 + i, H);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 6; j++) w[i][j] = rect_bayer_s<K>(src, s, cy[i], cx[j]);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) {
                int b, g, r;
                rect_bayer_bgr<3, 6>(w, 1, 1 + k, y, x + k, s, b, g, r);
                px[k] = (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
            }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) {
                int b, g, r;
                rect_decode<K>(src, s, y, x + k, b, g, r);
                px[k] = (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
            }
    }
    rect_store<ALIGNED>(out + ((size_t)y * W + x) * 3, px, n);
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

// format word -> kind and the kernel's description of the source; -1: not a layout
static int rect_kind(const adc_raw_format& f, RectSrc& d)
{
    const int code = adc_pix_code(f.format);
    d = RectSrc{f.width, f.height, f.pitch_bytes, adc_pix_shift(f.format), 0, 0};
    if (code >= ADC_PIX_BGR8 && code <= ADC_PIX_BGRA8) return code;
    if (code == ADC_PIX_GRAY16) return RK_GRAY16;
    if ((code >= ADC_PIX_BAYER_RGGB8 && code <= ADC_PIX_BAYER_BGGR8) || (code >= ADC_PIX_BAYER_RGGB16 && code <= ADC_PIX_BAYER_BGGR16)) {
        d.p0 = code & 1;        // red columns: RGGB, GBRG even; GRBG, BGGR odd
        d.p1 = (code >> 1) & 1; // red rows: RGGB, GRBG even; GBRG, BGGR odd
        return code < ADC_PIX_BAYER_RGGB16 ? RK_BAYER8 : RK_BAYER16;
    }
    if (code == ADC_PIX_YUYV) { d.p0 = 0; d.p1 = 1; return RK_YUV422; }
    if (code == ADC_PIX_UYVY) { d.p0 = 1; d.p1 = 0; return RK_YUV422; }
    if (code == ADC_PIX_NV12) return RK_NV12;
    return -1;
}

template <int K>
static void rect_remap_raw_launch(adc_handle* h, const AdcRectSide& s, const RectSrc& d, const uint8_t* raw, uint8_t* out)
{
    const dim3 grid((unsigned)((h->p.W + 63) / 64), (unsigned)((h->p.H + 15) / 16));
    const uint2* rec = reinterpret_cast<const uint2*>(s.rec);
    if ((h->p.W & 3) == 0 && ((uintptr_t)out & 3u) == 0) hipLaunchKernelGGL((k_rect_remap_raw<K, true>), grid, dim3(256), 0, h->stream, raw, rec, out, h->p.W, h->p.H, d);
    else hipLaunchKernelGGL((k_rect_remap_raw<K, false>), grid, dim3(256), 0, h->stream, raw, rec, out, h->p.W, h->p.H, d);
}

hipError_t adc_launch_rect_remap(adc_handle* h, int side, const uint8_t* raw, uint8_t* bgr_out)
{
    const AdcRectSide& s = h->rect[side];
    RectSrc d;
    switch (rect_kind(s.fmt, d)) {
    case ADC_PIX_BGR8: rect_remap_launch<ADC_PIX_BGR8>(h, s, raw, bgr_out); break;
    case ADC_PIX_RGB8: rect_remap_launch<ADC_PIX_RGB8>(h, s, raw, bgr_out); break;
    case ADC_PIX_GRAY8: rect_remap_launch<ADC_PIX_GRAY8>(h, s, raw, bgr_out); break;
    case ADC_PIX_BGRA8: rect_remap_launch<ADC_PIX_BGRA8>(h, s, raw, bgr_out); break;
    case RK_GRAY16: rect_remap_raw_launch<RK_GRAY16>(h, s, d, raw, bgr_out); break;
    case RK_BAYER8: rect_remap_raw_launch<RK_BAYER8>(h, s, d, raw, bgr_out); break;
    case RK_BAYER16: rect_remap_raw_launch<RK_BAYER16>(h, s, d, raw, bgr_out); break;
    case RK_YUV422: rect_remap_raw_launch<RK_YUV422>(h, s, d, raw, bgr_out); break;
    case RK_NV12: rect_remap_raw_launch<RK_NV12>(h, s, d, raw, bgr_out); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int K>
static void rect_convert_launch(adc_handle* h, const RectSrc& d, const uint8_t* raw, uint8_t* out)
{
    const dim3 grid((unsigned)((h->p.W + 63) / 64), (unsigned)((h->p.H + 15) / 16));
    if ((h->p.W & 3) == 0 && ((uintptr_t)out & 3u) == 0) hipLaunchKernelGGL((k_rect_convert<K, true>), grid, dim3(256), 0, h->stream, raw, out, h->p.W, h->p.H, d);
    else hipLaunchKernelGGL((k_rect_convert<K, false>), grid, dim3(256), 0, h->stream, raw, out, h->p.W, h->p.H, d);
}

hipError_t adc_launch_rect_convert(adc_handle* h, int side, const uint8_t* raw, uint8_t* bgr_out)
{
    const AdcRectSide& s = h->rect[side];
    RectSrc d;
    const int kind = rect_kind(s.fmt, d);
    if (d.Ws != h->p.W || d.Hs != h->p.H) return hipErrorInvalidValue; // (the kernel indexes the source by the destination's pixel)
    switch (kind) {
    case ADC_PIX_BGR8: rect_convert_launch<ADC_PIX_BGR8>(h, d, raw, bgr_out); break;
    case ADC_PIX_RGB8: rect_convert_launch<ADC_PIX_RGB8>(h, d, raw, bgr_out); break;
    case ADC_PIX_GRAY8: rect_convert_launch<ADC_PIX_GRAY8>(h, d, raw, bgr_out); break;
    case ADC_PIX_BGRA8: rect_convert_launch<ADC_PIX_BGRA8>(h, d, raw, bgr_out); break;
    case RK_GRAY16: rect_convert_launch<RK_GRAY16>(h, d, raw, bgr_out); break;
    case RK_BAYER8: rect_convert_launch<RK_BAYER8>(h, d, raw, bgr_out); break;
    case RK_BAYER16: rect_convert_launch<RK_BAYER16>(h, d, raw, bgr_out); break;
    case RK_YUV422: rect_convert_launch<RK_YUV422>(h, d, raw, bgr_out); break;
    case RK_NV12: rect_convert_launch<RK_NV12>(h, d, raw, bgr_out); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
