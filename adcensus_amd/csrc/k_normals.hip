// k_normals.hip -- surface normals from a disparity map: a windowed least-squares plane fit in (x, y, disparity), solved exactly in
// integers (include/adcensus_c_api.h: adc_normals_device; the arithmetic is normals_fit.h, the definition in numpy
// tests/normals_ref.py, which this kernel matches bit for bit).
//
//   k_normals   one tiled stencil kernel.  A workgroup of 256 lanes owns a tile of NRM_TW x NRM_TH = 64 x 16 output pixels.  It
//               quantises the tile plus a halo of r to int32 fixed point in LDS -- one sentinel (NRM_Q_NONE) stands for "not usable"
//               and for "outside the image", so the tap loop has no bounds tests -- and every lane then fits four pixels of one
//               column (rows wave, wave + 4, ...): nine int32 sums over the (2r+1)^2 taps, four 3x3 determinants in int64, a dozen
//               float operations, one 16-byte store (normals) and one 4-byte store (normals8).  The four report counts are ballots
//               reduced per wave and added with one atomic per count and workgroup.
//
// Tile shape: a wave is one row of 64 consecutive pixels, so a tap (dx, dy) is a ds_read_b32 of 64 consecutive dwords
// -- both 32-lane groups conflict-free whatever the row pitch -- and the stores of a wave are 1 KiB / 256 B contiguous.  16 rows keep
// the halo's share of the staged pixels at 2.3x for r = 7 (78 x 30 loaded for 64 x 16 written) and 1.3x for r = 2, in 9360 bytes of
// LDS (sized for r = 7 whatever the radius): 16 workgroups fit the 160 KiB of a CU, so the LDS never limits occupancy.
//
// The sums are accumulated row by row (five sums over a row's taps, folded into the nine with the row's dy): integer arithmetic is
// exact, so this is the definition's result in fewer operations per tap.
//
// Bounds: the staging loop reads map[gy * W + gx] only for 0 <= gx < W, 0 <= gy < H; LDS indices are < NRM_LH * NRM_LW by
// construction (r <= ADC_NORMALS_MAX_RADIUS is validated by the entry point); stores are guarded by x < W, y < H and indexed in size_t.
#include "adc_internal.h"
#include "adc_device_fn.h"
#include "normals_fit.h"

#define NRM_WG 256
#define NRM_WAVES (NRM_WG / ADC_WAVE)
#define NRM_TW 64
#define NRM_TH 16
#define NRM_LW (NRM_TW + 2 * ADC_NORMALS_MAX_RADIUS)
#define NRM_LH (NRM_TH + 2 * ADC_NORMALS_MAX_RADIUS)
static_assert(NRM_TW == ADC_WAVE, "a wave is one row of the tile");
static_assert(NRM_TW <= 128 && NRM_TH <= 64 && NRM_TH % NRM_WAVES == 0, "tile shape");

typedef float nrm_vf4 __attribute__((ext_vector_type(4)));

struct NrmArgs {
    NrmCam cam;
    const float* map;
    nrm_vf4* normals;   // may be NULL
    uint32_t* normals8; // may be NULL
    uint32_t* rep;      // [0] usable, [1] fitted, [2] few_points, [3] degenerate
    int W, H;
    int r, G, min_points;
};

__device__ __forceinline__ uint32_t nrm_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

__global__ __launch_bounds__(NRM_WG) void k_normals(const NrmArgs g)
{
    __shared__ int32_t s_q[NRM_LH * NRM_LW];
    __shared__ uint32_t s_cnt[4][NRM_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const int x0 = (int)blockIdx.x * NRM_TW, y0 = (int)blockIdx.y * NRM_TH;
    const int r = g.r, lw = NRM_TW + 2 * r, lh = NRM_TH + 2 * r;
    for (int ly = wave; ly < lh; ly += NRM_WAVES) {
        const int gy = y0 - r + ly;
        const bool row_in = gy >= 0 && gy < g.H;
        for (int lx = lane; lx < lw; lx += ADC_WAVE) {
            const int gx = x0 - r + lx;
            int32_t q = NRM_Q_NONE;
            if (row_in && gx >= 0 && gx < g.W) q = nrm_quantise(g.map[(size_t)gy * (size_t)g.W + (size_t)gx]);
            s_q[ly * NRM_LW + lx] = q;
        }
    }
    __syncthreads();
    uint32_t cnt[4] = {0, 0, 0, 0}; // wave-uniform
    const int x = x0 + lane;
    for (int ty = wave; ty < NRM_TH; ty += NRM_WAVES) {
        const int y = y0 + ty;
        if (y >= g.H) break; // (wave-uniform; no barrier below depends on it)
        const int32_t qc = s_q[(ty + r) * NRM_LW + lane + r];
        const bool in = x < g.W, usable = in && qc != NRM_Q_NONE;
        NrmSums s = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int dy = -r; dy <= r; dy++) {
            const int32_t* row = s_q + (ty + r + dy) * NRM_LW + lane;
            int32_t rn = 0, rsx = 0, rsxx = 0, rse = 0, rsxe = 0;
            for (int j = 0; j <= 2 * r; j++) {
                const int dx = j - r;
                const int32_t e = row[j] - qc;
                const bool ok = nrm_gate(e, g.G);
                const int32_t em = ok ? e : 0;
                rn += ok ? 1 : 0;
                rsx += ok ? dx : 0;
                rsxx += ok ? dx * dx : 0;
                rse += em;
                rsxe += dx * em;
            }
            s.n += rn; s.sx += rsx; s.sxx += rsxx; s.se += rse; s.sxe += rsxe;
            s.sy += dy * rn; s.sxy += dy * rsx; s.syy += dy * dy * rn; s.sye += dy * rse;
        }
        NrmPixel o;
        o.v[0] = o.v[1] = o.v[2] = o.v[3] = 0.0f;
        o.bytes = 0;
        o.cls = NRM_UNUSABLE;
        if (usable) o = nrm_fit(s, qc, x, y, g.cam, g.min_points);
        cnt[0] += nrm_count(usable);
        cnt[1] += nrm_count(o.cls == NRM_FITTED);
        cnt[2] += nrm_count(o.cls == NRM_FEW_POINTS);
        cnt[3] += nrm_count(o.cls == NRM_DEGENERATE);
        if (in) {
            const size_t i = (size_t)y * (size_t)g.W + (size_t)x;
            if (g.normals) {
                nrm_vf4 v;
                v.x = o.v[0]; v.y = o.v[1]; v.z = o.v[2]; v.w = o.v[3];
                g.normals[i] = v;
            }
            if (g.normals8) g.normals8[i] = o.bytes;
        }
    }
    if (lane == 0) { s_cnt[0][wave] = cnt[0]; s_cnt[1][wave] = cnt[1]; s_cnt[2][wave] = cnt[2]; s_cnt[3][wave] = cnt[3]; }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t t = 0;
        for (int w = 0; w < NRM_WAVES; w++) t += s_cnt[threadIdx.x][w];
        if (t) atomicAdd(&g.rep[threadIdx.x], t);
    }
}

hipError_t adc_launch_normals(adc_handle* h, const float* disp, const adc_calib* calib, int radius, int32_t G, int min_points, float* normals, uint8_t* normals8)
{
    if (radius < 1 || radius > ADC_NORMALS_MAX_RADIUS || G < 0 || G > 65536) return hipErrorInvalidValue; // (the LDS tile and the int32 sums are sized for these)
    NrmArgs g;
    g.cam.focal = calib->focal_px; g.cam.cx = calib->cx; g.cam.cy = calib->cy; g.cam.doffs = calib->doffs;
    g.map = disp;
    g.normals = reinterpret_cast<nrm_vf4*>(normals);
    g.normals8 = reinterpret_cast<uint32_t*>(normals8);
    g.rep = h->nrm_rep;
    g.W = h->p.W; g.H = h->p.H;
    g.r = radius; g.G = G; g.min_points = min_points;
    const dim3 grid((unsigned)((g.W + NRM_TW - 1) / NRM_TW), (unsigned)((g.H + NRM_TH - 1) / NRM_TH));
    hipLaunchKernelGGL(k_normals, grid, dim3(NRM_WG), 0, h->stream, g);
    return hipGetLastError();
}
