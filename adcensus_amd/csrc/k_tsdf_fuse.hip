// k_tsdf_fuse.hip -- the stereo-aware TSDF fusion (include/adcensus_c_api.h: adc_tsdf_weights_device, adc_tsdf_fuse_device; the rule
// is tsdf_fuse.h).
//
//   k_tsdf_obs_weight  the pixels of the map in raster order, a lane striding over them by the size of the grid (at most
//                      TSDF_WEIGHT_MAX_WG workgroups): one float (and, when given, one provenance byte and one confidence float) in,
//                      one byte out, so a wave reads and writes whole contiguous runs whatever W is; a pure function of the pixel.  Per
//                      workgroup one integer atomic per report count.
//   k_tsdf_fuse        the form of k_tsdf_integrate (k_tsdf.hip): a lane owns FOUR consecutive voxels of a row, a wave 256 voxels of a
//                      row and TSDF_ROWS_PER_WAVE rows; the projection and the decision come first, and a lane loads and stores its
//                      16-byte group of voxel words only when one of its four voxels is updated.  The weight byte is read behind the
//                      nearest pixel's validity, the four taps only behind a non-zero weight and the integer clip.  The bilinear
//                      switch and the presence of a weight map are template arguments: the plain form carries none of the tap code,
//                      and without a weight map the update is tsdf_update itself (step 9' with wo = 1 is step 9), with no 64-bit
//                      arithmetic.
// Every count is an integer and every voxel and pixel has one owner: no result depends on the order of the waves.
#include "adc_internal.h"
#include "tsdf_fuse.h"

#define TSDF_WG 256
#define TSDF_WAVES (TSDF_WG / ADC_WAVE)
#define TSDF_ROWS_PER_WAVE 4
#define TSDF_ROW_VOXELS (ADC_WAVE * 4) // voxels of a row one wave covers
#define TSDF_FUSE_COUNTS 6
#define TSDF_WEIGHT_COUNTS 4
#define TSDF_WEIGHT_MAX_WG 1024 // workgroups of the weight pass at most (four per CU of an MI355X): a lane strides over the map

// the counts of a workgroup's lanes added to rep[0 .. N); every lane of the workgroup calls it
template <int N>
__device__ __forceinline__ void tsdf_fuse_report(uint32_t (&cnt)[N], uint32_t* rep)
{
    __shared__ uint32_t s_cnt[N][TSDF_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
#pragma unroll
    for (int c = 0; c < N; c++) {
        uint32_t v = cnt[c];
        for (int o = ADC_WAVE / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_down((int)v, o, ADC_WAVE);
        if (lane == 0) s_cnt[c][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        uint32_t t = 0;
        for (int w = 0; w < TSDF_WAVES; w++) t += s_cnt[threadIdx.x][w];
        if (t) atomicAdd(&rep[threadIdx.x], t);
    }
}

struct TsdfWeightArgs {
    RegSource src;
    adc_tsdf_weight_params par;
    const float* map;
    const uint8_t* prov;    // may be null
    const float* conf;      // may be null
    uint8_t* weight;
    uint32_t* rep;          // [0] valid [1] nonzero [2] below_confidence [3] saturated
    int P;                  // pixels
};

__global__ __launch_bounds__(TSDF_WG) void k_tsdf_obs_weight(const TsdfWeightArgs g)
{
    const int stride = (int)gridDim.x * TSDF_WG;
    uint32_t cnt[TSDF_WEIGHT_COUNTS] = {0u, 0u, 0u, 0u};
    for (int n = (int)(blockIdx.x * TSDF_WG + threadIdx.x); n < g.P; n += stride) { // (P + stride stays below 2^31: P <= 2^24 pixels, the grid is capped)
        bool below = false;
        const int w = tsdf_obs_weight(g.src, g.par, g.map[n], g.prov != nullptr, g.prov ? (uint32_t)g.prov[n] : 0u, g.conf != nullptr, g.conf ? g.conf[n] : 0.0f, &below);
        g.weight[n] = (uint8_t)(w < 0 ? 0 : w);
        cnt[0] += w >= 0 ? 1u : 0u;
        cnt[1] += w > 0 ? 1u : 0u;
        cnt[2] += below ? 1u : 0u;
        cnt[3] += w == 255 ? 1u : 0u;
    }
    tsdf_fuse_report<TSDF_WEIGHT_COUNTS>(cnt, g.rep);
}

struct TsdfFuseArgs {
    TsdfVol vol;
    TsdfCam cam;
    const float* map;
    const uint8_t* img;     // may be null
    const uint8_t* weight;  // may be null: 1 everywhere
    float gap;
    uint32_t* tsdf;
    uint32_t* color;        // may be null
    uint32_t* rep;          // [0] in_frustum [1] no_depth [2] unweighted [3] occluded [4] updated [5] interpolated
    int xchunks, rows;      // 256-voxel pieces of a row; rows = ny * nz
};

template <bool BILINEAR, bool WEIGHTED>
__global__ __launch_bounds__(TSDF_WG) void k_tsdf_fuse(const TsdfFuseArgs g)
{
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const int xc = (int)(blockIdx.x % (unsigned)g.xchunks), rb = (int)(blockIdx.x / (unsigned)g.xchunks);
    const int i0 = xc * TSDF_ROW_VOXELS + lane * 4;
    const bool in = i0 < g.vol.nx; // (nx is a multiple of 4: all four voxels or none)
    const bool with_colour = g.color != nullptr && g.img != nullptr;
    uint32_t cnt[TSDF_FUSE_COUNTS] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll 1
    for (int r = 0; r < TSDF_ROWS_PER_WAVE; r++) {
        const int row = (rb * TSDF_WAVES + wave) * TSDF_ROWS_PER_WAVE + r;
        if (row >= g.rows || !in) continue;
        const int k = row / g.vol.ny, j = row - k * g.vol.ny;
        const TsdfRow rt = tsdf_row(g.vol, g.cam, j, k);
        int code[4], q[4], pixel[4];
        uint32_t wo[4];
        bool band[4], any = false, any_colour = false;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            bool interp = false;
            q[e] = 0; pixel[e] = 0; band[e] = false; wo[e] = 0u;
            code[e] = tsdf_fuse_decide(g.vol, g.cam, rt, i0 + e, g.map, WEIGHTED ? g.weight : nullptr, BILINEAR, g.gap, &q[e], &pixel[e], &band[e], &wo[e], &interp);
            cnt[0] += code[e] != TSDF_SKIP ? 1u : 0u;
            cnt[1] += code[e] == TSDF_NO_DEPTH ? 1u : 0u;
            cnt[2] += code[e] == TSDF_UNWEIGHTED ? 1u : 0u;
            cnt[3] += code[e] == TSDF_OCCLUDED ? 1u : 0u;
            cnt[4] += code[e] == TSDF_UPDATE ? 1u : 0u;
            cnt[5] += interp ? 1u : 0u;
            any = any || code[e] == TSDF_UPDATE;
            any_colour = any_colour || (code[e] == TSDF_UPDATE && band[e]);
        }
        if (!any) continue;
        const size_t at = (size_t)row * (size_t)g.vol.nx + (size_t)i0;
        uint4* pw = reinterpret_cast<uint4*>(g.tsdf + at);
        uint4 w4 = *pw;
        uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (code[e] == TSDF_UPDATE) w[e] = WEIGHTED ? tsdf_fuse_update(w[e], q[e], wo[e], g.vol.max_weight) : tsdf_update(w[e], q[e], g.vol.max_weight); // (wo == 1: step 9)
        w4.x = w[0]; w4.y = w[1]; w4.z = w[2]; w4.w = w[3];
        *pw = w4;
        if (with_colour && any_colour) {
            uint4* pc = reinterpret_cast<uint4*>(g.color + at);
            uint4 c4 = *pc;
            uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (code[e] == TSDF_UPDATE && band[e]) c[e] = tsdf_colour_update(c[e], g.img + (size_t)pixel[e] * 3, g.vol.max_weight);
            c4.x = c[0]; c4.y = c[1]; c4.z = c[2]; c4.w = c[3];
            *pc = c4;
        }
    }
    tsdf_fuse_report<TSDF_FUSE_COUNTS>(cnt, g.rep);
}

hipError_t adc_launch_tsdf_weights(adc_handle* h, const AdcTsdfWeightReq& r)
{
    if (!h->tsdfw_rep || !r.map || !r.weight) return hipErrorInvalidValue;
    TsdfWeightArgs g;
    g.src = tsdf_cam(r.frame, h->p.W, h->p.H).src;
    g.par = r.params;
    g.map = r.map;
    g.prov = r.prov;
    g.conf = r.conf;
    g.weight = r.weight;
    g.rep = h->tsdfw_rep;
    g.P = h->p.W * h->p.H;
    const int blocks = (g.P + TSDF_WG - 1) / TSDF_WG;
    hipLaunchKernelGGL(k_tsdf_obs_weight, dim3((unsigned)(blocks < TSDF_WEIGHT_MAX_WG ? blocks : TSDF_WEIGHT_MAX_WG)), dim3(TSDF_WG), 0, h->stream, g);
    return hipGetLastError();
}

hipError_t adc_launch_tsdf_fuse(adc_handle* h, const AdcTsdfFuseReq& r)
{
    if (!h->tsdf_vol || !h->tsdf_rep || !r.map) return hipErrorInvalidValue;
    TsdfFuseArgs g;
    g.vol = tsdf_vol(h->tsdf_params);
    g.cam = tsdf_cam(r.frame, h->p.W, h->p.H);
    g.map = r.map;
    g.img = r.img;
    g.weight = r.weight;
    g.gap = r.params.interp_gap;
    g.tsdf = h->tsdf_vol;
    g.color = h->tsdf_col;
    g.rep = h->tsdf_rep + ADC_TSDF_REP_FUSE;
    g.xchunks = (g.vol.nx + TSDF_ROW_VOXELS - 1) / TSDF_ROW_VOXELS;
    g.rows = g.vol.ny * g.vol.nz;
    const int rows_per_wg = TSDF_WAVES * TSDF_ROWS_PER_WAVE;
    const unsigned blocks = (unsigned)g.xchunks * (unsigned)((g.rows + rows_per_wg - 1) / rows_per_wg);
    const bool bilinear = (r.params.flags & ADC_TSDF_FUSE_BILINEAR) != 0, weighted = r.weight != nullptr;
    if (bilinear && weighted) hipLaunchKernelGGL((k_tsdf_fuse<true, true>), dim3(blocks), dim3(TSDF_WG), 0, h->stream, g);
    else if (bilinear) hipLaunchKernelGGL((k_tsdf_fuse<true, false>), dim3(blocks), dim3(TSDF_WG), 0, h->stream, g);
    else if (weighted) hipLaunchKernelGGL((k_tsdf_fuse<false, true>), dim3(blocks), dim3(TSDF_WG), 0, h->stream, g);
    else hipLaunchKernelGGL((k_tsdf_fuse<false, false>), dim3(blocks), dim3(TSDF_WG), 0, h->stream, g);
    return hipGetLastError();
}
