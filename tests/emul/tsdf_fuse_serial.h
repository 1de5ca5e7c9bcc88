// tsdf_fuse_serial.h -- adcensus_amd/csrc/tsdf_fuse.h walked serially, one pixel and one voxel at a time: the observation weights and
// the weighted fuse of include/adcensus_c_api.h (adc_tsdf_weights, adc_tsdf_fuse) on the host, for tests/emul/emul_tsdf_fuse.cpp and
// tests/sanitize/stub_capi_tsdf_fuse.cpp.
#pragma once
#include <cstring>

#include "../../adcensus_amd/csrc/tsdf_fuse.h"

// prov and conf may be null
inline void tsdf_weights_serial(const float* map, const uint8_t* prov, const float* conf, const adc_tsdf_frame& f, const adc_tsdf_weight_params& p, int W, int H,
                                uint8_t* weight, adc_tsdf_weight_report* rep)
{
    const RegSource src = tsdf_cam(f, W, H).src;
    memset(rep, 0, sizeof(*rep));
    for (size_t n = 0; n < (size_t)W * H; n++) {
        bool below = false;
        const int w = tsdf_obs_weight(src, p, map[n], prov != nullptr, prov ? (uint32_t)prov[n] : 0u, conf != nullptr, conf ? conf[n] : 0.0f, &below);
        weight[n] = (uint8_t)(w < 0 ? 0 : w);
        rep->valid += w >= 0 ? 1u : 0u;
        rep->nonzero += w > 0 ? 1u : 0u;
        rep->below_confidence += below ? 1u : 0u;
        rep->saturated += w == 255 ? 1u : 0u;
    }
}

// color, img and weight may be null (img only with color); the volume is updated in place
inline void tsdf_fuse_serial(uint32_t* tsdf, uint32_t* color, const adc_tsdf_params& p, const adc_tsdf_frame& f, const adc_tsdf_fuse_params& fp, const float* map,
                             const uint8_t* img, const uint8_t* weight, int W, int H, adc_tsdf_fuse_report* rep)
{
    const TsdfVol v = tsdf_vol(p);
    const TsdfCam c = tsdf_cam(f, W, H);
    const bool bilinear = (fp.flags & ADC_TSDF_FUSE_BILINEAR) != 0;
    memset(rep, 0, sizeof(*rep));
    for (int k = 0; k < v.nz; k++)
        for (int j = 0; j < v.ny; j++) {
            const TsdfRow r = tsdf_row(v, c, j, k);
            for (int i = 0; i < v.nx; i++) {
                const size_t n = ((size_t)k * v.ny + j) * v.nx + i;
                int q = 0, pixel = 0;
                uint32_t wo = 0;
                bool band = false, interp = false;
                const int code = tsdf_fuse_decide(v, c, r, i, map, weight, bilinear, fp.interp_gap, &q, &pixel, &band, &wo, &interp);
                if (code == TSDF_SKIP) continue;
                rep->in_frustum++;
                rep->interpolated += interp ? 1u : 0u;
                if (code == TSDF_NO_DEPTH) rep->no_depth++;
                else if (code == TSDF_UNWEIGHTED) rep->unweighted++;
                else if (code == TSDF_OCCLUDED) rep->occluded++;
                else {
                    rep->updated++;
                    tsdf[n] = tsdf_fuse_update(tsdf[n], q, wo, v.max_weight);
                    if (color && img && band) color[n] = tsdf_colour_update(color[n], img + (size_t)pixel * 3, v.max_weight);
                }
            }
        }
}
