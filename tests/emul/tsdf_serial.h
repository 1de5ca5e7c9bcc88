// tsdf_serial.h -- adcensus_amd/csrc/tsdf_voxel.h walked serially over a whole volume, one voxel at a time: the TSDF volume of
// include/adcensus_c_api.h (adc_tsdf_integrate, adc_tsdf_extract) on the host, for tests/emul/emul_tsdf.cpp and
// tests/sanitize/stub_capi_tsdf.cpp.
#pragma once
#include <cstring>
#include <vector>

#include "../../adcensus_amd/csrc/tsdf_voxel.h"

// color and img may be null (img only with color); the volume is updated in place
inline void tsdf_integrate_serial(uint32_t* tsdf, uint32_t* color, const adc_tsdf_params& p, const adc_tsdf_frame& f, const float* map, const uint8_t* img, int W, int H,
                                  adc_tsdf_report* rep)
{
    const TsdfVol v = tsdf_vol(p);
    const TsdfCam c = tsdf_cam(f, W, H);
    memset(rep, 0, sizeof(*rep));
    for (int k = 0; k < v.nz; k++)
        for (int j = 0; j < v.ny; j++) {
            const TsdfRow r = tsdf_row(v, c, j, k);
            for (int i = 0; i < v.nx; i++) {
                const size_t n = ((size_t)k * v.ny + j) * v.nx + i;
                int q = 0, pixel = 0;
                bool band = false;
                const int code = tsdf_decide(v, c, r, i, map, &q, &pixel, &band);
                if (code == TSDF_SKIP) continue;
                rep->in_frustum++;
                if (code == TSDF_NO_DEPTH) rep->no_depth++;
                else if (code == TSDF_OCCLUDED) rep->occluded++;
                else {
                    rep->updated++;
                    tsdf[n] = tsdf_update(tsdf[n], q, v.max_weight);
                    if (color && img && band) color[n] = tsdf_colour_update(color[n], img + (size_t)pixel * 3, v.max_weight);
                }
            }
        }
}

// color may be null; pts receives ALL records
inline void tsdf_extract_serial(const uint32_t* tsdf, const uint32_t* color, const adc_tsdf_params& p, uint32_t min_weight, std::vector<adc_point>& pts,
                                adc_tsdf_extract_report* rep)
{
    const TsdfVol v = tsdf_vol(p);
    const size_t off[3] = {1, (size_t)v.nx, (size_t)v.nx * v.ny};
    memset(rep, 0, sizeof(*rep));
    pts.clear();
    for (int k = 0; k < v.nz; k++)
        for (int j = 0; j < v.ny; j++)
            for (int i = 0; i < v.nx; i++) {
                const size_t n = ((size_t)k * v.ny + j) * v.nx + i;
                if (!tsdf_seen(tsdf[n], min_weight)) continue;
                rep->voxels_seen++;
                const bool inside[3] = {i + 1 < v.nx, j + 1 < v.ny, k + 1 < v.nz};
                for (int a = 0; a < 3; a++) {
                    if (!inside[a] || !tsdf_crossing(tsdf[n], tsdf[n + off[a]], min_weight)) continue;
                    uint32_t rec[4];
                    tsdf_point(v, i, j, k, a, tsdf[n], tsdf[n + off[a]], color ? color[n] : 0u, color ? color[n + off[a]] : 0u, rec);
                    adc_point pt;
                    memcpy(&pt, rec, sizeof(pt));
                    pts.push_back(pt);
                    rep->points++;
                }
            }
}
