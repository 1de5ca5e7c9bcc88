// tsdf_raycast_serial.h -- the ray cast of a TSDF volume on the host, one ray at a time in raster order, from the functions of
// adcensus_amd/csrc/tsdf_ray.h alone (tests/emul/emul_tsdf_raycast.cpp, tests/sanitize/stub_capi_tsdf_raycast.cpp).  Host-only C++.
#pragma once
#include <cstring>

#include "../../adcensus_amd/csrc/tsdf_ray.h"

// Each output may be null.  color may be null (then bgr must be).  The report is always filled.
inline void tsdf_raycast_serial(const uint32_t* tsdf, const uint32_t* color, const adc_tsdf_params& p, const adc_tsdf_raycast_params& view, float* depth,
                                float* normals, uint8_t* bgr, uint8_t* status, adc_tsdf_raycast_report* rep)
{
    const TsdfVol vol = tsdf_vol(p);
    const TsdfRayView v = tsdf_ray_view(view, p);
    uint32_t counts[5] = {0u, 0u, 0u, 0u, 0u};
    unsigned long long total = 0;
    for (int y = 0; y < v.H; y++)
        for (int x = 0; x < v.W; x++) {
            uint32_t samples = 0;
            const TsdfRayPixel o = tsdf_ray_cast(vol, v, tsdf, bgr ? color : nullptr, x, y, &samples);
            const size_t at = (size_t)y * (size_t)v.W + (size_t)x;
            if (depth) depth[at] = o.depth;
            if (normals) memcpy(normals + at * 4, o.normal, sizeof(o.normal));
            if (bgr) memcpy(bgr + at * 3, o.bgr, 3);
            if (status) status[at] = o.status;
            counts[o.status]++;
            total += samples;
        }
    memset(rep, 0, sizeof(*rep));
    rep->rays = (uint32_t)v.W * (uint32_t)v.H;
    rep->miss = counts[ADC_TSDF_RAY_MISS];
    rep->hit = counts[ADC_TSDF_RAY_HIT];
    rep->no_surface = counts[ADC_TSDF_RAY_NO_SURFACE];
    rep->behind = counts[ADC_TSDF_RAY_BEHIND];
    rep->exhausted = counts[ADC_TSDF_RAY_EXHAUSTED];
    rep->samples_lo = (uint32_t)(total & 0xFFFFFFFFull);
    rep->samples_hi = (uint32_t)(total >> 32);
}
