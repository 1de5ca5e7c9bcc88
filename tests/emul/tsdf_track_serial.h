// tsdf_track_serial.h -- frame-to-model tracking, one pixel and one solve at a time: adcensus_amd/csrc/tsdf_track.h run serially
// (tests/emul/emul_tsdf_track.cpp).  The loop of adc_track_device without a device: a reduce pass over the participating pixels in
// raster order, then track_solve, until a terminal status or `iterations` solves.
#pragma once
#include <string.h>
#include <vector>

#include "../../adcensus_amd/csrc/tsdf_track.h"

// sums (optional) receives the 28 sums of every reduce pass that ran
inline void tsdf_track_serial(const float* map, const float* fnormals, int W, int H, const adc_tsdf_frame& frame, const adc_tsdf_raycast_params& model,
                              const float* mdepth, const float* mnormals, const adc_track_params& p, adc_track_result* res, std::vector<long long>* sums)
{
    const TrackFrame f = track_frame(frame, W, H);
    const TrackModel m = track_model(model);
    const TrackGate g = track_gate(p);
    const uint32_t pixels = track_span(W, p.stride) * track_span(H, p.stride);
    TrackPose k = track_guess(frame);
    memset(res, 0, sizeof(*res));
    for (uint32_t iter = 0; iter < p.iterations; iter++) {
        long long S[TRACK_SUMS] = {0};
        uint32_t c[TRACK_COUNTS] = {0};
        for (uint32_t n = 0; n < pixels; n++) {
            int x, y, q[7];
            track_pixel_of(f, g, n, &x, &y);
            const int what = track_pixel(f, m, g, k, x, y, map, fnormals, mdepth, mnormals, q);
            if (what == TRACK_USED) track_accumulate(q, S);
            c[what]++;
        }
        if (sums) sums->insert(sums->end(), S, S + TRACK_SUMS);
        const bool done = track_solve(S, c, pixels, p, m, k, iter, res);
        memcpy(k.R, res->R, sizeof(k.R));
        memcpy(k.t, res->t, sizeof(k.t));
        if (done) break;
    }
}
