/* Stub of the surface normals (include/adcensus_c_api.h: adc_normals_device, adc_normals, adc_get_normals_report) for the SANITIZER
 * builds of the host C++ layer, next to stub_capi.c: the shared arithmetic of adcensus_amd/csrc/normals_fit.h run serially, one pixel
 * and one tap at a time, so that the CLI's --normals path (<out>-n.png, the normals of the cloud's points) runs under ASAN / UBSAN
 * and its files can be compared with tests/normals_ref.py.  Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <cmath>
#include <cstdlib>
#include <vector>

#include "../../adcensus_amd/csrc/normals_fit.h"

struct adc_handle { int w, h; adc_option opt; }; /* (the layout of stub_capi.c) */
static adc_normals_report g_report;
static int g_report_valid;

extern "C" int adc_normals(adc_handle* h, const float* disp, const adc_calib* c, const adc_normals_params* params, float* normals, uint8_t* normals8,
                           adc_normals_report* report)
{
    const adc_normals_params def = {2, 1.0f, 5, 0u, {0u, 0u, 0u, 0u}};
    const adc_normals_params p = params ? *params : def;
    if (!h || !disp || !c || !(std::isfinite(c->focal_px) && std::isfinite(c->baseline) && std::isfinite(c->cx) && std::isfinite(c->cy) && std::isfinite(c->doffs)) ||
        !(c->focal_px > 0.0f) || p.radius < 1 || p.radius > ADC_NORMALS_MAX_RADIUS || !(std::isfinite(p.max_diff) && p.max_diff > 0.0f && p.max_diff <= 64.0f) ||
        p.min_points < 3 || p.min_points > (2 * p.radius + 1) * (2 * p.radius + 1) || p.flags || p.reserved_[0] || p.reserved_[1] || p.reserved_[2] ||
        p.reserved_[3] || (!normals && !normals8))
        return 1;
    const int W = h->w, H = h->h, r = p.radius;
    const int32_t G = (int32_t)rintf(p.max_diff * 1024.0f);
    const NrmCam cam = {c->focal_px, c->cx, c->cy, c->doffs};
    std::vector<int32_t> q((size_t)W * H);
    for (size_t i = 0; i < q.size(); i++) q[i] = nrm_quantise(disp[i]);
    adc_normals_report rep = {0, 0, 0, 0};
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            NrmPixel o;
            o.v[0] = o.v[1] = o.v[2] = o.v[3] = 0.0f;
            o.bytes = 0;
            o.cls = NRM_UNUSABLE;
            if (q[i] != NRM_Q_NONE) {
                NrmSums s = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                for (int dy = -r; dy <= r; dy++)
                    for (int dx = -r; dx <= r; dx++) {
                        if (x + dx < 0 || x + dx >= W || y + dy < 0 || y + dy >= H) continue;
                        const int32_t e = q[(size_t)(y + dy) * W + (x + dx)] - q[i];
                        if (nrm_gate(e, G)) nrm_add_tap(&s, dx, dy, e);
                    }
                o = nrm_fit(s, q[i], x, y, cam, p.min_points);
                rep.usable++;
                rep.fitted += o.cls == NRM_FITTED;
                rep.few_points += o.cls == NRM_FEW_POINTS;
                rep.degenerate += o.cls == NRM_DEGENERATE;
            }
            for (int k = 0; k < 4; k++) {
                if (normals) normals[4 * i + k] = o.v[k];
                if (normals8) normals8[4 * i + k] = (uint8_t)(o.bytes >> (8 * k));
            }
        }
    g_report = rep;
    g_report_valid = 1;
    if (report) *report = rep;
    return 0;
}

/* (no device memory in the stub: the device form is never reached by the host layer) */
extern "C" int adc_normals_device(adc_handle* h, const void* d, const adc_calib* c, const adc_normals_params* p, void* n, void* n8)
{
    (void)h; (void)d; (void)c; (void)p; (void)n; (void)n8;
    return 1;
}

extern "C" int adc_get_normals_report(adc_handle* h, adc_normals_report* out)
{
    if (!h || !out || !g_report_valid) return 1;
    *out = g_report;
    return 0;
}
