/* Stub of adc_match_out / adc_get_cloud_count (include/adcensus_c_api.h) for the SANITIZER builds of the host C++ layer, next to
 * stub_capi.c: the disparity map of the stub's adc_match plus depth, point cloud and 8-bit image computed from it by the
 * header's definitions in plain C, so that the CLI's --calib writers (PFM, binary PLY) run under ASAN / UBSAN on holes, negative
 * values and a capacity limit.  Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <math.h>
#include <stddef.h>
#include "adcensus_c_api.h"

struct adc_handle { int w, h; adc_option opt; }; /* (the layout of stub_capi.c) */
static uint64_t g_count;

int adc_match_out(adc_handle* h, const uint8_t* l, const uint8_t* r, float* d, const adc_outputs* o)
{
    const int rc = adc_match(h, l, r, d);
    if (rc != 0 || !o) return rc;
    if (o->depth && !o->calib) return 1;
    if (o->calib && !(o->calib->focal_px > 0.0f)) return 1;
    const size_t n = (size_t)h->w * h->h;
    const float fb = o->calib ? o->calib->focal_px * o->calib->baseline : 0.0f;
    float mn = (float)h->w, mx = -(float)h->w;
    for (size_t i = 0; i < n; i++) {
        const float a = fabsf(d[i]);
        if (a != INFINITY) { mn = a < mn ? a : mn; mx = a > mx ? a : mx; }
    }
    uint64_t count = 0;
    for (size_t i = 0; i < n; i++) {
        const float a = fabsf(d[i]);
        const float s = o->calib ? a + o->calib->doffs : 1.0f;
        const int valid = o->calib ? (isfinite(a) && s > 0.0f) : (a != INFINITY);
        const float z = o->calib ? (valid ? fb / s : INFINITY) : a;
        if (o->disp8) o->disp8[i] = (a == INFINITY || !(mx > mn)) ? 0 : (uint8_t)((a - mn) / (mx - mn) * 255);
        if (o->depth) o->depth[i] = z;
        if (o->cloud && valid) {
            if (count < o->cloud_capacity) {
                adc_point* p = &o->cloud[count];
                const float x = (float)(i % (size_t)h->w), y = (float)(i / (size_t)h->w);
                p->x = o->calib ? ((x - o->calib->cx) * z) / o->calib->focal_px : x;
                p->y = o->calib ? ((y - o->calib->cy) * z) / o->calib->focal_px : y;
                p->z = z;
                p->r = l[3 * i + 2]; p->g = l[3 * i + 1]; p->b = l[3 * i]; p->pad = 0;
            }
            count++;
        }
    }
    if (o->cloud) { g_count = count; if (o->cloud_count) *o->cloud_count = (uint32_t)count; }
    return 0;
}

int adc_get_cloud_count(adc_handle* h, uint64_t* count)
{
    if (!h || !count) return 1;
    *count = g_count;
    return 0;
}
