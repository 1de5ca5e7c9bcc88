/* Stub of the registration into a second camera (include/adcensus_c_api.h: adc_set_register_target ... adc_get_register_report) for
 * the SANITIZER builds of the host C++ layer, next to stub_capi.c: the header's definition in plain C, one pixel at a time, so that
 * the CLI's --register path (the target file, <out>-reg.pfm, <out>-aligned.png, the recoloured cloud) runs under ASAN / UBSAN and its
 * files can be compared with tests/register_ref.py.  Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "adcensus_c_api.h"

struct adc_handle { int w, h; adc_option opt; }; /* (the layout of stub_capi.c) */
static adc_reg_target g_t;
static int g_set, g_report_valid;
static adc_reg_report g_report;

static int source_z(int kind, const adc_calib* c, float v, float* z)
{
    if (kind == ADC_REG_FROM_DEPTH) { *z = v; return isfinite(v) && v > 0.0f; }
    const float a = fabsf(v), s = a + c->doffs, fb = c->focal_px * c->baseline;
    if (!(isfinite(a) && s > 0.0f)) return 0;
    *z = fb / s;
    return 1;
}

static int project(const adc_calib* c, float xs, float ys, float Z, float* u, float* v, float* zt)
{
    const adc_reg_target* T = &g_t;
    const float X = ((xs - c->cx) * Z) / c->focal_px, Y = ((ys - c->cy) * Z) / c->focal_px;
    const float Xt = ((T->R[0] * X + T->R[1] * Y) + T->R[2] * Z) + T->t[0];
    const float Yt = ((T->R[3] * X + T->R[4] * Y) + T->R[5] * Z) + T->t[1];
    const float Zt = ((T->R[6] * X + T->R[7] * Y) + T->R[8] * Z) + T->t[2];
    *zt = Zt;
    if (!(isfinite(Zt) && Zt > 0.0f)) return 0;
    const float x = Xt / Zt, y = Yt / Zt, x2 = x * x, y2 = y * y, r2 = x2 + y2, xy = x * y;
    const float rad = 1.0f + r2 * (T->k1 + r2 * (T->k2 + r2 * T->k3));
    const float xd = (x * rad + (2.0f * T->p1) * xy) + T->p2 * (r2 + 2.0f * x2);
    const float yd = (y * rad + T->p1 * (r2 + 2.0f * y2)) + (2.0f * T->p2) * xy;
    *u = T->fx * xd + T->cx;
    *v = T->fy * yd + T->cy;
    return fabsf(*u) < 32768.0f && fabsf(*v) < 32768.0f;
}

static void extent(float a, float b, float c, int splat, int n, int* lo, int* hi)
{
    int e0, e1;
    if (splat) { e0 = (int)ceilf(fminf(a, b)); e1 = (int)ceilf(fmaxf(a, b)) - 1; }
    else e0 = e1 = (int)floorf(c + 0.5f);
    if (e0 < 0) e0 = 0;
    if (e1 > n - 1) e1 = n - 1;
    if (e1 > e0 + ADC_REG_MAX_SPLAT - 1) e1 = e0 + ADC_REG_MAX_SPLAT - 1;
    *lo = e0; *hi = e1;
}

static int request_ok(const adc_handle* h, const void* map, int kind, const adc_calib* c)
{
    return h && map && c && (kind == ADC_REG_FROM_DISPARITY || kind == ADC_REG_FROM_DEPTH) && isfinite(c->focal_px) && isfinite(c->baseline) &&
           isfinite(c->cx) && isfinite(c->cy) && isfinite(c->doffs) && c->focal_px > 0.0f && g_set;
}

int adc_set_register_target(adc_handle* h, const adc_reg_target* t)
{
    if (!h || !t || t->width < 1 || t->width > 32767 || t->height < 1 || t->height > 32767 || t->fx == 0.0f || t->fy == 0.0f) return 1;
    const float* f = &t->fx;
    for (int i = 0; i < 21; i++) if (!isfinite(f[i])) return 1; /* (fx .. t[2] are 21 consecutive floats) */
    g_t = *t;
    g_set = 1;
    return 0;
}

int adc_clear_register_target(adc_handle* h) { if (!h) return 1; g_set = 0; return 0; }

int adc_register_depth(adc_handle* h, const float* map, int kind, const adc_calib* c, uint32_t flags, float* depth, int32_t* index, adc_reg_report* report)
{
    if (!request_ok(h, map, kind, c) || (flags & ~(ADC_REG_NO_SPLAT | ADC_REG_PRETEST)) || (!depth && !index)) return 1;
    const size_t pt = (size_t)g_t.width * (size_t)g_t.height;
    uint64_t* z = (uint64_t*)malloc(pt * sizeof(uint64_t));
    if (!z) return 2;
    memset(z, 0xff, pt * sizeof(uint64_t));
    memset(&g_report, 0, sizeof(g_report));
    for (int y = 0; y < h->h; y++)
        for (int x = 0; x < h->w; x++) {
            float Z, uc, vc, zc, ua, va, ub, vb, zz;
            if (!source_z(kind, c, map[(size_t)y * h->w + x], &Z)) continue;
            g_report.src_valid++;
            if (!project(c, (float)x, (float)y, Z, &uc, &vc, &zc) || !project(c, (float)x - 0.5f, (float)y - 0.5f, Z, &ua, &va, &zz) ||
                !project(c, (float)x + 0.5f, (float)y + 0.5f, Z, &ub, &vb, &zz))
                continue;
            int j0, j1, i0, i1;
            extent(ua, ub, uc, !(flags & ADC_REG_NO_SPLAT), g_t.width, &j0, &j1);
            extent(va, vb, vc, !(flags & ADC_REG_NO_SPLAT), g_t.height, &i0, &i1);
            if (j0 > j1 || i0 > i1) continue;
            g_report.src_projected++;
            uint32_t bits;
            memcpy(&bits, &zc, 4);
            const uint64_t key = ((uint64_t)bits << 32) | (uint32_t)(y * h->w + x);
            for (int i = i0; i <= i1; i++)
                for (int j = j0; j <= j1; j++)
                    if (key < z[(size_t)i * g_t.width + j]) z[(size_t)i * g_t.width + j] = key;
        }
    for (size_t i = 0; i < pt; i++) {
        const int hit = z[i] != UINT64_MAX;
        const uint32_t bits = (uint32_t)(z[i] >> 32);
        float d = INFINITY;
        if (hit) memcpy(&d, &bits, 4);
        if (depth) depth[i] = d;
        if (index) index[i] = hit ? (int32_t)(uint32_t)z[i] : -1;
        g_report.dst_filled += (uint32_t)hit;
    }
    free(z);
    g_report_valid = 1;
    if (report) *report = g_report;
    return 0;
}

int adc_align_color(adc_handle* h, const float* map, int kind, const adc_calib* c, const uint8_t* target_bgr, uint8_t* out, uint8_t* valid)
{
    if (!request_ok(h, map, kind, c) || !target_bgr || !out) return 1;
    for (int y = 0; y < h->h; y++)
        for (int x = 0; x < h->w; x++) {
            const size_t p = (size_t)y * h->w + x;
            float Z, u, v, zc;
            int ok = source_z(kind, c, map[p], &Z) && project(c, (float)x, (float)y, Z, &u, &v, &zc);
            int i = 0, j = 0;
            if (ok) {
                j = (int)floorf(u + 0.5f);
                i = (int)floorf(v + 0.5f);
                ok = j >= 0 && j < g_t.width && i >= 0 && i < g_t.height;
            }
            for (int k = 0; k < 3; k++) out[p * 3 + k] = ok ? target_bgr[((size_t)i * g_t.width + j) * 3 + k] : 0;
            if (valid) valid[p] = (uint8_t)ok;
        }
    return 0;
}

/* (no device memory in the stub: the device forms are never reached by the host layer) */
int adc_register_depth_device(adc_handle* h, const void* m, int kind, const adc_calib* c, uint32_t flags, void* depth, void* index)
{
    (void)h; (void)m; (void)kind; (void)c; (void)flags; (void)depth; (void)index;
    return 1;
}
int adc_align_color_device(adc_handle* h, const void* m, int kind, const adc_calib* c, const void* t, void* out, void* valid)
{
    (void)h; (void)m; (void)kind; (void)c; (void)t; (void)out; (void)valid;
    return 1;
}
int adc_get_register_report(adc_handle* h, adc_reg_report* out)
{
    if (!h || !out || !g_report_valid) return 1;
    *out = g_report;
    return 0;
}
