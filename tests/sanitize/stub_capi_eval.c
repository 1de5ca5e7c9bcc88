/* Stub of the ground-truth evaluation (include/adcensus_c_api.h: adc_set_ground_truth ... adc_get_eval_report) for the SANITIZER
 * builds of the host C++ layer, next to stub_capi.c: the header's definition in plain C, one pixel at a time, so that the CLI's --gt
 * path (PNG / PFM ground truth, the table, <out>-err.pfm, <out>-bad.png) runs under ASAN / UBSAN and its files can be compared with
 * tests/eval_ref.py.  Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "adcensus_c_api.h"

struct adc_handle { int w, h; adc_option opt; }; /* (the layout of stub_capi.c) */
static float* g_gt[2];   /* decoded ground truth, unknown = +inf (reachable from here until the process ends) */
static uint8_t* g_nonocc;
static int g_set, g_has_right, g_has_mask, g_report_valid;
static float g_occ_thres;
static adc_eval_report g_report;

static int gt_ok(const adc_handle* h, const adc_gt* g)
{
    if (!g->data || g->format < ADC_GT_U8 || g->format > ADC_GT_F32 || !(isfinite(g->scale) && g->scale > 0.0f) || g->pitch_bytes < 0) return 0;
    const long long row = (long long)h->w * (g->format == ADC_GT_U8 ? 1 : (g->format == ADC_GT_U16 ? 2 : 4));
    const long long pitch = g->pitch_bytes ? g->pitch_bytes : row;
    return pitch >= row && pitch * h->h <= 2147483647LL;
}

static void decode(const adc_handle* h, const adc_gt* g, float* out)
{
    const int bpp = g->format == ADC_GT_U8 ? 1 : (g->format == ADC_GT_U16 ? 2 : 4);
    const size_t pitch = g->pitch_bytes ? (size_t)g->pitch_bytes : (size_t)h->w * bpp;
    for (int y = 0; y < h->h; y++)
        for (int x = 0; x < h->w; x++) {
            const uint8_t* p = (const uint8_t*)g->data + (size_t)y * pitch + (size_t)x * bpp;
            float v;
            int zero = 0;
            if (g->format == ADC_GT_U8) { zero = p[0] == 0; v = (float)p[0]; }
            else if (g->format == ADC_GT_U16) { uint16_t u; memcpy(&u, p, 2); zero = u == 0; v = (float)u; }
            else memcpy(&v, p, 4);
            const float q = v / g->scale;
            out[(size_t)y * h->w + x] = (!zero && isfinite(q)) ? q : INFINITY;
        }
}

int adc_set_ground_truth(adc_handle* h, const adc_gt* left, const adc_gt* right, const uint8_t* nonocc, float occ_thres)
{
    if (!h || !left || !gt_ok(h, left) || (right && !gt_ok(h, right)) || !(isfinite(occ_thres) && occ_thres >= 0.0f)) return 1;
    const size_t n = (size_t)h->w * h->h;
    for (int s = 0; s < 2; s++) { free(g_gt[s]); g_gt[s] = (float*)malloc(n * sizeof(float)); }
    free(g_nonocc);
    g_nonocc = (uint8_t*)calloc(n, 1);
    g_set = 0;
    if (!g_gt[0] || !g_gt[1] || !g_nonocc) return 2;
    decode(h, left, g_gt[0]);
    if (right) decode(h, right, g_gt[1]);
    for (int y = 0; y < h->h; y++)
        for (int x = 0; x < h->w; x++) {
            const size_t i = (size_t)y * h->w + x;
            const float g = g_gt[0][i];
            int ok = isfinite(g);
            if (ok && right) {
                const float r = rintf(g);
                ok = fabsf(r) <= 1073741824.0f;
                if (ok) {
                    const int xr = x - (int)r;
                    ok = xr >= 0 && xr < h->w;
                    if (ok) { const float v = g_gt[1][(size_t)y * h->w + xr]; ok = isfinite(v) && fabsf(v - g) <= occ_thres; }
                }
            } else if (ok) ok = nonocc && nonocc[i] != 0;
            g_nonocc[i] = (uint8_t)ok;
        }
    g_has_right = right != NULL;
    g_has_mask = !right && nonocc;
    g_occ_thres = occ_thres;
    g_set = 1;
    return 0;
}

int adc_clear_ground_truth(adc_handle* h)
{
    if (!h) return 1;
    g_set = 0;
    return 0;
}

static void add(adc_eval_mask_stats* m, adc_eval_fill_stats* f, int valid, const int* bad, uint32_t eq)
{
    if (m) {
        m->pixels++;
        if (!valid) { m->invalid++; return; }
        for (int k = 0; k < ADC_EVAL_MAX_THRESHOLDS; k++) m->bad[k] += (uint64_t)bad[k];
        m->sum_err_q += eq;
        m->sum_sq_err_q += (uint64_t)eq * eq;
        m->err_hist[(eq >> 8) < 255u ? (eq >> 8) : 255u]++;
    } else {
        f->pixels++;
        if (!valid) { f->invalid++; return; }
        for (int k = 0; k < ADC_EVAL_MAX_THRESHOLDS; k++) f->bad[k] += (uint64_t)bad[k];
        f->sum_err_q += eq;
    }
}

int adc_evaluate(adc_handle* h, const float* d, const uint8_t* prov, const float* conf, const adc_eval_params* params, float* err, uint8_t* cls,
                 adc_eval_report* out)
{
    float t[ADC_EVAL_MAX_THRESHOLDS] = {1.0f, INFINITY, INFINITY, INFINITY};
    int n = 1;
    if (!h || !d || (conf && !prov) || !g_set) return 1;
    if (params) {
        n = params->n_thresholds;
        if (n < 0 || n > ADC_EVAL_MAX_THRESHOLDS) return 1;
        for (int k = 0; k < ADC_EVAL_MAX_THRESHOLDS; k++) {
            t[k] = k < n ? params->thresholds[k] : INFINITY;
            if (k < n && !(isfinite(t[k]) && t[k] >= 0.0f)) return 1;
        }
    }
    adc_eval_report* r = &g_report;
    memset(r, 0, sizeof(*r));
    const int has_occ = g_has_right || g_has_mask;
    const size_t np = (size_t)h->w * h->h;
    for (size_t i = 0; i < np; i++) {
        const float g = g_gt[0][i];
        const int known = isfinite(g), valid = isfinite(d[i]), kv = known && valid, non = known && g_nonocc[i];
        const float e = kv ? fabsf(d[i] - g) : INFINITY;
        const uint32_t eq = kv ? (uint32_t)rintf(fminf(e, 2048.0f) * 1024.0f) : 0u;
        int bad[ADC_EVAL_MAX_THRESHOLDS];
        for (int k = 0; k < ADC_EVAL_MAX_THRESHOLDS; k++) bad[k] = kv && e > t[k];
        if (known) add(&r->all, NULL, valid, bad, eq);
        if (non) add(&r->nonocc, NULL, valid, bad, eq);
        if (prov && known) {
            const int fill = (prov[i] >> ADC_PROV_FILL_SHIFT) & 3;
            add(NULL, &r->by_fill[fill], valid, bad, eq);
            if (prov[i] & ADC_PROV_SPECKLE) r->speckle_removed_known++;
            if (conf && kv && fill == ADC_FILL_WTA) {
                const float c = conf[i] * 256.0f;
                const int b = !(c >= 0.0f) ? 0 : (c >= 255.0f ? 255 : (int)c);
                r->conf_pixels[b]++;
                r->conf_bad[b] += (uint64_t)bad[0];
            }
        }
        if (err) err[i] = e;
        if (cls) cls[i] = (uint8_t)((known ? ADC_EVAL_KNOWN : 0) | (valid ? ADC_EVAL_VALID : 0) | (bad[0] ? ADC_EVAL_BAD : 0) |
                                    ((known && has_occ && !non) ? ADC_EVAL_OCCLUDED : 0));
    }
    for (int k = 0; k < n; k++) r->thresholds[k] = t[k];
    r->n_thresholds = n;
    r->occ_thres = g_occ_thres;
    r->has_right_gt = (uint8_t)g_has_right;
    r->has_nonocc_mask = (uint8_t)g_has_mask;
    r->has_provenance = prov != NULL;
    r->has_confidence = conf != NULL;
    g_report_valid = 1;
    if (out) *out = *r;
    return 0;
}

int adc_get_eval_report(adc_handle* h, adc_eval_report* out)
{
    if (!h || !out || !g_report_valid) return 1;
    *out = g_report;
    return 0;
}
