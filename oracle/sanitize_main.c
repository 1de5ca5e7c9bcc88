/* oracle/sanitize_main.c -- TEST INFRASTRUCTURE ONLY: a small structured pair through adc_oracle_run (all stages dumped) and
 * adc_oracle_match of whichever oracle it is linked with, for the ASAN / UBSAN builds (`make -C oracle asan`): the port
 * (adcensus_port.c) and, where /root/reference exists, the reference's own sources behind ref_driver.cpp.  Exit code 0 and no
 * sanitizer report = clean on this input (min_disparity = 0; the reference's documented out-of-bounds read for
 * min_disparity > 0, ADCensusStereo.cpp:296-300, is not provoked).
 * Arguments: option overrides as field=value (lambda_ad, lambda_census, cross_L1, cross_L2, cross_t1, cross_t2, so_p1, so_p2, so_tso,
 * irv_ts, irv_th, lrcheck_thres), e.g. `sanitize_port so_p1=-1 so_p2=-3`; an unknown field or a malformed value is exit code 4.
 * Or `refine FILE`: one constructed refinement input through adc_oracle_refine_from (refine_mode below). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "oracle_abi.h"

static int override(adc_option* o, const char* arg)
{
    const char* eq = strchr(arg, '=');
    char* end = NULL;
    if (!eq || eq == arg || !eq[1]) return 0;
    const size_t n = (size_t)(eq - arg);
    const double v = strtod(eq + 1, &end);
    if (*end) return 0;
#define INT_FIELD(f) if (n == strlen(#f) && !strncmp(arg, #f, n)) { o->f = (int32_t)v; return (double)(int32_t)v == v; }
#define FLT_FIELD(f) if (n == strlen(#f) && !strncmp(arg, #f, n)) { o->f = (float)v; return 1; }
    INT_FIELD(lambda_ad) INT_FIELD(lambda_census) INT_FIELD(cross_L1) INT_FIELD(cross_L2) INT_FIELD(cross_t1) INT_FIELD(cross_t2)
    FLT_FIELD(so_p1) FLT_FIELD(so_p2) INT_FIELD(so_tso) INT_FIELD(irv_ts) FLT_FIELD(irv_th) FLT_FIELD(lrcheck_thres)
#undef INT_FIELD
#undef FLT_FIELD
    return 0;
}

/* `refine FILE`: one constructed refinement input (tests/refine_patterns.py) through adc_oracle_refine_from.  FILE = int32 {w, h, first,
 * last, has_left, has_cost, has_arms, has_right, has_label}, the adc_option, then the arrays that are there, in this order: left u8
 * [H][W][3], cost f32 [H][W][D], arms u8 [H][W][4], disp f32 [H][W], right f32 [H][W], label u8 [H][W].  Prints the sum of the
 * result's 32-bit patterns; exit code 5 = unreadable file, 2 = refine_from refused the input. */
static void* read_array(FILE* f, int present, size_t bytes, int* ok)
{
    if (!present) return NULL;
    void* p = malloc(bytes ? bytes : 1);
    if (!p || fread(p, 1, bytes, f) != bytes) *ok = 0;
    return p;
}

static int refine_mode(const char* path)
{
    FILE* f = fopen(path, "rb");
    int32_t hd[9];
    adc_option opt;
    if (!f || fread(hd, sizeof(hd), 1, f) != 1 || fread(&opt, sizeof(opt), 1, f) != 1 || hd[0] <= 0 || hd[1] <= 0 ||
        opt.max_disparity <= opt.min_disparity) {
        printf("unreadable pattern file: %s\n", path);
        if (f) fclose(f);
        return 5;
    }
    const size_t P = (size_t)hd[0] * (size_t)hd[1], D = (size_t)(opt.max_disparity - opt.min_disparity);
    int ok = 1;
    uint8_t* left = read_array(f, hd[4], P * 3, &ok);
    float* cost = read_array(f, hd[5], P * D * 4, &ok);
    uint8_t* arms = read_array(f, hd[6], P * 4, &ok);
    float* disp = read_array(f, 1, P * 4, &ok);
    float* right = read_array(f, hd[7], P * 4, &ok);
    uint8_t* label = read_array(f, hd[8], P, &ok);
    fclose(f);
    int rc = 5;
    if (ok) {
        rc = adc_oracle_refine_from(hd[0], hd[1], &opt, hd[2], hd[3], left, cost, arms, disp, right, label) != 0 ? 2 : 0;
        unsigned long long sum = 0;
        for (size_t i = 0; i < P; i++) { uint32_t u; memcpy(&u, disp + i, 4); sum += u; }
        if (rc == 0) printf("%s oracle under the sanitizers: refine_from ok, sum %llu\n", adc_oracle_kind(), sum);
        else printf("adc_oracle_refine_from refused the input\n");
    } else printf("unreadable pattern file: %s\n", path);
    free(left); free(cost); free(arms); free(disp); free(right); free(label);
    return rc;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "refine")) return refine_mode(argv[2]);
    const int W = 96, H = 64, D = 24;
    uint8_t* l = (uint8_t*)malloc((size_t)W * H * 3);
    uint8_t* r = (uint8_t*)malloc((size_t)W * H * 3);
    unsigned s = 12345u;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W + D; x++) { /* a textured strip; the left view is the right one shifted by a piecewise-constant disparity */
            s = s * 1664525u + 1013904223u;
            const int base = 128 + (int)(60.0 * ((x / 9 + y / 7) % 3 - 1)) + (int)((s >> 24) % 17) - 8;
            for (int c = 0; c < 3; c++) {
                const int v = base + 9 * c;
                const uint8_t px = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
                if (x >= D && x - D < W) r[((size_t)y * W + (x - D)) * 3 + c] = px;
                const int d = 4 + ((y / 16) % 2) * 6, xl = x - D + d;
                if (xl >= 0 && xl < W) l[((size_t)y * W + xl) * 3 + c] = px;
            }
        }
    for (int y = 0; y < H; y++) for (int x = 0; x < 12; x++) for (int c = 0; c < 3; c++) l[((size_t)y * W + x) * 3 + c] = (uint8_t)(40 + x);
    adc_option opt;
    memset(&opt, 0, sizeof(opt));
    opt.min_disparity = 0; opt.max_disparity = D; opt.lambda_ad = 10.0f; opt.lambda_census = 30.0f; opt.cross_L1 = 34; opt.cross_L2 = 17;
    opt.cross_t1 = 20; opt.cross_t2 = 6; opt.so_p1 = 1.0f; opt.so_p2 = 3.0f; opt.so_tso = 15; opt.irv_ts = 20; opt.irv_th = 0.4f;
    opt.lrcheck_thres = 1.0f; opt.do_lr_check = 1; opt.do_filling = 1; opt.do_discontinuity_adjustment = 1;
    for (int i = 1; i < argc; i++)
        if (!override(&opt, argv[i])) { printf("bad option override: %s\n", argv[i]); free(l); free(r); return 4; }
    const size_t P = (size_t)W * H;
    adc_oracle_dump d;
    memset(&d, 0, sizeof(d));
    d.gray_left = malloc(P); d.gray_right = malloc(P); d.census_left = malloc(P * 8); d.census_right = malloc(P * 8);
    d.cost_init = malloc(P * D * 4); d.arms = malloc(P * 4); d.sup_count_h = malloc(P * 2); d.sup_count_v = malloc(P * 2);
    d.cost_aggr = malloc(P * D * 4); d.cost_so = malloc(P * D * 4); d.disp_left_wta = malloc(P * 4); d.disp_right_wta = malloc(P * 4);
    d.outlier_label = malloc(P); d.disp_after_lr = malloc(P * 4); d.disp_after_irv = malloc(P * 4); d.disp_after_interp = malloc(P * 4);
    d.disp_after_dda = malloc(P * 4); d.disp_final = malloc(P * 4);
    if (adc_oracle_run(W, H, &opt, l, r, &d) != 0) { printf("adc_oracle_run failed\n"); return 2; }
    float* m = malloc(P * 4);
    double secs = 0;
    if (adc_oracle_match(W, H, &opt, l, r, m, &secs) != 0) { printf("adc_oracle_match failed\n"); return 2; }
    const int same = memcmp(m, d.disp_final, P * 4) == 0;
    printf("%s oracle under the sanitizers: run + match ok, match == staged run: %s\n", adc_oracle_kind(), same ? "yes" : "NO");
    free(l); free(r); free(m);
    free(d.gray_left); free(d.gray_right); free(d.census_left); free(d.census_right); free(d.cost_init); free(d.arms); free(d.sup_count_h);
    free(d.sup_count_v); free(d.cost_aggr); free(d.cost_so); free(d.disp_left_wta); free(d.disp_right_wta); free(d.outlier_label);
    free(d.disp_after_lr); free(d.disp_after_irv); free(d.disp_after_interp); free(d.disp_after_dda); free(d.disp_final);
    return same ? 0 : 3;
}
