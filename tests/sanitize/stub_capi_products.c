/* Stub of adc_match_products / adc_match_async_products (include/adcensus_c_api.h) for the SANITIZER builds of the host C++ layer,
 * next to stub_capi.c: the products of the other stubs (adc_match_ex, adc_match_out) from one call, plus the 16-bit fixed-point map
 * computed by the header's definition in plain C, so that the CLI's --disp16 writer (16-bit PGM) runs under ASAN / UBSAN on holes,
 * zeros, negative values and saturation.  Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <math.h>
#include <stddef.h>
#include "adcensus_c_api.h"

struct adc_handle { int w, h; adc_option opt; }; /* (the layout of stub_capi.c) */

int adc_match_products(adc_handle* h, const uint8_t* l, const uint8_t* r, float* d, const adc_products* p)
{
    if (!p) return adc_match(h, l, r, d);
    if (p->disp16 && !(isfinite(p->disp16_scale) && p->disp16_scale > 0.0f)) return 1;
    int rc = (p->provenance || p->confidence) ? adc_match_ex(h, l, r, d, p->provenance, p->confidence) : adc_match(h, l, r, d);
    if (rc == 0 && (p->out.depth || p->out.cloud || p->out.disp8)) rc = adc_match_out(h, l, r, d, &p->out); /* (the same map again) */
    if (rc != 0 || !p->disp16) return rc;
    const size_t n = (size_t)h->w * h->h;
    for (size_t i = 0; i < n; i++) {
        const float a = fabsf(d[i]);
        if (!isfinite(a)) { p->disp16[i] = 0; continue; }
        const float q = a * p->disp16_scale;
        p->disp16[i] = (uint16_t)fminf(fmaxf(q, 1.0f), 65535.0f);
    }
    return 0;
}

int adc_match_async_products(adc_handle* h, const uint8_t* l, const uint8_t* r, float* d, const adc_products* p)
{
    return adc_match_products(h, l, r, d, p); /* (the stub's adc_wait has nothing left to do) */
}
