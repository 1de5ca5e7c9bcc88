/* Stub of adc_match_ex (include/adcensus_c_api.h) for the SANITIZER builds of the host C++ layer, next to stub_capi.c: the
 * disparity map of the stub's adc_match plus synthetic provenance codes and confidences (every code; values in [0, 1]), so that
 * the CLI's --extras writers run under ASAN / UBSAN.  Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <math.h>
#include <stddef.h>
#include "adcensus_c_api.h"

struct adc_handle { int w, h; adc_option opt; }; /* (the layout of stub_capi.c) */

int adc_match_ex(adc_handle* h, const uint8_t* l, const uint8_t* r, float* d, uint8_t* prov, float* conf)
{
    const int rc = adc_match(h, l, r, d);
    if (rc != 0) return rc;
    const size_t n = (size_t)h->w * h->h;
    for (size_t i = 0; i < n; i++) {
        const int lr = (int)(i % 3), fill = isinf(d[i]) ? ADC_FILL_NONE : (int)((i / 3) % 3);
        if (prov) prov[i] = (uint8_t)(lr | (fill << ADC_PROV_FILL_SHIFT));
        if (conf) conf[i] = fill == ADC_FILL_WTA ? (float)(i % 101) / 100.0f : 0.0f;
    }
    return 0;
}
