/* Stub of adc_set_speckle_filter (include/adcensus_c_api.h) for the SANITIZER builds of the host C++ layer, next to stub_capi.c:
 * the facade's SetSpeckleFilter and the CLI's --speckle parsing link and run under ASAN / UBSAN; the stub checks the arguments as
 * the library does and filters nothing.  Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <math.h>
#include "adcensus_c_api.h"

int adc_set_speckle_filter(adc_handle* h, int32_t max_size, float max_diff)
{
    (void)max_size;
    if (!h || !isfinite(max_diff) || max_diff < 0.0f) return 1;
    return 0;
}
