/* Stub of the rectification entry points (include/adcensus_c_api.h) for the SANITIZER builds of the host C++ layer, next to
 * stub_capi.c: the facade's SetRectifyMaps / SetRectifyModel / ClearRectify / Rectify and the CLI's --rectify parsing link and run
 * under ASAN / UBSAN.  The stub checks the arguments as the library does and copies nothing: "device" buffers are host allocations
 * nobody reads, a "rectified" image stays what the caller put there.  Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <math.h>
#include <stdlib.h>
#include "adcensus_c_api.h"

static int format_ok(const adc_raw_format* f)
{
    if (!f || f->format < ADC_PIX_BGR8 || f->format > ADC_PIX_BGRA8) return 0;
    const int bpp = f->format == ADC_PIX_GRAY8 ? 1 : (f->format == ADC_PIX_BGRA8 ? 4 : 3);
    return f->width >= 1 && f->width <= 32767 && f->height >= 1 && f->height <= 32767 && (long long)f->pitch_bytes >= (long long)f->width * bpp &&
           (long long)f->height * f->pitch_bytes <= 2147483647LL;
}
static int side_ok(int side) { return side == ADC_SIDE_LEFT || side == ADC_SIDE_RIGHT; }

int adc_set_rectify_maps(adc_handle* h, int side, const adc_raw_format* raw, const float* map_x, const float* map_y)
{
    return (h && side_ok(side) && format_ok(raw) && map_x && map_y) ? 0 : 1;
}
int adc_set_rectify_model(adc_handle* h, int side, const adc_raw_format* raw, const adc_camera_model* m)
{
    if (!h || !side_ok(side) || !format_ok(raw) || !m) return 1;
    const float* v = &m->fx;
    for (size_t i = 0; i < sizeof(*m) / sizeof(float); i++)
        if (!isfinite(v[i])) return 1;
    return (m->fx != 0.0f && m->fy != 0.0f && m->new_fx != 0.0f && m->new_fy != 0.0f) ? 0 : 1;
}
int adc_clear_rectify(adc_handle* h) { return h ? 0 : 1; }
int adc_rectify_device(adc_handle* h, int side, const void* d_raw, void* d_bgr_out) { return (h && side_ok(side) && d_raw && d_bgr_out) ? 0 : 1; }
void* adc_device_malloc(size_t bytes) { return malloc(bytes ? bytes : 1); }
void adc_device_free(void* p) { free(p); }
int adc_memcpy_h2d(void* dst, const void* src, size_t bytes) { (void)bytes; return (dst && src) ? 0 : 1; }
int adc_memcpy_d2h(void* dst, const void* src, size_t bytes) { (void)bytes; return (dst && src) ? 0 : 1; }
