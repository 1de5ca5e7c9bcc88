/* Stub of adc_set_input_format (include/adcensus_c_api.h) for the SANITIZER builds of the host C++ layer, next to
 * stub_capi_rectify.c: the facade's SetInputFormat and the CLI's --raw parsing and frame loading link and run under ASAN / UBSAN.  The
 * stub checks the arguments as the library does (it has no handle geometry to compare with) and copies nothing.  Test infrastructure
 * (adcensus_amd/host/Makefile: `make asan`). */
#include "adcensus_c_api.h"

static int bytes_per_pixel(int c)
{
    if (c == ADC_PIX_BGR8 || c == ADC_PIX_RGB8) return 3;
    if (c == ADC_PIX_BGRA8) return 4;
    if (c == ADC_PIX_GRAY8 || c == ADC_PIX_NV12 || (c >= ADC_PIX_BAYER_RGGB8 && c <= ADC_PIX_BAYER_BGGR8)) return 1;
    if (c == ADC_PIX_GRAY16 || c == ADC_PIX_YUYV || c == ADC_PIX_UYVY || (c >= ADC_PIX_BAYER_RGGB16 && c <= ADC_PIX_BAYER_BGGR16)) return 2;
    return 0;
}

int adc_set_input_format(adc_handle* h, int side, const adc_raw_format* f)
{
    if (!h || !f || (side != ADC_SIDE_LEFT && side != ADC_SIDE_RIGHT) || f->format < 0 || f->format > 0xffff) return 1;
    const int c = f->format & 0xff, bits = (f->format >> 8) & 0xff, bpp = bytes_per_pixel(c);
    const int wide = c == ADC_PIX_GRAY16 || (c >= ADC_PIX_BAYER_RGGB16 && c <= ADC_PIX_BAYER_BGGR16);
    if (bpp == 0 || (bits != 0 && !(wide && bits >= 9 && bits <= 16))) return 1;
    if (f->width < 1 || f->width > 32767 || f->height < 1 || f->height > 32767 || (long long)f->pitch_bytes < (long long)f->width * bpp) return 1;
    if ((wide && (f->pitch_bytes & 1)) || (c >= ADC_PIX_BAYER_RGGB8 && c <= ADC_PIX_BAYER_BGGR16 && (f->width < 2 || f->height < 2))) return 1;
    if (((c == ADC_PIX_YUYV || c == ADC_PIX_UYVY || c == ADC_PIX_NV12) && (f->width & 1)) || (c == ADC_PIX_NV12 && (f->height & 1))) return 1;
    const long long luma = (long long)f->height * f->pitch_bytes;
    return (c == ADC_PIX_NV12 ? luma / 2 * 3 : luma) <= 2147483647LL ? 0 : 1;
}
