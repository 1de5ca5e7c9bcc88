// normals_fit.h -- plane-fit arithmetic of the surface normals from a disparity map (k_normals.hip; include/adcensus_c_api.h holds
// the definition in words, tests/normals_ref.py in numpy).  Plain inline functions shared by the kernel and by a g++-compiled serial
// program (tests/emul/emul_normals.cpp): no HIP header, no handle.
//
// Integers up to the four determinants (int32 sums, int64 products: exact, so the order of evaluation does not matter), then IEEE
// binary32, one rounding per operation, nothing fused (the pragma of adc_device_fn.h; the .hip files are compiled with
// -ffp-contract=off as well), divisions and the square root correctly rounded, every expression parenthesised in the order of the
// definition.  Each int64 -> float conversion is one rounding to nearest even.
#pragma once
#include <stdint.h>
#include "../../include/adcensus_c_api.h"
#include "adc_device_fn.h"

#define NRM_Q_NONE 0x40000000 // "not usable or outside the image": farther than any gate from every q in [0, 2^25)

// what the arithmetic takes from the calibration
struct NrmCam {
    float focal, cx, cy, doffs;
};

// the nine sums over the support of one centre
struct NrmSums {
    int32_t n, sx, sy, sxx, sxy, syy, se, sxe, sye;
};

enum { NRM_UNUSABLE = 0, NRM_FITTED = 1, NRM_FEW_POINTS = 2, NRM_DEGENERATE = 3 };

// one output pixel: v = the four floats of `normals`, bytes = the four bytes of `normals8` (byte k in bits 8k..8k+7), cls = NRM_*
struct NrmPixel {
    float v[4];
    uint32_t bytes;
    int cls;
};

// fixed-point disparity of a map value, NRM_Q_NONE where the value is not usable
ADC_HD int32_t nrm_quantise(float d)
{
    const float a = __builtin_fabsf(d);
    if (!(__builtin_isfinite(a) && a < 32768.0f)) return NRM_Q_NONE;
    return (int32_t)__builtin_rintf(a * 1024.0f);
}

// the gate |e| <= G in one unsigned comparison (|e| <= 2^30, 0 <= G <= 65536: nothing overflows)
ADC_HD bool nrm_gate(int32_t e, int32_t G) { return (uint32_t)(e + G) <= (uint32_t)(2 * G); }

ADC_HD void nrm_add_tap(NrmSums* s, int dx, int dy, int32_t e)
{
    s->n += 1;
    s->sx += dx; s->sy += dy;
    s->sxx += dx * dx; s->sxy += dx * dy; s->syy += dy * dy;
    s->se += e; s->sxe += dx * e; s->sye += dy * e;
}

ADC_HD int64_t nrm_det3(int64_t a, int64_t b, int64_t c, int64_t d, int64_t e, int64_t f, int64_t g, int64_t h, int64_t i)
{
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
}

ADC_HD uint32_t nrm_byte(float v) { return (uint32_t)(uint8_t)((int)__builtin_rintf(v * 127.0f) + 128); }

// from the sums of a USABLE centre (x, y) with fixed-point disparity qc to its outputs
ADC_HD NrmPixel nrm_fit(const NrmSums& s, int32_t qc, int x, int y, const NrmCam& c, int32_t min_points)
{
    NrmPixel o;
    o.v[0] = o.v[1] = o.v[2] = o.v[3] = 0.0f;
    o.bytes = 0;
    o.cls = NRM_FEW_POINTS;
    if (s.n < min_points) return o;
    o.cls = NRM_DEGENERATE;
    const int64_t Dt = nrm_det3(s.sxx, s.sxy, s.sx, s.sxy, s.syy, s.sy, s.sx, s.sy, s.n);
    if (!(Dt > 0)) return o;
    const int64_t Na = nrm_det3(s.sxe, s.sxy, s.sx, s.sye, s.syy, s.sy, s.se, s.sy, s.n);
    const int64_t Nb = nrm_det3(s.sxx, s.sxe, s.sx, s.sxy, s.sye, s.sy, s.sx, s.se, s.n);
    const int64_t Nc = nrm_det3(s.sxx, s.sxy, s.sxe, s.sxy, s.syy, s.sye, s.sx, s.sy, s.se);
    const float Df = (float)Dt;
    const float ga = ((float)Na / Df) * 0x1p-10f;
    const float gb = ((float)Nb / Df) * 0x1p-10f;
    const float dc = ((float)qc * 0x1p-10f) + (((float)Nc / Df) * 0x1p-10f);
    const float sd = dc + c.doffs;
    if (!(sd > 0.0f)) return o;
    const float nx = ga * c.focal;
    const float ny = gb * c.focal;
    const float nz = ((ga * (c.cx - (float)x)) + (gb * (c.cy - (float)y))) + sd;
    const float L = __builtin_sqrtf(((nx * nx) + (ny * ny)) + (nz * nz));
    if (!(__builtin_isfinite(L) && L > 0.0f)) return o;
    o.cls = NRM_FITTED;
    o.v[0] = -nx / L;
    o.v[1] = -ny / L;
    o.v[2] = -nz / L;
    o.v[3] = (float)s.n;
    o.bytes = nrm_byte(o.v[0]) | (nrm_byte(o.v[1]) << 8) | (nrm_byte(o.v[2]) << 16) | 0xff000000u;
    return o;
}
