// reg_project.h -- projection and footprint arithmetic of the registration of depth into a second camera (k_register.hip;
// include/adcensus_c_api.h holds the definition in words, tests/register_ref.py in numpy).  Plain inline functions shared by the
// kernels and by a g++-compiled serial program (tests/emul/emul_register.cpp): no HIP header, no handle.
//
// IEEE binary32, one rounding per operation, nothing fused (the pragma of adc_device_fn.h; the .hip files are compiled with
// -ffp-contract=off as well), divisions correctly rounded, every expression parenthesised in the order of the definition.
// No float reaches an address: the in-range test bounds u and v below 2^15 before they are converted, the clip is done in integers.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/adcensus_c_api.h"
#include "adc_device_fn.h"

// the source side of a request: what to make of a map value, and the rectified left camera
struct RegSource {
    int kind;                 // ADC_REG_FROM_DISPARITY / ADC_REG_FROM_DEPTH
    float fb, focal, cx, cy, doffs;
};

#define REG_KEY_EMPTY (~0ull) // no finite positive float has the high word 0xffffffff

ADC_HD uint32_t reg_float_bits(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
#endif
}

ADC_HD float reg_bits_float(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}

// Z of one map value; false: the pixel has no depth
ADC_HD bool reg_source_z(const RegSource& s, float v, float* z)
{
    if (s.kind == ADC_REG_FROM_DEPTH) {
        *z = v;
        return __builtin_isfinite(v) && v > 0.0f;
    }
    const float a = __builtin_fabsf(v);
    const float sum = a + s.doffs;
    const bool ok = __builtin_isfinite(a) && sum > 0.0f;
    *z = ok ? s.fb / sum : ADC_INVALID_FLOAT;
    return ok;
}

// the source point (xs, ys, Z) in the target image; false: behind the camera or out of range (then *u, *v, *zt are not to be used)
ADC_HD bool reg_project(const RegSource& s, const adc_reg_target& T, float xs, float ys, float Z, float* u, float* v, float* zt)
{
    const float X = ((xs - s.cx) * Z) / s.focal;
    const float Y = ((ys - s.cy) * Z) / s.focal;
    const float Xt = ((T.R[0] * X + T.R[1] * Y) + T.R[2] * Z) + T.t[0];
    const float Yt = ((T.R[3] * X + T.R[4] * Y) + T.R[5] * Z) + T.t[1];
    const float Zt = ((T.R[6] * X + T.R[7] * Y) + T.R[8] * Z) + T.t[2];
    *zt = Zt;
    if (!(__builtin_isfinite(Zt) && Zt > 0.0f)) return false;
    const float x = Xt / Zt, y = Yt / Zt;
    const float x2 = x * x, y2 = y * y, r2 = x2 + y2, xy = x * y;
    const float rad = 1.0f + r2 * (T.k1 + r2 * (T.k2 + r2 * T.k3));
    const float xd = (x * rad + (2.0f * T.p1) * xy) + T.p2 * (r2 + 2.0f * x2);
    const float yd = (y * rad + T.p1 * (r2 + 2.0f * y2)) + (2.0f * T.p2) * xy;
    *u = T.fx * xd + T.cx;
    *v = T.fy * yd + T.cy;
    return __builtin_fabsf(*u) < 32768.0f && __builtin_fabsf(*v) < 32768.0f;
}

// the target pixels [i0, i1] x [j0, j1] a source pixel writes its key to, already clipped and capped
struct RegFoot {
    int j0, j1, i0, i1;
    float zc;
};

// one axis: the centres in [lo, hi) of the two corner coordinates (splat) or the centre's nearest pixel, clipped to [0, n) and capped
ADC_HD void reg_extent(float a, float b, float c, bool splat, int n, int* lo, int* hi)
{
    int e0, e1;
    if (splat) {
        e0 = (int)__builtin_ceilf(__builtin_fminf(a, b));
        e1 = (int)__builtin_ceilf(__builtin_fmaxf(a, b)) - 1;
    } else {
        e0 = e1 = (int)__builtin_floorf(c + 0.5f);
    }
    e0 = adc_imax(e0, 0);
    e1 = adc_imin(e1, n - 1);
    e1 = adc_imin(e1, e0 + ADC_REG_MAX_SPLAT - 1);
    *lo = e0;
    *hi = e1;
}

// false: the pixel writes nothing (a projection behind or out of range, or an empty footprint)
ADC_HD bool reg_footprint(const RegSource& s, const adc_reg_target& T, int x, int y, float Z, bool splat, RegFoot* f)
{
    const float fx = (float)x, fy = (float)y;
    float uc, vc, ua, va, ub, vb, za, zb;
    if (!reg_project(s, T, fx, fy, Z, &uc, &vc, &f->zc)) return false;
    if (!reg_project(s, T, fx - 0.5f, fy - 0.5f, Z, &ua, &va, &za)) return false;
    if (!reg_project(s, T, fx + 0.5f, fy + 0.5f, Z, &ub, &vb, &zb)) return false;
    reg_extent(ua, ub, uc, splat, T.width, &f->j0, &f->j1);
    reg_extent(va, vb, vc, splat, T.height, &f->i0, &f->i1);
    return f->j0 <= f->j1 && f->i0 <= f->i1;
}

ADC_HD unsigned long long reg_key(float zc, int W, int x, int y)
{
    return ((unsigned long long)reg_float_bits(zc) << 32) | (unsigned long long)(uint32_t)(y * W + x);
}

// colour aligned to depth: the target pixel (i, j) a source pixel takes its colour from; false: none
ADC_HD bool reg_align_tap(const RegSource& s, const adc_reg_target& T, int x, int y, float v, int* i, int* j)
{
    float Z, uc, vc, zc;
    if (!reg_source_z(s, v, &Z)) return false;
    if (!reg_project(s, T, (float)x, (float)y, Z, &uc, &vc, &zc)) return false;
    *j = (int)__builtin_floorf(uc + 0.5f);
    *i = (int)__builtin_floorf(vc + 0.5f);
    return *j >= 0 && *j < T.width && *i >= 0 && *i < T.height;
}
