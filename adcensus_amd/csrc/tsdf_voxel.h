// tsdf_voxel.h -- the per-voxel arithmetic of the TSDF volume (k_tsdf.hip; include/adcensus_c_api.h holds the definition in words,
// tests/tsdf_ref.py in numpy).  Plain inline functions shared by the kernels and by g++-compiled serial programs
// (tests/emul/emul_tsdf.cpp, tests/sanitize/stub_capi_tsdf.cpp): no HIP header, no handle.
//
// IEEE binary32, one rounding per operation, nothing fused (the pragma of adc_device_fn.h; the .hip files are compiled with
// -ffp-contract=off as well), divisions correctly rounded, every expression parenthesised in the order of the definition.  No float
// reaches an address: u and v are bounded below 2^15 before they are converted and the pixel is clipped in integers.  Everything a
// voxel accumulates is an integer, and one thread owns a voxel: nothing here depends on an order of evaluation.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/adcensus_c_api.h"
#include "adc_device_fn.h"
#include "reg_project.h" // RegSource, reg_source_z, reg_float_bits

#define TSDF_Q 32767      // t counts units of trunc / TSDF_Q
#define TSDF_MAX_VOXELS (1u << 30)

// the volume as the arithmetic sees it: the caller's parameters and inv_trunc = 1.0f / trunc (one division on the host)
struct TsdfVol {
    int nx, ny, nz;
    float voxel, ox, oy, oz, trunc, inv_trunc, z_min, z_max;
    uint32_t max_weight;
};

// one frame: what to make of a map value, the rectified left camera, world -> camera
struct TsdfCam {
    RegSource src;
    float R[9], t[3];
    int W, H;
};

// what a voxel does with a frame
enum { TSDF_SKIP = 0, TSDF_NO_DEPTH = 1, TSDF_OCCLUDED = 2, TSDF_UPDATE = 3 };

// why a set of parameters is refused, or null (the entry points, the serial programs)
inline const char* tsdf_params_refusal(const adc_tsdf_params& p)
{
    if (p.nx < 4 || p.ny < 4 || p.nz < 4 || p.nx > ADC_TSDF_MAX_DIM || p.ny > ADC_TSDF_MAX_DIM || p.nz > ADC_TSDF_MAX_DIM) return "nx, ny, nz must lie in [4, 2048]";
    if (p.nx & 3) return "nx must be a multiple of 4";
    if ((unsigned long long)p.nx * (unsigned long long)p.ny * (unsigned long long)p.nz > (unsigned long long)TSDF_MAX_VOXELS) return "nx * ny * nz must not exceed 2^30";
    if (!(__builtin_isfinite(p.voxel) && p.voxel > 0.0f)) return "voxel must be finite and > 0";
    if (!(__builtin_isfinite(p.origin[0]) && __builtin_isfinite(p.origin[1]) && __builtin_isfinite(p.origin[2]))) return "origin must be finite";
    if (!(__builtin_isfinite(p.trunc) && p.trunc > 0.0f)) return "trunc must be finite and > 0";
    if (!(p.z_min >= 0.0f && p.z_min <= p.z_max)) return "z_min, z_max must satisfy 0 <= z_min <= z_max (no NaN)";
    if (p.max_weight < 1u || p.max_weight > 65535u) return "max_weight must lie in [1, 65535]";
    if (p.flags & ~ADC_TSDF_COLOR) return "unknown flag";
    if (p.reserved_[0] | p.reserved_[1] | p.reserved_[2] | p.reserved_[3]) return "a reserved word is not 0";
    return nullptr;
}

inline const char* tsdf_frame_refusal(const adc_tsdf_frame& f)
{
    if (f.kind != ADC_REG_FROM_DISPARITY && f.kind != ADC_REG_FROM_DEPTH) return "kind must be ADC_REG_FROM_DISPARITY or ADC_REG_FROM_DEPTH";
    const adc_calib& c = f.calib;
    if (!(__builtin_isfinite(c.focal_px) && __builtin_isfinite(c.baseline) && __builtin_isfinite(c.cx) && __builtin_isfinite(c.cy) && __builtin_isfinite(c.doffs)))
        return "the calibration has a non-finite field";
    if (!(c.focal_px > 0.0f)) return "the calibration's focal_px must be positive";
    for (int i = 0; i < 9; i++)
        if (!__builtin_isfinite(f.R[i])) return "R has a non-finite entry";
    for (int i = 0; i < 3; i++)
        if (!__builtin_isfinite(f.t[i])) return "t has a non-finite entry";
    if (f.flags != 0u) return "unknown flag";
    if (f.reserved_[0] | f.reserved_[1] | f.reserved_[2] | f.reserved_[3] | f.reserved_[4]) return "a reserved word is not 0";
    return nullptr;
}

inline TsdfVol tsdf_vol(const adc_tsdf_params& p)
{
    TsdfVol v;
    v.nx = p.nx; v.ny = p.ny; v.nz = p.nz;
    v.voxel = p.voxel;
    v.ox = p.origin[0]; v.oy = p.origin[1]; v.oz = p.origin[2];
    v.trunc = p.trunc;
    v.inv_trunc = 1.0f / p.trunc;
    v.z_min = p.z_min; v.z_max = p.z_max;
    v.max_weight = p.max_weight;
    return v;
}

inline TsdfCam tsdf_cam(const adc_tsdf_frame& f, int W, int H)
{
    TsdfCam c;
    c.src.kind = f.kind;
    c.src.fb = f.calib.focal_px * f.calib.baseline;
    c.src.focal = f.calib.focal_px; c.src.cx = f.calib.cx; c.src.cy = f.calib.cy; c.src.doffs = f.calib.doffs;
    for (int i = 0; i < 9; i++) c.R[i] = f.R[i];
    for (int i = 0; i < 3; i++) c.t[i] = f.t[i];
    c.W = W; c.H = H;
    return c;
}

// the centre of voxel index i on an axis with origin o (step 1)
ADC_HD float tsdf_centre(float o, int i, float voxel) { return o + ((float)i + 0.5f) * voxel; }

// The terms of step 2 that are the same along a row of voxels (j and k fixed): the products with yw and zw.  The sums stay with the
// voxel, in the order of the definition.
struct TsdfRow {
    float ry[3], rz[3]; // R[1] * yw, R[4] * yw, R[7] * yw; R[2] * zw, R[5] * zw, R[8] * zw
};

ADC_HD TsdfRow tsdf_row(const TsdfVol& v, const TsdfCam& c, int j, int k)
{
    const float yw = tsdf_centre(v.oy, j, v.voxel), zw = tsdf_centre(v.oz, k, v.voxel);
    TsdfRow r;
    r.ry[0] = c.R[1] * yw; r.ry[1] = c.R[4] * yw; r.ry[2] = c.R[7] * yw;
    r.rz[0] = c.R[2] * zw; r.rz[1] = c.R[5] * zw; r.rz[2] = c.R[8] * zw;
    return r;
}

// Steps 1 to 8 for voxel i of a row: what the voxel does; with TSDF_UPDATE *q is the quantised distance, *pixel the raster index of
// the pixel it saw and *band says whether fabsf(sdf) <= trunc (the colour's condition).  Reads the map only behind the integer clip.
ADC_HD int tsdf_decide(const TsdfVol& v, const TsdfCam& c, const TsdfRow& r, int i, const float* map, int* q, int* pixel, bool* band)
{
    const float xw = tsdf_centre(v.ox, i, v.voxel);
    const float Xc = ((c.R[0] * xw + r.ry[0]) + r.rz[0]) + c.t[0];
    const float Yc = ((c.R[3] * xw + r.ry[1]) + r.rz[1]) + c.t[1];
    const float Zc = ((c.R[6] * xw + r.ry[2]) + r.rz[2]) + c.t[2];
    if (!(__builtin_isfinite(Zc) && Zc > 0.0f && v.z_min <= Zc && Zc <= v.z_max)) return TSDF_SKIP;
    const float rz = 1.0f / Zc;
    const float pu = ((Xc * c.src.focal) * rz) + c.src.cx;
    const float pv = ((Yc * c.src.focal) * rz) + c.src.cy;
    if (!(__builtin_fabsf(pu) < 32768.0f && __builtin_fabsf(pv) < 32768.0f)) return TSDF_SKIP;
    const int x = (int)__builtin_floorf(pu + 0.5f), y = (int)__builtin_floorf(pv + 0.5f);
    if (x < 0 || x >= c.W || y < 0 || y >= c.H) return TSDF_SKIP;
    *pixel = y * c.W + x;
    float D;
    if (!reg_source_z(c.src, map[*pixel], &D)) return TSDF_NO_DEPTH;
    const float sdf = D - Zc;
    if (!(sdf >= -v.trunc)) return TSDF_OCCLUDED;
    const float f = __builtin_fminf(sdf * v.inv_trunc, 1.0f);
    *q = (int)__builtin_floorf(f * 32767.0f + 0.5f);
    *band = __builtin_fabsf(sdf) <= v.trunc;
    return TSDF_UPDATE;
}

// t and w of a voxel word (a stored -32768 is read as -32767)
ADC_HD int tsdf_word_t(uint32_t word) { return adc_imax((int)(int16_t)(uint16_t)(word & 0xFFFFu), -TSDF_Q); }
ADC_HD uint32_t tsdf_word_w(uint32_t word) { return word >> 16; }

// step 9: (t + 32767) * w + (q + 32767) + m / 2 < 2^32, all terms non-negative
ADC_HD uint32_t tsdf_update(uint32_t word, int q, uint32_t max_weight)
{
    const uint32_t w = tsdf_word_w(word), m = w + 1u;
    const uint32_t num = (uint32_t)(tsdf_word_t(word) + TSDF_Q) * w + (uint32_t)(q + TSDF_Q) + m / 2u;
    const int t = (int)(num / m) - TSDF_Q;
    const uint32_t wn = m < max_weight ? m : max_weight;
    return ((uint32_t)t & 0xFFFFu) | (wn << 16);
}

// step 10: bgr points at the B,G,R bytes of the pixel
ADC_HD uint32_t tsdf_colour_update(uint32_t cword, const uint8_t* bgr, uint32_t max_weight)
{
    const uint32_t cw = cword >> 24, cm = cw + 1u, cap = max_weight < 255u ? max_weight : 255u;
    const uint32_t r = ((cword & 0xFFu) * cw + (uint32_t)bgr[2] + cm / 2u) / cm;
    const uint32_t g = (((cword >> 8) & 0xFFu) * cw + (uint32_t)bgr[1] + cm / 2u) / cm;
    const uint32_t b = (((cword >> 16) & 0xFFu) * cw + (uint32_t)bgr[0] + cm / 2u) / cm;
    return r | (g << 8) | (b << 16) | ((cm < cap ? cm : cap) << 24);
}

// extraction: a voxel counts as seen; a pair of voxel words is a crossing
ADC_HD bool tsdf_seen(uint32_t word, uint32_t min_weight) { return tsdf_word_w(word) >= min_weight; }
ADC_HD bool tsdf_crossing(uint32_t wa, uint32_t wb, uint32_t min_weight)
{
    return tsdf_seen(wa, min_weight) && tsdf_seen(wb, min_weight) && ((tsdf_word_t(wa) < 0) != (tsdf_word_t(wb) < 0));
}

// the record of the crossing between voxel a = (i, j, k) and its neighbour b on `axis` (0 x, 1 y, 2 z): four words of an adc_point;
// ca, cb: the colour words (0 without a colour volume)
ADC_HD void tsdf_point(const TsdfVol& v, int i, int j, int k, int axis, uint32_t wa, uint32_t wb, uint32_t ca, uint32_t cb, uint32_t out[4])
{
    const float ta = (float)tsdf_word_t(wa), tb = (float)tsdf_word_t(wb);
    const float s = ta / (ta - tb);
    const float d = s * v.voxel;
    float p[3] = {tsdf_centre(v.ox, i, v.voxel), tsdf_centre(v.oy, j, v.voxel), tsdf_centre(v.oz, k, v.voxel)};
    if (axis == 0) p[0] = p[0] + d;
    else if (axis == 1) p[1] = p[1] + d;
    else p[2] = p[2] + d;
    const uint32_t wm = tsdf_word_w(wa) < tsdf_word_w(wb) ? tsdf_word_w(wa) : tsdf_word_w(wb);
    const uint32_t col = (s <= 0.5f ? ca : cb) & 0xFFFFFFu;
    out[0] = reg_float_bits(p[0]);
    out[1] = reg_float_bits(p[1]);
    out[2] = reg_float_bits(p[2]);
    out[3] = col | ((wm < 255u ? wm : 255u) << 24);
}
