// tsdf_fuse.h -- the per-pixel observation weight and the weighted, interpolating voxel update of the stereo-aware TSDF fusion
// (k_tsdf_fuse.hip; include/adcensus_c_api.h holds the definition in words, tests/tsdf_fuse_ref.py in numpy).  Plain inline functions
// shared by the kernels and by g++-compiled serial programs (tests/emul/emul_tsdf_fuse.cpp, tests/sanitize/stub_capi_tsdf_fuse.cpp): no
// HIP header, no handle.  The arithmetic rules are those of tsdf_voxel.h, whose steps 1 to 5, 7, 8 and 10 are repeated or reused here;
// that header itself is unchanged, so that k_tsdf_integrate stays the code it was.
#pragma once
#include "tsdf_voxel.h"

enum { TSDF_UNWEIGHTED = 4 }; // behind TSDF_SKIP .. TSDF_UPDATE: the pixel's weight is 0

static const adc_tsdf_weight_params TSDF_WEIGHT_DEFAULT = {{16, 4, 1, 0}, 0.0f, 0u, 4u, 1.0f, {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}};
static const adc_tsdf_fuse_params TSDF_FUSE_DEFAULT = {0u, 0.0f, {0u, 0u, 0u, 0u, 0u, 0u}};

inline const char* tsdf_weight_params_refusal(const adc_tsdf_weight_params& p)
{
    if (!(p.min_confidence >= 0.0f && p.min_confidence <= 1.0f)) return "min_confidence must lie in [0, 1]";
    if (p.flags & ~ADC_TSDF_W_SCALE_CONFIDENCE) return "unknown flag";
    if (p.depth_power != 0u && p.depth_power != 2u && p.depth_power != 4u) return "depth_power must be 0, 2 or 4";
    if (!(__builtin_isfinite(p.z_ref) && p.z_ref > 0.0f)) return "z_ref must be finite and > 0";
    for (int i = 0; i < 11; i++)
        if (p.reserved_[i]) return "a reserved word is not 0";
    return nullptr;
}

inline const char* tsdf_fuse_params_refusal(const adc_tsdf_fuse_params& p)
{
    if (p.flags & ~ADC_TSDF_FUSE_BILINEAR) return "unknown flag";
    if (!(__builtin_isfinite(p.interp_gap) && p.interp_gap >= 0.0f)) return "interp_gap must be finite and >= 0";
    for (int i = 0; i < 6; i++)
        if (p.reserved_[i]) return "a reserved word is not 0";
    return nullptr;
}

// The weight of one pixel (steps 1 to 5 of the definition); -1: the pixel has no depth.  has_prov / has_conf: the maps were given.
// *below: the confidence test of step 4 failed.
ADC_HD int tsdf_obs_weight(const RegSource& s, const adc_tsdf_weight_params& p, float v, bool has_prov, uint32_t code, bool has_conf, float conf, bool* below)
{
    *below = false;
    float D;
    if (!reg_source_z(s, v, &D)) return -1;
    const uint32_t fill = has_prov ? ((code >> ADC_PROV_FILL_SHIFT) & 3u) : (uint32_t)ADC_FILL_WTA;
    uint32_t wc = p.class_weight[fill];
    if (has_prov && (code & ADC_PROV_SPECKLE)) wc = 0u;
    if (has_conf && fill == (uint32_t)ADC_FILL_WTA) {
        if (!(conf >= p.min_confidence)) {
            wc = 0u;
            *below = true;
        } else if (p.flags & ADC_TSDF_W_SCALE_CONFIDENCE) {
            const uint32_t cq = (uint32_t)(int)__builtin_floorf(__builtin_fminf(__builtin_fmaxf(conf, 0.0f), 1.0f) * 256.0f + 0.5f);
            wc = (wc * cq + 128u) >> 8;
        }
    }
    if (wc == 0u || !__builtin_isfinite(D)) return 0;
    const float g = p.z_ref / D;
    float sc = (float)wc;
    if (p.depth_power == 2u) sc = sc * (g * g);
    else if (p.depth_power == 4u) sc = sc * ((g * g) * (g * g));
    return (int)__builtin_floorf(__builtin_fminf(sc, 255.0f) + 0.5f);
}

// Steps 1 to 8 of the fuse for voxel i of a row, as tsdf_decide with steps 6a and 6b: *wo is the observation's weight (with
// TSDF_UPDATE), *interp says whether D came from the four pixels around (u, v) (with TSDF_UPDATE or TSDF_OCCLUDED).  weight may be null.
// Every load stands behind an integer clip.
ADC_HD int tsdf_fuse_decide(const TsdfVol& v, const TsdfCam& c, const TsdfRow& r, int i, const float* map, const uint8_t* weight, bool bilinear, float gap, int* q,
                            int* pixel, bool* band, uint32_t* wo, bool* interp)
{
    *interp = false;
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
    *wo = weight ? (uint32_t)weight[*pixel] : 1u;
    if (*wo == 0u) return TSDF_UNWEIGHTED;
    if (bilinear) {
        const int x0 = (int)__builtin_floorf(pu), y0 = (int)__builtin_floorf(pv);
        if (0 <= x0 && x0 + 1 < c.W && 0 <= y0 && y0 + 1 < c.H) {
            const float* m0 = map + (y0 * c.W + x0);
            const float a = m0[0], b = m0[1], cc = m0[c.W], d = m0[c.W + 1];
            float za, zb, zc, zd;
            const bool va = reg_source_z(c.src, a, &za), vb = reg_source_z(c.src, b, &zb), vc = reg_source_z(c.src, cc, &zc), vd = reg_source_z(c.src, d, &zd);
            if (va && vb && vc && vd) {
                const float hi = __builtin_fmaxf(__builtin_fmaxf(a, b), __builtin_fmaxf(cc, d)), lo = __builtin_fminf(__builtin_fminf(a, b), __builtin_fminf(cc, d));
                if ((hi - lo) <= gap) {
                    const float fx = pu - (float)x0, fy = pv - (float)y0;
                    const float top = a + fx * (b - a), bot = cc + fx * (d - cc);
                    const float val = top + fy * (bot - top);
                    float Dv;
                    if (reg_source_z(c.src, val, &Dv)) {
                        D = Dv;
                        *interp = true;
                    }
                }
            }
        }
    }
    const float sdf = D - Zc;
    if (!(sdf >= -v.trunc)) return TSDF_OCCLUDED;
    const float f = __builtin_fminf(sdf * v.inv_trunc, 1.0f);
    *q = (int)__builtin_floorf(f * 32767.0f + 0.5f);
    *band = __builtin_fabsf(sdf) <= v.trunc;
    return TSDF_UPDATE;
}

// step 9': the numerator needs 64 bits only behind 2^32 - 1 (w near its cap with a large wo); below that one 32-bit division serves
ADC_HD uint32_t tsdf_fuse_update(uint32_t word, int q, uint32_t wo, uint32_t max_weight)
{
    const uint32_t w = tsdf_word_w(word), m = w + wo;
    const unsigned long long num = (unsigned long long)(uint32_t)(tsdf_word_t(word) + TSDF_Q) * w + (unsigned long long)(uint32_t)(q + TSDF_Q) * wo + m / 2u;
    const uint32_t mean = num <= 0xFFFFFFFFull ? (uint32_t)num / m : (uint32_t)(num / m);
    const int t = (int)mean - TSDF_Q;
    const uint32_t wn = m < max_weight ? m : max_weight;
    return ((uint32_t)t & 0xFFFFu) | (wn << 16);
}
