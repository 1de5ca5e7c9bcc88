// tsdf_ray.h -- the per-ray arithmetic of the TSDF volume's ray caster (k_tsdf_raycast.hip; include/adcensus_c_api.h holds the
// definition in words, tests/tsdf_raycast_ref.py in numpy).  Plain inline functions on top of tsdf_voxel.h, shared by the kernel and
// by g++-compiled serial programs (tests/emul/emul_tsdf_raycast.cpp, tests/sanitize/stub_capi_tsdf_raycast.cpp): no HIP header, no
// handle.
//
// IEEE binary32, one rounding per operation, nothing fused (the pragma of adc_device_fn.h; the .hip files are compiled with
// -ffp-contract=off as well), divisions and the square root correctly rounded, every expression parenthesised in the order of the
// definition.  No float reaches an address: a sample's coordinates are bounded below 2^15 before they are converted and the cell is
// clipped in integers before any load.  One thread owns a ray: nothing here depends on an order of evaluation.  Every loop over the
// samples of a ray ends on the sample counter (max_steps), whatever the floats do.
#pragma once
#include "tsdf_voxel.h"

#define TSDF_RAY_LIVE 255u   // a ray that is still marching (never written to an output)
#define TSDF_RAY_MAX_DIM 8192
#define TSDF_RAY_MAX_STEPS 16384u

// the view as the arithmetic sees it: the caller's parameters and inv_voxel = 1.0f / voxel (one division on the host)
struct TsdfRayView {
    int W, H;
    float focal, cx, cy;
    float R[9], t[3];
    float z_near, z_far, step, skip, inv_voxel;
    uint32_t min_weight, max_steps;
};

// one ray in grid coordinates (voxel centres are the integers) and its clipped range of depths
struct TsdfRay {
    float g0[3], gd[3];
    float z_lo, z_hi;
    bool miss;
};

// what the march keeps from sample to sample
struct TsdfRayState {
    float Z, Z_prev, f_prev;
    uint32_t count;      // samples taken
    uint32_t status;     // TSDF_RAY_LIVE or ADC_TSDF_RAY_*
    bool prev_valid;
    float Zh;            // with ADC_TSDF_RAY_HIT: the depth
};

// one pixel's outputs
struct TsdfRayPixel {
    float depth;
    float normal[4];
    uint8_t bgr[3];
    uint8_t status;
};

// why a view is refused, or null (the entry points, the serial programs)
inline const char* tsdf_raycast_refusal(const adc_tsdf_raycast_params& p)
{
    if (p.width < 1 || p.height < 1 || p.width > TSDF_RAY_MAX_DIM || p.height > TSDF_RAY_MAX_DIM) return "width, height must lie in [1, 8192]";
    if (!(__builtin_isfinite(p.focal_px) && p.focal_px > 0.0f)) return "focal_px must be finite and > 0";
    if (!(__builtin_isfinite(p.cx) && __builtin_isfinite(p.cy))) return "cx, cy must be finite";
    for (int i = 0; i < 9; i++)
        if (!__builtin_isfinite(p.R[i])) return "R has a non-finite entry";
    for (int i = 0; i < 3; i++)
        if (!__builtin_isfinite(p.t[i])) return "t has a non-finite entry";
    if (!(__builtin_isfinite(p.z_near) && __builtin_isfinite(p.z_far) && 0.0f < p.z_near && p.z_near < p.z_far)) return "z_near, z_far must be finite with 0 < z_near < z_far";
    if (!(__builtin_isfinite(p.step) && p.step > 0.0f)) return "step must be finite and > 0";
    if (!(__builtin_isfinite(p.skip) && p.skip >= p.step)) return "skip must be finite and >= step";
    if (p.min_weight < 1u || p.min_weight > 65535u) return "min_weight must lie in [1, 65535]";
    if (p.max_steps < 1u || p.max_steps > TSDF_RAY_MAX_STEPS) return "max_steps must lie in [1, 16384]";
    if (p.flags != 0u) return "unknown flag";
    for (int i = 0; i < 8; i++)
        if (p.reserved_[i]) return "a reserved word is not 0";
    return nullptr;
}

inline TsdfRayView tsdf_ray_view(const adc_tsdf_raycast_params& p, const adc_tsdf_params& vol)
{
    TsdfRayView v;
    v.W = p.width; v.H = p.height;
    v.focal = p.focal_px; v.cx = p.cx; v.cy = p.cy;
    for (int i = 0; i < 9; i++) v.R[i] = p.R[i];
    for (int i = 0; i < 3; i++) v.t[i] = p.t[i];
    v.z_near = p.z_near; v.z_far = p.z_far; v.step = p.step; v.skip = p.skip;
    v.inv_voxel = 1.0f / vol.voxel;
    v.min_weight = p.min_weight; v.max_steps = p.max_steps;
    return v;
}

// The ray of pixel (x, y) and its clip against the box of voxel centres [0, n - 1] per axis (the slab method).  An axis along which
// the ray does not move (gd == 0) constrains nothing when g0 lies in [0, n - 1] and makes the ray a miss otherwise; any non-finite
// g0, gd or slab bound makes the ray a miss.
ADC_HD TsdfRay tsdf_ray_setup(const TsdfVol& v, const TsdfRayView& c, int x, int y)
{
    TsdfRay r;
    const float dx = ((float)x - c.cx) / c.focal;
    const float dy = ((float)y - c.cy) / c.focal;
    const float o[3] = {v.ox, v.oy, v.oz};
    const int n[3] = {v.nx, v.ny, v.nz};
    r.z_lo = c.z_near;
    r.z_hi = c.z_far;
    r.miss = false;
    for (int a = 0; a < 3; a++) {
        const float dw = ((c.R[a] * dx) + (c.R[3 + a] * dy)) + c.R[6 + a];
        const float cc = -(((c.R[a] * c.t[0]) + (c.R[3 + a] * c.t[1])) + (c.R[6 + a] * c.t[2]));
        r.g0[a] = ((cc - o[a]) * c.inv_voxel) - 0.5f;
        r.gd[a] = dw * c.inv_voxel;
        const float top = (float)(n[a] - 1);
        if (!(__builtin_isfinite(r.g0[a]) && __builtin_isfinite(r.gd[a]))) { r.miss = true; continue; }
        if (r.gd[a] == 0.0f) {
            if (!(r.g0[a] >= 0.0f && r.g0[a] <= top)) r.miss = true;
            continue;
        }
        const float t1 = (0.0f - r.g0[a]) / r.gd[a];
        const float t2 = (top - r.g0[a]) / r.gd[a];
        if (!(__builtin_isfinite(t1) && __builtin_isfinite(t2))) { r.miss = true; continue; }
        const float lo = t1 < t2 ? t1 : t2, hi = t1 < t2 ? t2 : t1;
        r.z_lo = lo > r.z_lo ? lo : r.z_lo;
        r.z_hi = hi < r.z_hi ? hi : r.z_hi;
    }
    if (!(r.z_lo <= r.z_hi)) r.miss = true;
    return r;
}

// the cell of the sample at depth Z and its fractions; false: not inside (0 <= cell < n - 1 on every axis, decided in integers)
ADC_HD bool tsdf_ray_cell(const TsdfVol& v, const TsdfRay& r, float Z, int cell[3], float frac[3])
{
    const int n[3] = {v.nx, v.ny, v.nz};
    bool inside = true;
    for (int a = 0; a < 3; a++) {
        const float g = r.g0[a] + (Z * r.gd[a]);
        if (!(__builtin_fabsf(g) < 32768.0f)) { cell[a] = -1; frac[a] = 0.0f; inside = false; continue; }
        const float fl = __builtin_floorf(g);
        cell[a] = (int)fl;
        frac[a] = g - fl;
        inside = inside && cell[a] >= 0 && cell[a] < n[a] - 1;
    }
    return inside;
}

ADC_HD size_t tsdf_ray_index(const TsdfVol& v, int i, int j, int k) { return ((size_t)k * (size_t)v.ny + (size_t)j) * (size_t)v.nx + (size_t)i; }

// the nearest voxel of an INSIDE sample: cell + (fraction >= 0.5f) per axis, at most n - 1
ADC_HD size_t tsdf_ray_nearest(const TsdfVol& v, const int cell[3], const float frac[3])
{
    return tsdf_ray_index(v, cell[0] + (frac[0] >= 0.5f ? 1 : 0), cell[1] + (frac[1] >= 0.5f ? 1 : 0), cell[2] + (frac[2] >= 0.5f ? 1 : 0));
}

// the eight corner words of an INSIDE cell, corner c = (i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)) as in tsdf_cell.h
ADC_HD void tsdf_ray_corners(const TsdfVol& v, const uint32_t* tsdf, const int cell[3], uint32_t w[8])
{
    const size_t n = tsdf_ray_index(v, cell[0], cell[1], cell[2]), sy = (size_t)v.nx, sz = (size_t)v.nx * (size_t)v.ny;
    w[0] = tsdf[n];           w[1] = tsdf[n + 1];
    w[2] = tsdf[n + sy];      w[3] = tsdf[n + sy + 1];
    w[4] = tsdf[n + sz];      w[5] = tsdf[n + sz + 1];
    w[6] = tsdf[n + sz + sy]; w[7] = tsdf[n + sz + sy + 1];
}

ADC_HD bool tsdf_ray_all_seen(const uint32_t w[8], uint32_t min_weight)
{
    bool seen = true;
    for (int c = 0; c < 8; c++) seen = seen && tsdf_seen(w[c], min_weight);
    return seen;
}

ADC_HD float tsdf_ray_lerp(float lo, float hi, float frac) { return lo + (frac * (hi - lo)); }

// the trilinear interpolant of the corners' t: x, then y, then z
ADC_HD float tsdf_ray_trilinear(const uint32_t w[8], const float frac[3])
{
    float t[8];
    for (int c = 0; c < 8; c++) t[c] = (float)tsdf_word_t(w[c]);
    const float c00 = tsdf_ray_lerp(t[0], t[1], frac[0]), c10 = tsdf_ray_lerp(t[2], t[3], frac[0]);
    const float c01 = tsdf_ray_lerp(t[4], t[5], frac[0]), c11 = tsdf_ray_lerp(t[6], t[7], frac[0]);
    const float c0 = tsdf_ray_lerp(c00, c10, frac[1]), c1 = tsdf_ray_lerp(c01, c11, frac[1]);
    return tsdf_ray_lerp(c0, c1, frac[2]);
}

ADC_HD void tsdf_ray_start(const TsdfRay& r, TsdfRayState* s)
{
    s->Z = r.z_lo; s->Z_prev = 0.0f; s->f_prev = 0.0f; s->Zh = 0.0f;
    s->count = 0u;
    s->prev_valid = false;
    s->status = r.miss ? (uint32_t)ADC_TSDF_RAY_MISS : TSDF_RAY_LIVE;
}

// The sample at depth Z (steps 1 to 4 of the definition): false = unseen; otherwise *f its value and *next the depth behind it.
ADC_HD bool tsdf_ray_sample(const TsdfVol& v, const TsdfRayView& c, const TsdfRay& r, const uint32_t* tsdf, float Z, float* f, float* next)
{
    int cell[3];
    float frac[3];
    *f = 0.0f;
    *next = Z + c.step;
    if (!tsdf_ray_cell(v, r, Z, cell, frac)) return false;
    const uint32_t nv = tsdf[tsdf_ray_nearest(v, cell, frac)];
    if (tsdf_seen(nv, c.min_weight) && tsdf_word_t(nv) == TSDF_Q) {
        *f = (float)TSDF_Q;
        *next = Z + c.skip;
        return true;
    }
    uint32_t w[8];
    tsdf_ray_corners(v, tsdf, cell, w);
    if (!tsdf_ray_all_seen(w, c.min_weight)) return false;
    *f = tsdf_ray_trilinear(w, frac);
    return true;
}

// Before a sample: false = the ray has ended (out of range: NO_SURFACE; out of samples: EXHAUSTED); otherwise the sample is counted.
ADC_HD bool tsdf_ray_begin(const TsdfRayView& c, const TsdfRay& r, TsdfRayState* s)
{
    if (!(s->Z <= r.z_hi)) { s->status = ADC_TSDF_RAY_NO_SURFACE; return false; }
    if (s->count >= c.max_steps) { s->status = ADC_TSDF_RAY_EXHAUSTED; return false; }
    s->count++;
    return true;
}

// Behind a sample: the ray stays live at its next depth or gets its final status (HIT with the depth, BEHIND).
ADC_HD void tsdf_ray_advance(TsdfRayState* s, bool valid, float f, float next)
{
    if (!valid) {
        s->prev_valid = false;
        s->Z = next;
        return;
    }
    if (f <= 0.0f) {
        if (s->prev_valid && s->f_prev > 0.0f) {
            s->status = ADC_TSDF_RAY_HIT;
            s->Zh = s->Z_prev + ((s->Z - s->Z_prev) * (s->f_prev / (s->f_prev - f)));
        } else {
            s->status = ADC_TSDF_RAY_BEHIND;
        }
        return;
    }
    s->prev_valid = true;
    s->f_prev = f;
    s->Z_prev = s->Z;
    s->Z = next;
}

// One turn of a LIVE ray.  Every turn either counts a sample (at most max_steps of them) or ends the ray.
ADC_HD void tsdf_ray_step(const TsdfVol& v, const TsdfRayView& c, const TsdfRay& r, const uint32_t* tsdf, TsdfRayState* s)
{
    if (!tsdf_ray_begin(c, r, s)) return;
    float f, next;
    const bool valid = tsdf_ray_sample(v, c, r, tsdf, s->Z, &f, &next);
    tsdf_ray_advance(s, valid, f, next);
}

// The outputs of a ray whose march has ended.  color may be null (no colour volume, or no colour asked for).
ADC_HD TsdfRayPixel tsdf_ray_finish(const TsdfVol& v, const TsdfRayView& c, const TsdfRay& r, const uint32_t* tsdf, const uint32_t* color, const TsdfRayState& s,
                                    bool want_normal)
{
    TsdfRayPixel o;
    o.depth = 0.0f;
    o.normal[0] = o.normal[1] = o.normal[2] = o.normal[3] = 0.0f;
    o.bgr[0] = o.bgr[1] = o.bgr[2] = 0;
    o.status = (uint8_t)s.status;
    if (s.status != ADC_TSDF_RAY_HIT) return o;
    o.depth = s.Zh;
    int cell[3];
    float frac[3];
    if (!tsdf_ray_cell(v, r, s.Zh, cell, frac)) return o;
    if (color) {
        const uint32_t cw = color[tsdf_ray_nearest(v, cell, frac)];
        if (cw >> 24) {
            o.bgr[0] = (uint8_t)((cw >> 16) & 0xFFu);
            o.bgr[1] = (uint8_t)((cw >> 8) & 0xFFu);
            o.bgr[2] = (uint8_t)(cw & 0xFFu);
        }
    }
    if (!want_normal) return o;
    uint32_t w[8];
    tsdf_ray_corners(v, tsdf, cell, w);
    if (!tsdf_ray_all_seen(w, c.min_weight)) return o;
    float t[8];
    uint32_t wm = 0xFFFFu;
    for (int k = 0; k < 8; k++) {
        t[k] = (float)tsdf_word_t(w[k]);
        wm = tsdf_word_w(w[k]) < wm ? tsdf_word_w(w[k]) : wm;
    }
    // the gradient of the trilinear interpolant: per axis the bilinear blend of the four corner differences along it
    const float gx = tsdf_ray_lerp(tsdf_ray_lerp(t[1] - t[0], t[3] - t[2], frac[1]), tsdf_ray_lerp(t[5] - t[4], t[7] - t[6], frac[1]), frac[2]);
    const float gy = tsdf_ray_lerp(tsdf_ray_lerp(t[2] - t[0], t[3] - t[1], frac[0]), tsdf_ray_lerp(t[6] - t[4], t[7] - t[5], frac[0]), frac[2]);
    const float gz = tsdf_ray_lerp(tsdf_ray_lerp(t[4] - t[0], t[5] - t[1], frac[0]), tsdf_ray_lerp(t[6] - t[2], t[7] - t[3], frac[0]), frac[1]);
    const float L = __builtin_sqrtf(((gx * gx) + (gy * gy)) + (gz * gz));
    if (!(__builtin_isfinite(L) && L > 0.0f)) return o;
    const float nx = gx / L, ny = gy / L, nz = gz / L;
    o.normal[0] = ((c.R[0] * nx) + (c.R[1] * ny)) + (c.R[2] * nz);
    o.normal[1] = ((c.R[3] * nx) + (c.R[4] * ny)) + (c.R[5] * nz);
    o.normal[2] = ((c.R[6] * nx) + (c.R[7] * ny)) + (c.R[8] * nz);
    o.normal[3] = (float)wm;
    return o;
}

// the whole ray, serially (the serial programs; the kernel runs the same three functions with its own loop over the wave)
inline TsdfRayPixel tsdf_ray_cast(const TsdfVol& v, const TsdfRayView& c, const uint32_t* tsdf, const uint32_t* color, int x, int y, uint32_t* samples)
{
    const TsdfRay r = tsdf_ray_setup(v, c, x, y);
    TsdfRayState s;
    tsdf_ray_start(r, &s);
    while (s.status == TSDF_RAY_LIVE) tsdf_ray_step(v, c, r, tsdf, &s);
    *samples = s.count;
    return tsdf_ray_finish(v, c, r, tsdf, color, s, true);
}
