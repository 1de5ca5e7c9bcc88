// tsdf_track.h -- the arithmetic of frame-to-model camera tracking (k_tsdf_track.hip; include/adcensus_c_api.h holds the definition in
// words, tests/tsdf_track_ref.py in numpy).  Plain inline functions on top of reg_project.h, shared by the two kernels and by
// g++-compiled serial programs (tests/emul/emul_tsdf_track.cpp): no HIP header, no handle.
//
// Per pixel: IEEE binary32, one rounding per operation, nothing fused (the pragma of adc_device_fn.h; the .hip files are compiled with
// -ffp-contract=off as well), divisions correctly rounded, every expression parenthesised in the order of the definition.  No float
// reaches an address: u and v are bounded below 2^15 before they are converted and the model pixel is clipped in integers.  What a
// pixel contributes is seven integers, and everything summed over pixels is an int64: no sum depends on the order of the pixels.
//
// No overflow.  A pixel is `used` only when each of its seven scaled values s (the three a_i = (Pm x nm)_i / z_far, the three nm_i and
// r / max_dist) satisfies |s| < 4, so |q| = |rintf(s * 65536)| <= 4 * 65536 = 2^18 (the product s * 65536 is exact, a power of two) and
// a product of two of them is at most 2^36.  The entry points refuse more than 2^26 participating pixels, so the magnitude of every one
// of the 28 sums stays at or below 2^26 * 2^36 = 2^62 < 2^63.  (For a unit normal and a pixel inside the distance gate the residual and
// translation entries stay below 2^16 + 1; only the rotation entries need the range up to 4.)  TRACK_Q, the bound 4 and
// TRACK_MAX_PIXELS may change only together with this derivation.
//
// The solve: IEEE binary64, + - * / only, a fixed order, nothing fused; the two square roots at its end fill the record's norms and
// the rms and are read by no decision (every threshold is compared in squares).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/adcensus_c_api.h"
#include "adc_device_fn.h"
#include "reg_project.h" // RegSource, reg_source_z
#include "tsdf_voxel.h"  // tsdf_frame_refusal

#define TRACK_Q 65536.0f
#define TRACK_RANGE 4.0f
#define TRACK_MAX_PIXELS (1u << 26)
#define TRACK_MAX_DIM 8192
#define TRACK_SUMS 28 // [0, 21) the upper triangle of J J^T by rows, [21, 27) J * r, [27] r * r
#define TRACK_COUNTS 7
// what a pixel counts as (the order of the counts behind `pixels` in adc_track_result)
enum { TRACK_NO_DEPTH = 0, TRACK_OUTSIDE = 1, TRACK_NO_MODEL = 2, TRACK_FAR = 3, TRACK_ANGLE = 4, TRACK_OUT_OF_RANGE = 5, TRACK_USED = 6 };

static const adc_track_params TRACK_DEFAULT = {10u, 1u, 0.1f, 0.8f, 8.0f, 64u, 1.0e-5f, 1.0e-5f, 0.5f, 0.5f, 0.0f, 1.0e-6f, 0u, {0u, 0u, 0u}};

// the current frame's map and the model view as the arithmetic sees them
struct TrackFrame {
    RegSource src;
    int W, H;
};
struct TrackModel {
    int W, H;
    float focal, cx, cy;
    float R[9], t[3];
};
struct TrackGate {
    int stride;
    float max_dist, max_dist2, min_cos, z_far; // max_dist2 = max_dist * max_dist, one multiply on the host
};
struct TrackPose {
    float R[9], t[3];
};

// why a set of parameters is refused, or null (the entry points, the serial programs)
inline const char* track_params_refusal(const adc_track_params& p)
{
    if (p.iterations < 1u || p.iterations > ADC_TRACK_MAX_ITERATIONS_LIMIT) return "iterations must lie in [1, 32]";
    if (p.stride < 1u || p.stride > 16u) return "stride must lie in [1, 16]";
    if (!(__builtin_isfinite(p.max_dist) && p.max_dist > 0.0f)) return "max_dist must be finite and > 0";
    if (!(p.min_cos >= -1.0f && p.min_cos <= 1.0f)) return "min_cos must lie in [-1, 1]";
    if (!(__builtin_isfinite(p.z_far) && p.z_far > 0.0f)) return "z_far must be finite and > 0";
    if (p.min_pixels < 6u) return "min_pixels must be at least 6";
    if (!(p.eps_rot >= 0.0f && p.eps_trans >= 0.0f)) return "eps_rot, eps_trans must be >= 0 (no NaN)";
    if (!(__builtin_isfinite(p.max_rot) && p.max_rot > 0.0f && __builtin_isfinite(p.max_trans) && p.max_trans > 0.0f)) return "max_rot, max_trans must be finite and > 0";
    if (!(p.damping >= 0.0f && __builtin_isfinite(p.damping))) return "damping must be finite and >= 0";
    if (!(p.pivot_ratio >= 0.0f && p.pivot_ratio < 1.0f)) return "pivot_ratio must lie in [0, 1)";
    if (p.flags != 0u) return "unknown flag";
    if (p.reserved_[0] | p.reserved_[1] | p.reserved_[2]) return "a reserved word is not 0";
    return nullptr;
}

// the fields of the model view the tracker reads
inline const char* track_model_refusal(const adc_tsdf_raycast_params& m)
{
    if (m.width < 1 || m.height < 1 || m.width > TRACK_MAX_DIM || m.height > TRACK_MAX_DIM) return "the model view's width, height must lie in [1, 8192]";
    if (!(__builtin_isfinite(m.focal_px) && m.focal_px > 0.0f)) return "the model view's focal_px must be finite and > 0";
    if (!(__builtin_isfinite(m.cx) && __builtin_isfinite(m.cy))) return "the model view's cx, cy must be finite";
    for (int i = 0; i < 9; i++)
        if (!__builtin_isfinite(m.R[i])) return "the model view's R has a non-finite entry";
    for (int i = 0; i < 3; i++)
        if (!__builtin_isfinite(m.t[i])) return "the model view's t has a non-finite entry";
    return nullptr;
}

// participating pixels per row / column, and why a frame size is refused
inline uint32_t track_span(int n, uint32_t stride) { return ((uint32_t)n + stride - 1u) / stride; }
inline const char* track_size_refusal(int W, int H, uint32_t stride)
{
    if (W < 1 || H < 1) return "the frame is empty";
    if ((unsigned long long)track_span(W, stride) * (unsigned long long)track_span(H, stride) > (unsigned long long)TRACK_MAX_PIXELS)
        return "more than 2^26 participating pixels";
    return nullptr;
}

inline TrackFrame track_frame(const adc_tsdf_frame& f, int W, int H)
{
    TrackFrame c;
    c.src.kind = f.kind;
    c.src.fb = f.calib.focal_px * f.calib.baseline;
    c.src.focal = f.calib.focal_px; c.src.cx = f.calib.cx; c.src.cy = f.calib.cy; c.src.doffs = f.calib.doffs;
    c.W = W; c.H = H;
    return c;
}

inline TrackPose track_guess(const adc_tsdf_frame& f)
{
    TrackPose p;
    for (int i = 0; i < 9; i++) p.R[i] = f.R[i];
    for (int i = 0; i < 3; i++) p.t[i] = f.t[i];
    return p;
}

inline TrackModel track_model(const adc_tsdf_raycast_params& m)
{
    TrackModel c;
    c.W = m.width; c.H = m.height;
    c.focal = m.focal_px; c.cx = m.cx; c.cy = m.cy;
    for (int i = 0; i < 9; i++) c.R[i] = m.R[i];
    for (int i = 0; i < 3; i++) c.t[i] = m.t[i];
    return c;
}

inline TrackGate track_gate(const adc_track_params& p)
{
    TrackGate g;
    g.stride = (int)p.stride;
    g.max_dist = p.max_dist;
    g.max_dist2 = p.max_dist * p.max_dist;
    g.min_cos = p.min_cos;
    g.z_far = p.z_far;
    return g;
}

// transpose(R) * d and R * d, each ((a + b) + c)
ADC_HD void track_rot_t(const float R[9], const float d[3], float o[3])
{
    for (int a = 0; a < 3; a++) o[a] = ((R[a] * d[0]) + (R[3 + a] * d[1])) + (R[6 + a] * d[2]);
}
ADC_HD void track_rot(const float R[9], const float d[3], float o[3])
{
    for (int r = 0; r < 3; r++) o[r] = ((R[3 * r] * d[0]) + (R[3 * r + 1] * d[1])) + (R[3 * r + 2] * d[2]);
}

// Steps 1 to 10 for pixel (x, y) of the frame under the estimate k: what the pixel counts as; with TRACK_USED q[0..5] is the
// quantised Jacobian (rotation, then translation) and q[6] the quantised residual.  fnormals may be null.  Reads the model maps only
// behind the integer clip.
ADC_HD int track_pixel(const TrackFrame& f, const TrackModel& m, const TrackGate& g, const TrackPose& k, int x, int y, const float* map, const float* fnormals,
                       const float* mdepth, const float* mnormals, int q[7])
{
    const size_t at = (size_t)y * (size_t)f.W + (size_t)x;
    float Z;
    if (!reg_source_z(f.src, map[at], &Z)) return TRACK_NO_DEPTH;
    if (!(Z <= g.z_far)) return TRACK_NO_DEPTH;
    const float Pc[3] = {(((float)x - f.src.cx) / f.src.focal) * Z, (((float)y - f.src.cy) / f.src.focal) * Z, Z};
    const float d[3] = {Pc[0] - k.t[0], Pc[1] - k.t[1], Pc[2] - k.t[2]};
    float Pw[3], Pm[3];
    track_rot_t(k.R, d, Pw);
    track_rot(m.R, Pw, Pm);
    for (int a = 0; a < 3; a++) Pm[a] = Pm[a] + m.t[a];
    if (!(__builtin_isfinite(Pm[2]) && Pm[2] > 0.0f)) return TRACK_OUTSIDE;
    const float rz = 1.0f / Pm[2];
    const float pu = ((Pm[0] * m.focal) * rz) + m.cx;
    const float pv = ((Pm[1] * m.focal) * rz) + m.cy;
    if (!(__builtin_fabsf(pu) < 32768.0f && __builtin_fabsf(pv) < 32768.0f)) return TRACK_OUTSIDE;
    const int xm = (int)__builtin_floorf(pu + 0.5f), ym = (int)__builtin_floorf(pv + 0.5f);
    if (xm < 0 || xm >= m.W || ym < 0 || ym >= m.H) return TRACK_OUTSIDE;
    const size_t am = (size_t)ym * (size_t)m.W + (size_t)xm;
    const float Dm = mdepth[am];
    const float nm[3] = {mnormals[4 * am], mnormals[4 * am + 1], mnormals[4 * am + 2]};
    if (!(Dm > 0.0f) || !(mnormals[4 * am + 3] > 0.0f)) return TRACK_NO_MODEL; // (a NaN is no model either)
    const float Qm[3] = {(((float)xm - m.cx) / m.focal) * Dm, (((float)ym - m.cy) / m.focal) * Dm, Dm};
    const float df[3] = {Pm[0] - Qm[0], Pm[1] - Qm[1], Pm[2] - Qm[2]};
    const float d2 = ((df[0] * df[0]) + (df[1] * df[1])) + (df[2] * df[2]);
    if (!(d2 <= g.max_dist2)) return TRACK_FAR;
    if (fnormals && fnormals[4 * at + 3] > 0.0f) {
        const float nf[3] = {fnormals[4 * at], fnormals[4 * at + 1], fnormals[4 * at + 2]};
        float nw[3], nr[3];
        track_rot_t(k.R, nf, nw);
        track_rot(m.R, nw, nr);
        const float dot = ((nr[0] * nm[0]) + (nr[1] * nm[1])) + (nr[2] * nm[2]);
        if (!(dot >= g.min_cos)) return TRACK_ANGLE;
    }
    const float r = ((nm[0] * df[0]) + (nm[1] * df[1])) + (nm[2] * df[2]);
    const float c[3] = {(Pm[1] * nm[2]) - (Pm[2] * nm[1]), (Pm[2] * nm[0]) - (Pm[0] * nm[2]), (Pm[0] * nm[1]) - (Pm[1] * nm[0])};
    const float s[7] = {c[0] / g.z_far, c[1] / g.z_far, c[2] / g.z_far, nm[0], nm[1], nm[2], r / g.max_dist};
    bool in = true;
    for (int i = 0; i < 7; i++) in = in && __builtin_fabsf(s[i]) < TRACK_RANGE; // (a NaN fails)
    if (!in) return TRACK_OUT_OF_RANGE;
    for (int i = 0; i < 7; i++) q[i] = (int)__builtin_rintf(s[i] * TRACK_Q);
    return TRACK_USED;
}

// step 11: a used pixel's 28 products, added to S
ADC_HD void track_accumulate(const int q[7], long long S[TRACK_SUMS])
{
    int n = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) S[n++] += (long long)q[i] * (long long)q[j];
    for (int i = 0; i < 6; i++) S[21 + i] += (long long)q[i] * (long long)q[6];
    S[27] += (long long)q[6] * (long long)q[6];
}

// the participating pixel number p in [0, span(W) * span(H))
ADC_HD void track_pixel_of(const TrackFrame& f, const TrackGate& g, uint32_t p, int* x, int* y)
{
    const uint32_t pw = ((uint32_t)f.W + (uint32_t)g.stride - 1u) / (uint32_t)g.stride;
    *x = (int)(p % pw) * g.stride;
    *y = (int)(p / pw) * g.stride;
}

// ------------------------------------------------------------------------------------------------ the solve (binary64)
// rigid transforms as (R, t) in doubles: (R1, t1) * (R2, t2) = (R1 R2, R1 t2 + t1), every entry ((a + b) + c) [+ t]
struct TrackRigid {
    double R[9], t[3];
};

ADC_HD void track_mat3(const double A[9], const double B[9], double C[9])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = ((A[3 * i] * B[j]) + (A[3 * i + 1] * B[3 + j])) + (A[3 * i + 2] * B[6 + j]);
}

ADC_HD TrackRigid track_compose(const TrackRigid& a, const TrackRigid& b)
{
    TrackRigid c;
    track_mat3(a.R, b.R, c.R);
    for (int i = 0; i < 3; i++) c.t[i] = (((a.R[3 * i] * b.t[0]) + (a.R[3 * i + 1] * b.t[1])) + (a.R[3 * i + 2] * b.t[2])) + a.t[i];
    return c;
}

// the inverse by transposition: (R^T, -(R^T t))
ADC_HD TrackRigid track_inverse(const TrackRigid& a)
{
    TrackRigid c;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) c.R[3 * i + j] = a.R[3 * j + i];
    for (int i = 0; i < 3; i++) c.t[i] = -(((c.R[3 * i] * a.t[0]) + (c.R[3 * i + 1] * a.t[1])) + (c.R[3 * i + 2] * a.t[2]));
    return c;
}

ADC_HD bool track_finite(double v) { return v - v == 0.0; }

// One solve: the sums and counts of reduce pass `iter` under the pose `cur` -> the record of that iteration, H, b and the counts of
// `res`, and with a step accepted the next pose.  Returns true when the status is terminal (res->status is then final); otherwise
// res->status stays ADC_TRACK_MAX_ITERATIONS, which is what it is when no later solve runs.  res->R, res->t always hold the last
// accepted pose.
ADC_HD bool track_solve(const long long S[TRACK_SUMS], const uint32_t cnt[TRACK_COUNTS], uint32_t pixels, const adc_track_params& p, const TrackModel& m,
                        const TrackPose& cur, uint32_t iter, adc_track_result* res)
{
    const uint32_t used = cnt[TRACK_USED];
    res->solves = iter + 1u;
    res->status = ADC_TRACK_MAX_ITERATIONS;
    res->pixels = pixels;
    res->no_depth = cnt[TRACK_NO_DEPTH]; res->outside = cnt[TRACK_OUTSIDE]; res->no_model = cnt[TRACK_NO_MODEL]; res->too_far =cnt[TRACK_FAR];
    res->angle = cnt[TRACK_ANGLE]; res->out_of_range = cnt[TRACK_OUT_OF_RANGE]; res->used = used;
    for (int i = 0; i < 9; i++) res->R[i] = cur.R[i];
    for (int i = 0; i < 3; i++) res->t[i] = cur.t[i];
    // undo the three scales (each a power of two times z_far or max_dist: exact unless the sum itself had to be rounded)
    const double inv_q = 1.0 / 65536.0, zs = (double)p.z_far * inv_q, rs = (double)p.max_dist * inv_q;
    double sc[6] = {zs, zs, zs, inv_q, inv_q, inv_q};
    double H[36], b[6];
    int n = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) {
            const double v = ((double)S[n++] * sc[i]) * sc[j];
            H[6 * i + j] = v;
            H[6 * j + i] = v;
        }
    for (int i = 0; i < 6; i++) b[i] = ((double)S[21 + i] * sc[i]) * rs;
    for (int i = 0; i < 36; i++) res->H[i] = H[i];
    for (int i = 0; i < 6; i++) res->b[i] = b[i];
    adc_track_iteration* it = &res->iteration[iter];
    it->used = used;
    it->rms = used ? (float)__builtin_sqrt((((double)S[27] * rs) * rs) / (double)used) : 0.0f;
    it->rot = 0.0f;
    it->trans = 0.0f;
    if (used < p.min_pixels) { res->status = ADC_TRACK_LOST; return true; }
    // H = L D L^T without pivoting, on the damped diagonal
    const double damping = (double)p.damping, ratio = (double)p.pivot_ratio;
    double L[36], D[6], diag[6];
    for (int i = 0; i < 6; i++) diag[i] = H[7 * i] + (damping * H[7 * i]);
    for (int j = 0; j < 6; j++) {
        double dj = diag[j];
        for (int c = 0; c < j; c++) dj = dj - ((L[6 * j + c] * L[6 * j + c]) * D[c]);
        if (!(track_finite(dj) && dj > ratio * diag[j])) { res->status = ADC_TRACK_DEGENERATE; return true; }
        D[j] = dj;
        for (int i = j + 1; i < 6; i++) {
            double v = H[6 * i + j];
            for (int c = 0; c < j; c++) v = v - ((L[6 * i + c] * L[6 * j + c]) * D[c]);
            L[6 * i + j] = v / dj;
        }
    }
    // H xi = -b: L y = -b, z = y / D, L^T xi = z
    double xi[6];
    for (int i = 0; i < 6; i++) {
        double v = -b[i];
        for (int c = 0; c < i; c++) v = v - (L[6 * i + c] * xi[c]);
        xi[i] = v;
    }
    for (int i = 0; i < 6; i++) xi[i] = xi[i] / D[i];
    for (int i = 5; i >= 0; i--) {
        double v = xi[i];
        for (int c = i + 1; c < 6; c++) v = v - (L[6 * c + i] * xi[c]);
        xi[i] = v;
    }
    const double w2 = ((xi[0] * xi[0]) + (xi[1] * xi[1])) + (xi[2] * xi[2]);
    const double v2 = ((xi[3] * xi[3]) + (xi[4] * xi[4])) + (xi[5] * xi[5]);
    it->rot = (float)__builtin_sqrt(w2);
    it->trans = (float)__builtin_sqrt(v2);
    if (!(w2 <= (double)p.max_rot * (double)p.max_rot) || !(v2 <= (double)p.max_trans * (double)p.max_trans)) { res->status = ADC_TRACK_DIVERGED; return true; } // (a NaN diverges)
    // the update's rotation: the Cayley map of a = omega / 2
    const double a[3] = {xi[0] * 0.5, xi[1] * 0.5, xi[2] * 0.5};
    const double aa = ((a[0] * a[0]) + (a[1] * a[1])) + (a[2] * a[2]);
    const double den = 1.0 + aa, one = 1.0 - aa;
    const double X[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
    TrackRigid dT, Tk, Tm;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) dT.R[3 * i + j] = (((i == j ? one : 0.0) + (2.0 * (a[i] * a[j]))) + (2.0 * X[3 * i + j])) / den;
    for (int i = 0; i < 3; i++) dT.t[i] = xi[3 + i];
    for (int i = 0; i < 9; i++) { Tk.R[i] = (double)cur.R[i]; Tm.R[i] = (double)m.R[i]; }
    for (int i = 0; i < 3; i++) { Tk.t[i] = (double)cur.t[i]; Tm.t[i] = (double)m.t[i]; }
    // Tk <- Tk * Tm^-1 * dT^-1 * Tm, from the left
    const TrackRigid T3 = track_compose(track_compose(track_compose(Tk, track_inverse(Tm)), track_inverse(dT)), Tm);
    // one square-root-free step towards an orthonormal R: R <- R (3 I - R^T R) / 2
    double Rt[9], G[9], B[9], Rn[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rt[3 * i + j] = T3.R[3 * j + i];
    track_mat3(Rt, T3.R, G);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) B[3 * i + j] = ((i == j ? 3.0 : 0.0) - G[3 * i + j]) * 0.5;
    track_mat3(T3.R, B, Rn);
    for (int i = 0; i < 9; i++) res->R[i] = (float)Rn[i];
    for (int i = 0; i < 3; i++) res->t[i] = (float)T3.t[i];
    if (w2 < (double)p.eps_rot * (double)p.eps_rot && v2 < (double)p.eps_trans * (double)p.eps_trans) { res->status = ADC_TRACK_CONVERGED; return true; }
    return false;
}
