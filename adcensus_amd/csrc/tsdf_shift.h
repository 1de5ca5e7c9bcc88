// tsdf_shift.h -- the rule of the moving TSDF volume (k_tsdf_shift.hip; include/adcensus_c_api.h holds the definition in words,
// tests/tsdf_shift_ref.py in numpy).  Plain inline functions shared by the kernels, the entry points and a g++-compiled serial program
// (tests/emul/emul_tsdf_shift.cpp): no HIP header, no handle.  The voxel rule (tsdf_voxel.h) is untouched: a shift moves voxel WORDS
// by whole voxels and moves the origin along, so every consumer of tsdf_params.origin sees the same surface in the same place.
//
// Everything that decides what a voxel does is an integer comparison; no test forms coordinate + shift (a shift may be any int32):
// the comparisons are written on the shift alone.  The only float arithmetic is the origin (binary32, one multiply and one add from
// the TOTAL offset, nothing fused, nothing accumulated) and the follow rule (binary64, in the order written).
#pragma once
#include "tsdf_voxel.h"

#define TSDF_SHIFT_MAX_OFFSET (1 << 24) // |offset| up to here converts to binary32 exactly
#define TSDF_FOLLOW_MAX_SHIFT (1 << 30) // the follow rule's result is clipped to this magnitude (it would be refused long before)

// one shift, and the box it acts on
struct TsdfShiftRule {
    int sx, sy, sz;
    int nx, ny, nz;
};

inline TsdfShiftRule tsdf_shift_rule(const adc_tsdf_params& p, const int32_t s[3])
{
    TsdfShiftRule r;
    r.sx = s[0]; r.sy = s[1]; r.sz = s[2];
    r.nx = p.nx; r.ny = p.ny; r.nz = p.nz;
    return r;
}

// c + s lies in [0, n), for c in [0, n) and any s
ADC_HD bool tsdf_shift_in(int c, int s, int n) { return s >= -c && s < n - c; }
// c - s lies outside [0, n): the voxel at c leaves on this axis
ADC_HD bool tsdf_shift_out(int c, int s, int n) { return s > c || s <= c - n; }

// new voxel (i, j, k) takes the words of old voxel (i + sx, j + sy, k + sz) iff that lies inside the box; otherwise it is empty
ADC_HD bool tsdf_shift_row_has_source(const TsdfShiftRule& r, int j, int k) { return tsdf_shift_in(j, r.sy, r.ny) && tsdf_shift_in(k, r.sz, r.nz); }
ADC_HD bool tsdf_shift_has_source(const TsdfShiftRule& r, int i, int j, int k) { return tsdf_shift_in(i, r.sx, r.nx) && tsdf_shift_row_has_source(r, j, k); }

// old voxel (i, j, k) leaves iff (i - sx, j - sy, k - sz) lies outside the box
ADC_HD bool tsdf_shift_row_leaves(const TsdfShiftRule& r, int j, int k) { return tsdf_shift_out(j, r.sy, r.ny) || tsdf_shift_out(k, r.sz, r.nz); }
ADC_HD bool tsdf_shift_leaves(const TsdfShiftRule& r, int i, int j, int k) { return tsdf_shift_out(i, r.sx, r.nx) || tsdf_shift_row_leaves(r, j, k); }

// the voxel at c, or its neighbour at c + 1 if the box has one, leaves on this axis
ADC_HD bool tsdf_shift_near_out(int c, int s, int n) { return tsdf_shift_out(c, s, n) || (c + 1 < n && tsdf_shift_out(c + 1, s, n)); }

// The edges of old voxel a = (i, j, k) towards its +x, +y, +z neighbours (bit 0, 1, 2) of which an endpoint leaves: the crossings of
// the extraction with this mask are the leaving list.  The neighbour differs from a on one axis only.
ADC_HD uint32_t tsdf_shift_edge_mask(const TsdfShiftRule& r, int i, int j, int k)
{
    const bool ox = tsdf_shift_out(i, r.sx, r.nx), oy = tsdf_shift_out(j, r.sy, r.ny), oz = tsdf_shift_out(k, r.sz, r.nz);
    if (ox || oy || oz) return 7u;
    return (tsdf_shift_near_out(i, r.sx, r.nx) ? 1u : 0u) | (tsdf_shift_near_out(j, r.sy, r.ny) ? 2u : 0u) | (tsdf_shift_near_out(k, r.sz, r.nz) ? 4u : 0u);
}

// some c of [lo, hi] (0 <= lo <= hi < n) leaves or has a leaving + 1 neighbour on this axis.  s > 0: the voxels c < s leave (c + 1 < s
// implies it); s < 0: the voxels c >= n + s leave, so c >= n + s - 1 is near.
ADC_HD bool tsdf_shift_range_near_out(int lo, int hi, int s, int n)
{
    if (s > 0) return s > lo;
    if (s < 0) return s <= hi + 1 - n;
    return false;
}

// A run of consecutive voxels n0 .. n1 (linear indices of one tile, n1 inside the volume) MAY hold an edge of the leaving list.  Exact
// per axis on the coordinate range the run spans; a run that crosses a row (a layer) spans every x (every y).  Never false for a run
// that holds one: the lanes apply tsdf_shift_edge_mask behind it.  Uniform in a wave, integers only, in front of every load.
ADC_HD bool tsdf_shift_tile_relevant(const TsdfShiftRule& r, int n0, int n1)
{
    const int row0 = n0 / r.nx, row1 = n1 / r.nx;
    const int k0 = row0 / r.ny, k1 = row1 / r.ny;
    if (tsdf_shift_range_near_out(k0, k1, r.sz, r.nz)) return true;
    const bool one_layer = k0 == k1, one_row = row0 == row1;
    const int j0 = one_layer ? row0 - k0 * r.ny : 0, j1 = one_layer ? row1 - k1 * r.ny : r.ny - 1;
    if (tsdf_shift_range_near_out(j0, j1, r.sy, r.ny)) return true;
    const int i0 = one_row ? n0 - row0 * r.nx : 0, i1 = one_row ? n1 - row1 * r.nx : r.nx - 1;
    return tsdf_shift_range_near_out(i0, i1, r.sx, r.nx);
}

// everything leaves: the shift kernel is not needed (two memsets), and n + delta need not fit anything
inline bool tsdf_shift_all_leave(const TsdfShiftRule& r)
{
    return r.sx >= r.nx || r.sx <= -r.nx || r.sy >= r.ny || r.sy <= -r.ny || r.sz >= r.nz || r.sz <= -r.nz;
}

inline bool tsdf_shift_is_zero(const int32_t s[3]) { return s[0] == 0 && s[1] == 0 && s[2] == 0; }

// why a shift is refused, or null (the entry points, the serial program)
inline const char* tsdf_shift_params_refusal(const adc_tsdf_shift_params& p)
{
    if (p.min_weight < 1u || p.min_weight > 65535u) return "min_weight must lie in [1, 65535]";
    if (p.flags != 0u) return "unknown flag";
    if (p.reserved_[0] | p.reserved_[1] | p.reserved_[2]) return "a reserved word is not 0";
    return nullptr;
}

// the offset after the shift, or a refusal: |offset| stays <= 2^24 on every axis (64-bit sum: no int32 overflow on the way)
inline const char* tsdf_shift_offset_refusal(const int32_t offset[3], const int32_t s[3], int32_t out[3])
{
    for (int a = 0; a < 3; a++) {
        const long long v = (long long)offset[a] + (long long)s[a];
        if (v > (long long)TSDF_SHIFT_MAX_OFFSET || v < -(long long)TSDF_SHIFT_MAX_OFFSET) return "the total offset would pass 2^24 voxels";
        out[a] = (int32_t)v;
    }
    return nullptr;
}

// the origin of the window from the origin at creation and the TOTAL offset: one conversion (exact), one multiply, one add
inline float tsdf_shift_origin(float origin0, int32_t offset, float voxel)
{
    const float step = (float)offset * voxel;
    return origin0 + step;
}

// why a follow request is refused, or null
inline const char* tsdf_follow_params_refusal(const adc_tsdf_follow_params& f)
{
    if (!(__builtin_isfinite(f.anchor[0]) && __builtin_isfinite(f.anchor[1]) && __builtin_isfinite(f.anchor[2]))) return "anchor must be finite";
    if (f.margin < 0) return "margin must be >= 0";
    if (f.quantum < 1) return "quantum must be >= 1";
    if (f.reserved_[0] | f.reserved_[1] | f.reserved_[2]) return "a reserved word is not 0";
    return nullptr;
}

// The follow rule: how far to shift so that the camera-frame point `anchor` of the pose (R, t: world -> camera) stays near the
// volume's centre.  binary64, every expression in the order written.
//   d = anchor - t;  A[a] = (R[0][a] * d[0] + R[1][a] * d[1]) + R[2][a] * d[2]        (A = transpose(R) * d)
//   p = (A[a] - origin[a]) / voxel - n_a / 2;   shift[a] = quantum * trunc(p / quantum) if |p| > margin, else 0 (a NaN: 0)
// clipped to +-TSDF_FOLLOW_MAX_SHIFT.
inline void tsdf_follow_plan(const adc_tsdf_params& p, const float R[9], const float t[3], const adc_tsdf_follow_params& f, int32_t shift[3])
{
    const double d[3] = {(double)f.anchor[0] - (double)t[0], (double)f.anchor[1] - (double)t[1], (double)f.anchor[2] - (double)t[2]};
    const int n[3] = {p.nx, p.ny, p.nz};
    for (int a = 0; a < 3; a++) {
        const double A = ((double)R[a] * d[0] + (double)R[3 + a] * d[1]) + (double)R[6 + a] * d[2];
        const double c = (A - (double)p.origin[a]) / (double)p.voxel - (double)n[a] / 2.0;
        double v = 0.0;
        if (__builtin_fabs(c) > (double)f.margin) v = (double)f.quantum * __builtin_trunc(c / (double)f.quantum);
        if (v > (double)TSDF_FOLLOW_MAX_SHIFT) v = (double)TSDF_FOLLOW_MAX_SHIFT;
        if (v < -(double)TSDF_FOLLOW_MAX_SHIFT) v = -(double)TSDF_FOLLOW_MAX_SHIFT;
        shift[a] = (int32_t)v;
    }
}
