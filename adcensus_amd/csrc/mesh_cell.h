// mesh_cell.h -- the cell rule of the triangle mesh from a disparity map (k_mesh.hip; include/adcensus_c_api.h holds the definition
// in words, tests/mesh_ref.py in numpy).  Plain inline functions shared by the kernels and by g++-compiled serial programs
// (tests/emul/emul_mesh.cpp, tests/sanitize/stub_capi_mesh.cpp): no HIP header, no handle.
//
// Everything that decides the mesh is a comparison of binary32 values, each the result of one subtraction and one fabsf; the vertex
// record is the point arithmetic of the cloud (k_outputs.hip: k_out_emit), one rounding per operation, nothing fused (the pragma of
// adc_device_fn.h; the .hip files are compiled with -ffp-contract=off as well).  Nothing here depends on an order of evaluation.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/adcensus_c_api.h"
#include "adc_device_fn.h"

// what the arithmetic takes from the calibration (calibrated = 0: none was given, the other fields are unused)
struct MeshCam {
    int calibrated;
    float fb, focal, cx, cy, doffs;
};

// A cell code: bit 0 = T0 is emitted, bit 1 = T1 is emitted, bit 2 = the diagonal is BC (0: AD).  0 = nothing is emitted.
#define MESH_T0 1u
#define MESH_T1 2u
#define MESH_BC 4u
// corners of a cell: A = (i, j), B = (i+1, j), C = (i, j+1), D = (i+1, j+1); corner k sits at lattice offset (k & 1, k >> 1)
enum { MESH_A = 0, MESH_B = 1, MESH_C = 2, MESH_D = 3 };

ADC_HD MeshCam mesh_cam(const adc_calib* c)
{
    MeshCam m = {0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (c) {
        m.calibrated = 1;
        m.fb = c->focal_px * c->baseline;
        m.focal = c->focal_px; m.cx = c->cx; m.cy = c->cy; m.doffs = c->doffs;
    }
    return m;
}

// lattice columns / rows of an image side of n pixels
ADC_HD int mesh_lattice(int n, int step) { return (n - 1) / step + 1; }

// validity of a lattice pixel, a = fabsf(d): that of the cloud (k_outputs.hip: out_cloud_valid)
ADC_HD bool mesh_valid(const MeshCam& c, float a)
{
    if (!c.calibrated) return a != ADC_INVALID_FLOAT;
    return __builtin_isfinite(a) && a + c.doffs > 0.0f;
}

// the gate of an edge between two VALID lattice pixels: one subtraction; a NaN fails
ADC_HD bool mesh_near(float ap, float aq, float max_diff) { return __builtin_fabsf(ap - aq) <= max_diff; }

// The code of one cell from the values a[] and validities v[] of its corners A, B, C, D.
// Four valid corners: the diagonal is AD iff |aA - aD| <= |aB - aC| (a tie: AD; a NaN: BC).  Three: the diagonal that does not touch the
// missing corner (D or A missing: BC; B or C missing: AD) -- the candidate that would need the missing corner fails on its edges, so the
// other one is the definition's single candidate.  Fewer: every candidate has an invalid corner.
// AD: T0 = (A, C, D), T1 = (A, D, B).  BC: T0 = (A, C, B), T1 = (B, C, D).  A candidate is emitted iff its three edges are joined.
ADC_HD uint32_t mesh_cell_code(const float a[4], const bool v[4], float max_diff)
{
    const bool jab = v[MESH_A] && v[MESH_B] && mesh_near(a[MESH_A], a[MESH_B], max_diff);
    const bool jac = v[MESH_A] && v[MESH_C] && mesh_near(a[MESH_A], a[MESH_C], max_diff);
    const bool jbd = v[MESH_B] && v[MESH_D] && mesh_near(a[MESH_B], a[MESH_D], max_diff);
    const bool jcd = v[MESH_C] && v[MESH_D] && mesh_near(a[MESH_C], a[MESH_D], max_diff);
    bool bc;
    if (v[MESH_A] && v[MESH_B] && v[MESH_C] && v[MESH_D])
        bc = !(__builtin_fabsf(a[MESH_A] - a[MESH_D]) <= __builtin_fabsf(a[MESH_B] - a[MESH_C]));
    else
        bc = !v[MESH_A] || !v[MESH_D];
    uint32_t code = 0;
    if (bc) {
        const bool jbc = v[MESH_B] && v[MESH_C] && mesh_near(a[MESH_B], a[MESH_C], max_diff);
        if (jac && jbc && jab) code |= MESH_T0;
        if (jbc && jcd && jbd) code |= MESH_T1;
    } else {
        const bool jad = v[MESH_A] && v[MESH_D] && mesh_near(a[MESH_A], a[MESH_D], max_diff);
        if (jac && jcd && jad) code |= MESH_T0;
        if (jad && jbd && jab) code |= MESH_T1;
    }
    return code ? code | (bc ? MESH_BC : 0u) : 0u;
}

// the three corners (MESH_A .. MESH_D) of triangle t (0 or 1) of a cell with this code, in the winding of the definition
ADC_HD void mesh_triangle_corners(uint32_t code, int t, int corner[3])
{
    if (code & MESH_BC) {
        if (t == 0) { corner[0] = MESH_A; corner[1] = MESH_C; corner[2] = MESH_B; }
        else        { corner[0] = MESH_B; corner[1] = MESH_C; corner[2] = MESH_D; }
    } else {
        if (t == 0) { corner[0] = MESH_A; corner[1] = MESH_C; corner[2] = MESH_D; }
        else        { corner[0] = MESH_A; corner[1] = MESH_D; corner[2] = MESH_B; }
    }
}

// does a cell with this code emit a triangle that has this corner?  (bit k of the masks: corner k)
ADC_HD bool mesh_code_uses(uint32_t code, int corner)
{
    const uint32_t t0 = (code & MESH_BC) ? 0x7u /* A C B */ : 0xDu /* A C D */;
    const uint32_t t1 = (code & MESH_BC) ? 0xEu /* B C D */ : 0xBu /* A D B */;
    const uint32_t m = ((code & MESH_T0) ? t0 : 0u) | ((code & MESH_T1) ? t1 : 0u);
    return (m >> corner) & 1u;
}

// number of triangles of a code
ADC_HD uint32_t mesh_code_triangles(uint32_t code) { return (code & 1u) + ((code >> 1) & 1u); }

// position of a valid pixel (x, y) with a = fabsf(d): the point of the cloud (k_outputs.hip: k_out_emit)
ADC_HD void mesh_point(const MeshCam& c, int x, int y, float a, float p[3])
{
    float px = (float)x, py = (float)y, pz = a;
    if (c.calibrated) {
        const float s = a + c.doffs;
        pz = c.fb / s;
        px = ((px - c.cx) * pz) / c.focal;
        py = ((py - c.cy) * pz) / c.focal;
    }
    p[0] = px; p[1] = py; p[2] = pz;
}

// the fourth word of a vertex record: r, g, b from the left image (B,G,R per pixel; null: 0), pad = 0
ADC_HD uint32_t mesh_colour(const uint8_t* bgr, size_t pixel)
{
    if (!bgr) return 0u;
    const uint8_t* c = bgr + pixel * 3;
    return (uint32_t)c[2] | ((uint32_t)c[1] << 8) | ((uint32_t)c[0] << 16);
}
