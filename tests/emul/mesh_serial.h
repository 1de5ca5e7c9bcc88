// mesh_serial.h -- adcensus_amd/csrc/mesh_cell.h walked serially over a whole map, one cell at a time: the mesh of
// include/adcensus_c_api.h (adc_mesh) on the host, for tests/emul/emul_mesh.cpp and tests/sanitize/stub_capi_mesh.cpp.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../../adcensus_amd/csrc/mesh_cell.h"

// bgr may be null (colours 0), calib may be null (no calibration); the outputs hold ALL records
inline void mesh_serial(const float* disp, const uint8_t* bgr, int W, int H, const adc_calib* calib, float max_diff, int step, std::vector<adc_point>& vertices,
                        std::vector<int32_t>& vertex_index, std::vector<uint32_t>& triangles, adc_mesh_report* rep)
{
    const MeshCam cam = mesh_cam(calib);
    const int Wl = mesh_lattice(W, step), Hl = mesh_lattice(H, step);
    const size_t Nl = (size_t)Wl * (size_t)Hl;
    std::vector<float> a(Nl);
    std::vector<unsigned char> valid(Nl), used(Nl, 0), code(Nl, 0);
    memset(rep, 0, sizeof(*rep));
    for (int j = 0; j < Hl; j++)
        for (int i = 0; i < Wl; i++) {
            const size_t L = (size_t)j * Wl + i;
            a[L] = fabsf(disp[(size_t)(j * step) * W + (size_t)(i * step)]);
            valid[L] = mesh_valid(cam, a[L]) ? 1 : 0;
            rep->lattice_valid += valid[L];
        }
    for (int j = 0; j + 1 < Hl; j++)
        for (int i = 0; i + 1 < Wl; i++) {
            const size_t L = (size_t)j * Wl + i;
            const size_t at[4] = {L, L + 1, L + Wl, L + Wl + 1};
            const float ca[4] = {a[at[0]], a[at[1]], a[at[2]], a[at[3]]};
            const bool cv[4] = {valid[at[0]] != 0, valid[at[1]] != 0, valid[at[2]] != 0, valid[at[3]] != 0};
            const uint32_t c = mesh_cell_code(ca, cv, max_diff);
            code[L] = (unsigned char)c;
            for (int k = 0; k < 4; k++)
                if (mesh_code_uses(c, k)) used[at[k]] = 1;
            const uint32_t n = mesh_code_triangles(c);
            rep->cells_two += n == 2;
            rep->cells_one += n == 1;
        }
    std::vector<uint32_t> number(Nl, 0);
    vertices.clear();
    vertex_index.clear();
    triangles.clear();
    for (int j = 0; j < Hl; j++)
        for (int i = 0; i < Wl; i++) {
            const size_t L = (size_t)j * Wl + i;
            if (!used[L]) continue;
            number[L] = (uint32_t)vertices.size();
            const int x = i * step, y = j * step;
            const size_t pixel = (size_t)y * W + x;
            float p[3];
            mesh_point(cam, x, y, a[L], p);
            const uint32_t colour = mesh_colour(bgr, pixel);
            adc_point pt;
            memset(&pt, 0, sizeof(pt));
            memcpy(&pt, p, 12);
            memcpy(reinterpret_cast<unsigned char*>(&pt) + 12, &colour, 4); // (r, g, b, pad in memory order: little endian)
            vertices.push_back(pt);
            vertex_index.push_back((int32_t)pixel);
        }
    for (size_t L = 0; L < Nl; L++)
        for (int t = 0; t < 2; t++) {
            if (!(code[L] & (1u << t))) continue;
            int corner[3];
            mesh_triangle_corners(code[L], t, corner);
            for (int k = 0; k < 3; k++) triangles.push_back(number[L + (size_t)(corner[k] & 1) + (size_t)(corner[k] >> 1) * Wl]);
        }
    rep->vertices = (uint32_t)vertices.size();
    rep->triangles = (uint32_t)(triangles.size() / 3);
}
