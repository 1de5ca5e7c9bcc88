// tsdf_mesh_serial.h -- adcensus_amd/csrc/tsdf_cell.h walked serially over a whole volume, one cell at a time: the triangle mesh of
// include/adcensus_c_api.h (adc_tsdf_mesh) on the host, for tests/emul/emul_tsdf_mesh.cpp and tests/sanitize/stub_capi_tsdf_mesh.cpp.
#pragma once
#include <cstring>
#include <vector>

#include "../../adcensus_amd/csrc/tsdf_cell.h"
#include "tsdf_serial.h"

// color may be null; vtx receives ALL vertex records (the points of tsdf_extract_serial), tri ALL triangle records (three vertex
// numbers each)
inline void tsdf_mesh_serial(const uint32_t* tsdf, const uint32_t* color, const adc_tsdf_params& p, uint32_t min_weight, std::vector<adc_point>& vtx,
                             std::vector<uint32_t>& tri, adc_tsdf_mesh_report* rep)
{
    const TsdfVol v = tsdf_vol(p);
    const size_t nx = (size_t)v.nx, nxy = nx * (size_t)v.ny, N = nxy * (size_t)v.nz;
    adc_tsdf_extract_report xrep;
    tsdf_extract_serial(tsdf, color, p, min_weight, vtx, &xrep);
    memset(rep, 0, sizeof(*rep));
    rep->voxels_seen = xrep.voxels_seen;
    rep->vertices = xrep.points;
    // the rank of every voxel's first crossing, as the kernels keep it (written only where a voxel owns a crossing)
    std::vector<uint32_t> first(N, 0xFFFFFFFFu);
    uint32_t rank = 0;
    for (int k = 0; k < v.nz; k++)
        for (int j = 0; j < v.ny; j++)
            for (int i = 0; i < v.nx; i++) {
                const size_t n = (size_t)k * nxy + (size_t)j * nx + (size_t)i;
                const size_t off[3] = {1, nx, nxy};
                const bool inside[3] = {i + 1 < v.nx, j + 1 < v.ny, k + 1 < v.nz};
                uint32_t own = 0;
                for (int a = 0; a < 3; a++) own += inside[a] && tsdf_crossing(tsdf[n], tsdf[n + off[a]], min_weight) ? 1u : 0u;
                if (own) first[n] = rank;
                rank += own;
            }
    tri.clear();
    for (int k = 0; k + 1 < v.nz; k++)
        for (int j = 0; j + 1 < v.ny; j++)
            for (int i = 0; i + 1 < v.nx; i++) {
                const size_t n = (size_t)k * nxy + (size_t)j * nx + (size_t)i;
                uint32_t w[8];
                for (int c = 0; c < 8; c++) w[c] = tsdf[n + (size_t)(c & 1) + (size_t)((c >> 1) & 1) * nx + (size_t)((c >> 2) & 1) * nxy];
                if (!tsdf_cell_seen(w, min_weight)) continue;
                rep->cells_seen++;
                const uint8_t* row = TSDF_MC_TABLE + tsdf_cell_case(w) * TSDF_MC_ROW;
                if (!row[0]) continue;
                rep->cells_surface++;
                for (uint32_t e = 0; e < 3u * row[0]; e++) {
                    int di, dj, dk;
                    const int axis = tsdf_edge_owner(row[1 + e], &di, &dj, &dk);
                    const size_t no = n + (size_t)di + (size_t)dj * nx + (size_t)dk * nxy;
                    tri.push_back(tsdf_vertex_number(v, tsdf, min_weight, first[no], no, i + di, j + dj, axis));
                }
                rep->triangles += row[0];
            }
}
