// tsdf_cell.h -- the per-cell rule of the TSDF volume's triangle mesh (k_tsdf.hip: k_tsdf_mesh_*; include/adcensus_c_api.h holds the
// definition in words, tests/tsdf_mesh_ref.py in numpy).  Plain inline functions on top of tsdf_voxel.h, shared by the kernels and by
// g++-compiled serial programs (tests/emul/emul_tsdf_mesh.cpp, tests/sanitize/stub_capi_tsdf_mesh.cpp): no HIP header, no handle.
// Everything here is an integer comparison: a triangle is three vertex numbers, and a vertex number is a prefix count of crossings.
#pragma once
#include "tsdf_voxel.h"
#include "tsdf_mc_table.h" // GENERATED: TSDF_MC_TABLE, TSDF_MC_ROW, TSDF_MC_MAX_TRIS (tools/gen_tsdf_mc_table.py)

// why a volume's mesh is refused, or null: the counts are 32-bit, and M triangles per cell must fit them
inline const char* tsdf_mesh_refusal(const adc_tsdf_params& p)
{
    const unsigned long long cells = (unsigned long long)(p.nx - 1) * (unsigned long long)(p.ny - 1) * (unsigned long long)(p.nz - 1);
    if ((unsigned long long)TSDF_MC_MAX_TRIS * cells > 0xFFFFFFFFull) return "the volume has too many cells for 32-bit triangle counts (M * (nx-1)(ny-1)(nz-1) must not exceed 2^32 - 1)";
    return nullptr;
}

// cell (i, j, k) exists: all eight corners lie inside the volume
ADC_HD bool tsdf_cell_exists(const TsdfVol& v, int i, int j, int k) { return i + 1 < v.nx && j + 1 < v.ny && k + 1 < v.nz; }

// the eight corner words w[c], corner c = (i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)): all seen; the case index (bit c set
// iff t_c < 0 by tsdf_word_t: a stored -32768 reads as -32767, t = 0 counts as positive, as in tsdf_crossing)
ADC_HD bool tsdf_cell_seen(const uint32_t w[8], uint32_t min_weight)
{
    bool seen = true;
    for (int c = 0; c < 8; c++) seen = seen && tsdf_seen(w[c], min_weight);
    return seen;
}

ADC_HD uint32_t tsdf_cell_case(const uint32_t w[8])
{
    uint32_t index = 0;
    for (int c = 0; c < 8; c++) index |= tsdf_word_t(w[c]) < 0 ? 1u << c : 0u;
    return index;
}

// cell edge e = 4 * axis + m: the offset of its owner corner in the cell; returns the axis.  The edge runs from the owner to the
// owner's +axis neighbour and its vertex is the crossing (owner voxel, axis).
ADC_HD int tsdf_edge_owner(uint32_t e, int* di, int* dj, int* dk)
{
    const int axis = (int)(e >> 2), a = (int)(e & 1u), b = (int)((e >> 1) & 1u);
    *di = axis == 0 ? 0 : a;
    *dj = axis == 0 ? a : axis == 1 ? 0 : b;
    *dk = axis == 2 ? 0 : b;
    return axis;
}

// The vertex number of the crossing (voxel n = (i, j, k), axis): `first` is the rank of the voxel's first crossing in the full vertex
// list; x, y, z follow in that order, so the crossings of the voxel on the axes in front of `axis` are counted from the volume's words.
ADC_HD uint32_t tsdf_vertex_number(const TsdfVol& v, const uint32_t* tsdf, uint32_t min_weight, uint32_t first, size_t n, int i, int j, int axis)
{
    uint32_t rank = first;
    const uint32_t word = tsdf[n];
    if (axis > 0 && i + 1 < v.nx && tsdf_crossing(word, tsdf[n + 1], min_weight)) rank++;
    if (axis > 1 && j + 1 < v.ny && tsdf_crossing(word, tsdf[n + (size_t)v.nx], min_weight)) rank++;
    return rank;
}
