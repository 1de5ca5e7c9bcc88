// k_tsdf_ext.h -- what the ordered compactions of the TSDF volume share (k_tsdf.hip: the extraction and the mesh; k_tsdf_shift.hip: the
// leaving list of a shift): the launch shape, the arguments, and the crossings a lane finds for its voxel.  Device code; included by
// .hip files only.
#pragma once
#include "adc_internal.h"
#include "tsdf_voxel.h"

#define TSDF_WG 256
#define TSDF_WAVES (TSDF_WG / ADC_WAVE)
#define TSDF_ROWS_PER_WAVE 4
#define TSDF_ROW_VOXELS (ADC_WAVE * 4)               // voxels of a row one wave covers
#define TSDF_TILE 256                                // voxels per tile of the extraction
#define TSDF_TILES_PER_WAVE 4

struct TsdfExtArgs {
    TsdfVol vol;
    const uint32_t* tsdf;
    const uint32_t* color;  // may be null
    uint32_t min_weight;
    int N, ntiles, nxy;     // voxels, tiles of TSDF_TILE voxels, nx * ny
    uint32_t* rep;          // [0] voxels_seen [1] points
    uint32_t* tbase;        // per tile: crossings -> (scan) crossings of all tiles before it
    uint4* points;          // may be null
    uint32_t cap;
    uint32_t* count;        // may be null
};

// the crossings of voxel n as a mask (bit 0 x, 1 y, 2 z); word = its voxel word, nb[] the neighbour words of the set bits, (i, j, k) its place
__device__ __forceinline__ uint32_t tsdf_lane_crossings(const TsdfExtArgs& g, int n, int lane, uint32_t* word, uint32_t nb[3], int* i, int* j, int* k, bool* seen)
{
    const bool in = n < g.N;
    *word = in ? g.tsdf[n] : 0u;
    const int row = n / g.vol.nx;
    *i = n - row * g.vol.nx;
    *k = row / g.vol.ny;
    *j = row - *k * g.vol.ny;
    *seen = in && tsdf_seen(*word, g.min_weight);
    nb[0] = (uint32_t)__shfl_down((int)*word, 1, ADC_WAVE); // (every lane of the wave takes part)
    nb[1] = nb[2] = 0u;
    if (!*seen) return 0u;
    uint32_t mask = 0u;
    if (*i + 1 < g.vol.nx) { // (then n + 1 lies in the same row, inside the volume)
        if (lane == ADC_WAVE - 1) nb[0] = g.tsdf[n + 1];
        mask |= tsdf_crossing(*word, nb[0], g.min_weight) ? 1u : 0u;
    }
    if (*j + 1 < g.vol.ny) {
        nb[1] = g.tsdf[n + g.vol.nx];
        mask |= tsdf_crossing(*word, nb[1], g.min_weight) ? 2u : 0u;
    }
    if (*k + 1 < g.vol.nz) {
        nb[2] = g.tsdf[n + g.nxy];
        mask |= tsdf_crossing(*word, nb[2], g.min_weight) ? 4u : 0u;
    }
    return mask;
}
