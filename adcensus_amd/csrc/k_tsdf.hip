// k_tsdf.hip -- the TSDF volume (include/adcensus_c_api.h: adc_tsdf_integrate_device, adc_tsdf_extract_device; the voxel rule is
// tsdf_voxel.h): one frame fused into the volume, and the volume's surface points compacted in voxel order.
//
//   k_tsdf_integrate  x is the fastest axis of the volume.  A lane owns FOUR consecutive voxels of a row (nx is a multiple of 4: one
//                     16-byte group), a wave 256 voxels of a row, and walks TSDF_ROWS_PER_WAVE rows.  The projection and the update
//                     decision come FIRST: a lane loads its group of voxel words only when one of its four voxels is updated, and
//                     stores it only then (the unchanged words of the group go back with their own bits: nobody else owns them).
//                     The traffic is 8 bytes per updated voxel (16 with colour) rounded up to 16-byte groups, plus the gather from
//                     the map -- not 8 bytes per voxel of the volume.  The products with yw and zw are formed once per row.  Per
//                     workgroup one integer atomic per report count.
//   k_tsdf_measure    the volume in linear chunks of 64 voxels, a lane per voxel, four chunks = one tile of 256 voxels per wave and
//                     turn; the +x neighbour comes from the next lane (lane 63: one extra word), +y and +z from loads nx and nx * ny
//                     words away, and only for a voxel that counts as seen.  Per tile the number of crossings.
//   k_tsdf_scan       one workgroup: exclusive scan of the tile counts in place; the total -> the report and the caller's count word
//   k_tsdf_emit       the crossings again, each record behind its tile's base at the prefix two ballots of the per-lane counts
//                     (0 to 3) give.
// Every count is an integer, every rank a prefix of ballots, every voxel has one owner: no result depends on the order of the waves.
// Behind them, at the end of the file: the volume's triangle mesh (adc_tsdf_mesh_device; k_tsdf_mesh_measure, k_tsdf_mesh_emit, and
// k_tsdf_emit<true>, which also keeps every voxel's first rank).
#include "adc_internal.h"
#include "tsdf_voxel.h"
#include "tsdf_cell.h"
#include "k_tsdf_ext.h" // TSDF_WG .. TSDF_TILES_PER_WAVE, TsdfExtArgs, tsdf_lane_crossings

struct TsdfIntArgs {
    TsdfVol vol;
    TsdfCam cam;
    const float* map;
    const uint8_t* img;     // may be null
    uint32_t* tsdf;
    uint32_t* color;        // may be null
    uint32_t* rep;          // [0] in_frustum [1] no_depth [2] occluded [3] updated
    int xchunks, rows;      // 256-voxel pieces of a row; rows = ny * nz
};

__global__ __launch_bounds__(TSDF_WG) void k_tsdf_integrate(const TsdfIntArgs g)
{
    __shared__ uint32_t s_cnt[4][TSDF_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const int xc = (int)(blockIdx.x % (unsigned)g.xchunks), rb = (int)(blockIdx.x / (unsigned)g.xchunks);
    const int i0 = xc * TSDF_ROW_VOXELS + lane * 4;
    const bool in = i0 < g.vol.nx; // (nx is a multiple of 4: all four voxels or none)
    const bool with_colour = g.color != nullptr && g.img != nullptr;
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
    for (int r = 0; r < TSDF_ROWS_PER_WAVE; r++) {
        const int row = (rb * TSDF_WAVES + wave) * TSDF_ROWS_PER_WAVE + r;
        if (row >= g.rows || !in) continue;
        const int k = row / g.vol.ny, j = row - k * g.vol.ny;
        const TsdfRow rt = tsdf_row(g.vol, g.cam, j, k);
        int code[4], q[4], pixel[4];
        bool band[4], any = false, any_colour = false;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            q[e] = 0; pixel[e] = 0; band[e] = false;
            code[e] = tsdf_decide(g.vol, g.cam, rt, i0 + e, g.map, &q[e], &pixel[e], &band[e]);
            cnt[0] += code[e] != TSDF_SKIP ? 1u : 0u;
            cnt[1] += code[e] == TSDF_NO_DEPTH ? 1u : 0u;
            cnt[2] += code[e] == TSDF_OCCLUDED ? 1u : 0u;
            cnt[3] += code[e] == TSDF_UPDATE ? 1u : 0u;
            any = any || code[e] == TSDF_UPDATE;
            any_colour = any_colour || (code[e] == TSDF_UPDATE && band[e]);
        }
        if (!any) continue;
        const size_t at = (size_t)row * (size_t)g.vol.nx + (size_t)i0;
        uint4* pw = reinterpret_cast<uint4*>(g.tsdf + at);
        uint4 w4 = *pw;
        uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (code[e] == TSDF_UPDATE) w[e] = tsdf_update(w[e], q[e], g.vol.max_weight);
        w4.x = w[0]; w4.y = w[1]; w4.z = w[2]; w4.w = w[3];
        *pw = w4;
        if (with_colour && any_colour) {
            uint4* pc = reinterpret_cast<uint4*>(g.color + at);
            uint4 c4 = *pc;
            uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (code[e] == TSDF_UPDATE && band[e]) c[e] = tsdf_colour_update(c[e], g.img + (size_t)pixel[e] * 3, g.vol.max_weight);
            c4.x = c[0]; c4.y = c[1]; c4.z = c[2]; c4.w = c[3];
            *pc = c4;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        uint32_t v = cnt[c];
        for (int o = ADC_WAVE / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_down((int)v, o, ADC_WAVE);
        if (lane == 0) s_cnt[c][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t t = 0;
        for (int w = 0; w < TSDF_WAVES; w++) t += s_cnt[threadIdx.x][w];
        if (t) atomicAdd(&g.rep[threadIdx.x], t);
    }
}

__global__ __launch_bounds__(TSDF_WG) void k_tsdf_measure(const TsdfExtArgs g)
{
    __shared__ uint32_t s_seen[TSDF_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    uint32_t n_seen = 0;
#pragma unroll 1
    for (int t = 0; t < TSDF_TILES_PER_WAVE; t++) {
        const int tile = ((int)blockIdx.x * TSDF_WAVES + wave) * TSDF_TILES_PER_WAVE + t;
        if (tile >= g.ntiles) continue; // (uniform in the wave)
        uint32_t total = 0;
#pragma unroll 1
        for (int c = 0; c < TSDF_TILE / ADC_WAVE; c++) {
            const int n = tile * TSDF_TILE + c * ADC_WAVE + lane;
            uint32_t word, nb[3];
            int i, j, k;
            bool seen;
            const uint32_t mask = tsdf_lane_crossings(g, n, lane, &word, nb, &i, &j, &k, &seen);
            const uint32_t cnt = (uint32_t)__popc(mask);
            total += (uint32_t)__popcll(__ballot((cnt & 1u) != 0)) + 2u * (uint32_t)__popcll(__ballot((cnt & 2u) != 0));
            n_seen += (uint32_t)__popcll(__ballot(seen));
        }
        if (lane == 0) g.tbase[tile] = total;
    }
    if (lane == 0) s_seen[wave] = n_seen;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < TSDF_WAVES; w++) t += s_seen[w];
        if (t) atomicAdd(&g.rep[0], t);
    }
}

// One workgroup of 1024: the tile counts -> exclusive prefix sums in place, TSDF_SCAN_TILE entries at a time with a carry (the form
// of k_mesh_scan, one array); the total goes to the report word and to the caller's device word.  A lane owns four consecutive
// entries: the 524288 tiles of a 512^3 volume take 128 turns and 0.31 ms, a third of the extraction; sixteen entries per lane (32
// turns) were measured and took 0.47 ms, the lane's serial loads 64 bytes apart cost more than the barriers saved (profiles/tsdf_timing.md).
#define TSDF_SCAN_PER_LANE 4
#define TSDF_SCAN_TILE (1024 * TSDF_SCAN_PER_LANE)
__global__ __launch_bounds__(1024) void k_tsdf_scan(uint32_t* __restrict__ tbase, int ntiles, uint32_t* __restrict__ rep, uint32_t* __restrict__ count)
{
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_carry;
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int c = 0; c < ntiles; c += TSDF_SCAN_TILE) {
        const int i0 = c + (int)threadIdx.x * TSDF_SCAN_PER_LANE;
        uint32_t v[TSDF_SCAN_PER_LANE], sv = 0;
#pragma unroll
        for (int k = 0; k < TSDF_SCAN_PER_LANE; k++) {
            v[k] = i0 + k < ntiles ? tbase[i0 + k] : 0u;
            sv += v[k];
        }
        uint32_t iv = sv; // inclusive over the lanes of the wave
        for (int o = 1; o < ADC_WAVE; o <<= 1) {
            const uint32_t uv = (uint32_t)__shfl_up((int)iv, o, ADC_WAVE);
            if (lane >= o) iv += uv;
        }
        if (lane == ADC_WAVE - 1) s_wave[wave] = iv;
        __syncthreads();
        uint32_t bv = s_carry, total = 0;
        for (int w = 0; w < 16; w++) {
            const uint32_t wv = s_wave[w];
            if (w < wave) bv += wv;
            total += wv;
        }
        bv += iv - sv; // entries of all lanes, waves and turns in front of this lane's first
#pragma unroll
        for (int k = 0; k < TSDF_SCAN_PER_LANE; k++)
            if (i0 + k < ntiles) {
                tbase[i0 + k] = bv;
                bv += v[k];
            }
        __syncthreads();
        if (threadIdx.x == 0) s_carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        rep[1] = s_carry;
        if (count) *count = s_carry;
    }
}

// FIRST (the triangle mesh): additionally first[n] = the rank of voxel n's first crossing, for EVERY voxel that owns a crossing, whatever
// the capacity (a capacity of 0 writes no record: the twin that only ranks)
template <bool FIRST>
__global__ __launch_bounds__(TSDF_WG) void k_tsdf_emit(const TsdfExtArgs g, uint32_t* __restrict__ first)
{
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll 1
    for (int t = 0; t < TSDF_TILES_PER_WAVE; t++) {
        const int tile = ((int)blockIdx.x * TSDF_WAVES + wave) * TSDF_TILES_PER_WAVE + t;
        if (tile >= g.ntiles) continue; // (uniform in the wave)
        uint32_t base = g.tbase[tile];
        if (!FIRST && base >= g.cap) continue; // (uniform: every record of this tile lies behind the capacity)
#pragma unroll 1
        for (int c = 0; c < TSDF_TILE / ADC_WAVE; c++) {
            const int n = tile * TSDF_TILE + c * ADC_WAVE + lane;
            uint32_t word, nb[3];
            int i, j, k;
            bool seen;
            const uint32_t mask = tsdf_lane_crossings(g, n, lane, &word, nb, &i, &j, &k, &seen);
            const uint32_t cnt = (uint32_t)__popc(mask);
            const unsigned long long b0 = __ballot((cnt & 1u) != 0), b1 = __ballot((cnt & 2u) != 0);
            uint32_t rank = base + (uint32_t)__popcll(b0 & below) + 2u * (uint32_t)__popcll(b1 & below);
            base += (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1);
            if (FIRST && mask) first[n] = rank;
            if (!mask || rank >= g.cap) continue;
            const uint32_t ca = g.color ? g.color[n] : 0u;
            const int off[3] = {1, g.vol.nx, g.nxy};
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (!(mask & (1u << a))) continue;
                if (rank < g.cap) {
                    const uint32_t cb = g.color ? g.color[n + off[a]] : 0u;
                    uint32_t rec[4];
                    tsdf_point(g.vol, i, j, k, a, word, nb[a], ca, cb, rec);
                    uint4 pt;
                    pt.x = rec[0]; pt.y = rec[1]; pt.z = rec[2]; pt.w = rec[3];
                    g.points[rank] = pt;
                }
                rank++;
            }
        }
    }
}

static int tsdf_tiles(const adc_tsdf_params& p)
{
    const long long N = (long long)p.nx * p.ny * p.nz;
    return (int)((N + TSDF_TILE - 1) / TSDF_TILE);
}

size_t adc_tsdf_tile_count(const adc_tsdf_params* p) { return (size_t)tsdf_tiles(*p); }

hipError_t adc_launch_tsdf_integrate(adc_handle* h, const float* map, const uint8_t* img, const adc_tsdf_frame* frame)
{
    if (!h->tsdf_vol || !h->tsdf_rep) return hipErrorInvalidValue;
    TsdfIntArgs g;
    g.vol = tsdf_vol(h->tsdf_params);
    g.cam = tsdf_cam(*frame, h->p.W, h->p.H);
    g.map = map;
    g.img = img;
    g.tsdf = h->tsdf_vol;
    g.color = h->tsdf_col;
    g.rep = h->tsdf_rep;
    g.xchunks = (g.vol.nx + TSDF_ROW_VOXELS - 1) / TSDF_ROW_VOXELS;
    g.rows = g.vol.ny * g.vol.nz;
    const int rows_per_wg = TSDF_WAVES * TSDF_ROWS_PER_WAVE;
    const unsigned blocks = (unsigned)g.xchunks * (unsigned)((g.rows + rows_per_wg - 1) / rows_per_wg);
    hipLaunchKernelGGL(k_tsdf_integrate, dim3(blocks), dim3(TSDF_WG), 0, h->stream, g);
    return hipGetLastError();
}

static TsdfExtArgs tsdf_ext_args(adc_handle* h, const AdcTsdfExtReq& r)
{
    TsdfExtArgs g;
    g.vol = tsdf_vol(h->tsdf_params);
    g.tsdf = h->tsdf_vol;
    g.color = h->tsdf_col;
    g.min_weight = r.min_weight;
    g.N = g.vol.nx * g.vol.ny * g.vol.nz;
    g.ntiles = tsdf_tiles(h->tsdf_params);
    g.nxy = g.vol.nx * g.vol.ny;
    g.rep = h->tsdf_rep + ADC_TSDF_REP_EXTRACT;
    g.tbase = h->tsdf_tiles;
    g.points = static_cast<uint4*>(r.points);
    g.cap = r.points ? r.capacity : 0u;
    g.count = r.count;
    return g;
}

static unsigned tsdf_ext_blocks(const TsdfExtArgs& g)
{
    const int per_wg = TSDF_WAVES * TSDF_TILES_PER_WAVE;
    return (unsigned)((g.ntiles + per_wg - 1) / per_wg);
}

hipError_t adc_launch_tsdf_measure(adc_handle* h, const AdcTsdfExtReq& r)
{
    if (!h->tsdf_vol || !h->tsdf_rep || !h->tsdf_tiles) return hipErrorInvalidValue;
    const TsdfExtArgs g = tsdf_ext_args(h, r);
    hipLaunchKernelGGL(k_tsdf_measure, dim3(tsdf_ext_blocks(g)), dim3(TSDF_WG), 0, h->stream, g);
    return hipGetLastError();
}

hipError_t adc_launch_tsdf_scan(adc_handle* h, const AdcTsdfExtReq& r)
{
    const TsdfExtArgs g = tsdf_ext_args(h, r);
    hipLaunchKernelGGL(k_tsdf_scan, dim3(1), dim3(1024), 0, h->stream, g.tbase, g.ntiles, g.rep, g.count);
    return hipGetLastError();
}

hipError_t adc_launch_tsdf_scan_on(adc_handle* h, uint32_t* tbase, int ntiles, uint32_t* rep, uint32_t* count)
{
    hipLaunchKernelGGL(k_tsdf_scan, dim3(1), dim3(1024), 0, h->stream, tbase, ntiles, rep, count);
    return hipGetLastError();
}

hipError_t adc_launch_tsdf_emit(adc_handle* h, const AdcTsdfExtReq& r)
{
    const TsdfExtArgs g = tsdf_ext_args(h, r);
    hipLaunchKernelGGL(k_tsdf_emit<false>, dim3(tsdf_ext_blocks(g)), dim3(TSDF_WG), 0, h->stream, g, static_cast<uint32_t*>(nullptr));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ triangle mesh of the volume (marching cubes)
// include/adcensus_c_api.h: adc_tsdf_mesh_device; the cell rule is tsdf_cell.h, the case table tsdf_mc_table.h (generated).  The
// vertices are the extraction's points; the triangles are a second ordered compaction in the same shape: a lane owns cell n (the cell
// whose corner 0 is voxel n), a wave 64 consecutive n, a tile 256.
//   k_tsdf_mesh_measure  ONE pass for both lists: per tile the number of crossings (the counts of k_tsdf_measure) and the number of
//                        triangles; voxels_seen, cells_seen, cells_surface.  The eight corner words come from the lane's own loads
//                        of the rows (j, k), (j+1, k), (j, k+1), (j+1, k+1); the +x corners from the next lane (lane 63 loads
//                        them).  A chunk of 64 voxels none of which is seen owns no crossing and no seen cell: it leaves after its
//                        first load.  The per-case counts lie in LDS (256 bytes); a lane reads them only for a seen cell whose case
//                        is neither 0 nor 255.
//   k_tsdf_scan          twice: the crossings, the triangles
//   k_tsdf_emit<true>    the vertex records (none with a capacity of 0) and first[n], the rank of voxel n's first crossing
//   k_tsdf_mesh_emit     the cells again; each record behind its tile's base at the prefix three ballots of the per-lane counts (0 to
//                        5) give.  The table lies in LDS (4 KB), rows diverge across the lanes.  The vertex number of an edge is
//                        first[owner] plus the owner's crossings on the axes in front of the edge's (tsdf_vertex_number): a gather
//                        of one rank and up to three voxel words per triangle corner, for surface cells only.
// No float reaches an address; the only atomics are the per-workgroup report adds.
static_assert(TSDF_MC_MAX_TRIS <= 7, "three ballots rank the per-lane triangle counts");
static_assert(TSDF_MC_ROW == 16, "k_tsdf_mesh_emit copies the table with one 16-byte load per lane");

struct TsdfMeshArgs {
    TsdfExtArgs x;          // the vertex side: x.tbase the crossings per tile, x.rep the mesh report words (see below), x.points / x.cap
    uint32_t* tbase_t;      // per tile: triangles -> (scan) triangles of all tiles before it
    uint32_t* first;        // per voxel: the rank of its first crossing (written where it owns one); null when no triangle is written
    uint32_t* tris;         // may be null
    uint32_t tcap;
};
// x.rep: [0] voxels_seen [1] vertices [2] triangles [3] cells_seen [4] cells_surface

// The eight corner words of cell n.  false (uniform in the wave): no voxel of the chunk is seen, nothing was loaded behind w[0].
// Every load lies inside the volume: row (j+1, k) is read only with j + 1 < ny, row (., k+1) only with k + 1 < nz, and n + 1 (+ nx,
// + nxy) only with i + 1 < nx, which keeps it in the same row as n.
__device__ __forceinline__ bool tsdf_lane_corners(const TsdfExtArgs& g, int n, int lane, uint32_t w[8], int* i, int* j, int* k, bool* seen)
{
    const bool in = n < g.N;
    w[0] = in ? g.tsdf[n] : 0u;
    *seen = in && tsdf_seen(w[0], g.min_weight);
    const int row = n / g.vol.nx;
    *i = n - row * g.vol.nx;
    *k = row / g.vol.ny;
    *j = row - *k * g.vol.ny;
    if (!__ballot(*seen)) return false;
    const bool iy = in && *j + 1 < g.vol.ny, iz = in && *k + 1 < g.vol.nz;
    w[2] = iy ? g.tsdf[n + g.vol.nx] : 0u;
    w[4] = iz ? g.tsdf[n + g.nxy] : 0u;
    w[6] = iy && iz ? g.tsdf[n + g.vol.nx + g.nxy] : 0u;
#pragma unroll
    for (int c = 0; c < 8; c += 2) w[c + 1] = (uint32_t)__shfl_down((int)w[c], 1, ADC_WAVE); // (every lane of the wave takes part)
    if (lane == ADC_WAVE - 1 && in && *i + 1 < g.vol.nx) {
        w[1] = g.tsdf[n + 1];
        w[3] = iy ? g.tsdf[n + 1 + g.vol.nx] : 0u;
        w[5] = iz ? g.tsdf[n + 1 + g.nxy] : 0u;
        w[7] = iy && iz ? g.tsdf[n + 1 + g.vol.nx + g.nxy] : 0u;
    }
    return true;
}

// the crossings voxel n owns, counted (the rule of tsdf_lane_crossings on the corner words)
__device__ __forceinline__ uint32_t tsdf_corner_crossings(const TsdfExtArgs& g, const uint32_t w[8], int i, int j, int k)
{
    uint32_t cnt = 0;
    cnt += i + 1 < g.vol.nx && tsdf_crossing(w[0], w[1], g.min_weight) ? 1u : 0u;
    cnt += j + 1 < g.vol.ny && tsdf_crossing(w[0], w[2], g.min_weight) ? 1u : 0u;
    cnt += k + 1 < g.vol.nz && tsdf_crossing(w[0], w[4], g.min_weight) ? 1u : 0u;
    return cnt;
}

// cell n exists and is seen; *index its case
__device__ __forceinline__ bool tsdf_corner_cell(const TsdfExtArgs& g, const uint32_t w[8], bool seen, int i, int j, int k, uint32_t* index)
{
    *index = 0u;
    if (!seen || !tsdf_cell_exists(g.vol, i, j, k) || !tsdf_cell_seen(w, g.min_weight)) return false;
    *index = tsdf_cell_case(w);
    return true;
}

__global__ __launch_bounds__(TSDF_WG) void k_tsdf_mesh_measure(const TsdfMeshArgs g)
{
    __shared__ uint8_t s_count[256];
    __shared__ uint32_t s_rep[3][TSDF_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    s_count[threadIdx.x] = TSDF_MC_TABLE[threadIdx.x * TSDF_MC_ROW]; // (TSDF_WG = 256 = the cases)
    __syncthreads();
    uint32_t n_seen = 0, n_cells = 0, n_surface = 0;
#pragma unroll 1
    for (int t = 0; t < TSDF_TILES_PER_WAVE; t++) {
        const int tile = ((int)blockIdx.x * TSDF_WAVES + wave) * TSDF_TILES_PER_WAVE + t;
        if (tile >= g.x.ntiles) continue; // (uniform in the wave)
        uint32_t total_v = 0, total_t = 0;
#pragma unroll 1
        for (int c = 0; c < TSDF_TILE / ADC_WAVE; c++) {
            const int n = tile * TSDF_TILE + c * ADC_WAVE + lane;
            uint32_t w[8], index;
            int i, j, k;
            bool seen;
            if (!tsdf_lane_corners(g.x, n, lane, w, &i, &j, &k, &seen)) continue; // (uniform: nothing seen in this chunk)
            const uint32_t cv = tsdf_corner_crossings(g.x, w, i, j, k);
            const bool cell = tsdf_corner_cell(g.x, w, seen, i, j, k, &index);
            const uint32_t ct = cell && index != 0u && index != 255u ? (uint32_t)s_count[index] : 0u;
            total_v += (uint32_t)__popcll(__ballot((cv & 1u) != 0)) + 2u * (uint32_t)__popcll(__ballot((cv & 2u) != 0));
            total_t += (uint32_t)__popcll(__ballot((ct & 1u) != 0)) + 2u * (uint32_t)__popcll(__ballot((ct & 2u) != 0)) + 4u * (uint32_t)__popcll(__ballot((ct & 4u) != 0));
            n_seen += (uint32_t)__popcll(__ballot(seen));
            n_cells += (uint32_t)__popcll(__ballot(cell));
            n_surface += (uint32_t)__popcll(__ballot(ct != 0u));
        }
        if (lane == 0) {
            g.x.tbase[tile] = total_v;
            g.tbase_t[tile] = total_t;
        }
    }
    if (lane == 0) {
        s_rep[0][wave] = n_seen;
        s_rep[1][wave] = n_cells;
        s_rep[2][wave] = n_surface;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t t = 0;
        for (int w = 0; w < TSDF_WAVES; w++) t += s_rep[threadIdx.x][w];
        if (t) atomicAdd(&g.x.rep[threadIdx.x == 0 ? 0 : 2 + threadIdx.x], t);
    }
}

__global__ __launch_bounds__(TSDF_WG) void k_tsdf_mesh_emit(const TsdfMeshArgs g)
{
    __shared__ uint4 s_table4[256];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
    s_table4[threadIdx.x] = reinterpret_cast<const uint4*>(TSDF_MC_TABLE)[threadIdx.x]; // (a row of 16 bytes per lane, TSDF_WG = 256 rows)
    __syncthreads();
    const uint8_t* s_table = reinterpret_cast<const uint8_t*>(s_table4);
#pragma unroll 1
    for (int t = 0; t < TSDF_TILES_PER_WAVE; t++) {
        const int tile = ((int)blockIdx.x * TSDF_WAVES + wave) * TSDF_TILES_PER_WAVE + t;
        if (tile >= g.x.ntiles) continue; // (uniform in the wave)
        uint32_t base = g.tbase_t[tile];
        if (base >= g.tcap) continue;     // (uniform: every record of this tile lies behind the capacity)
#pragma unroll 1
        for (int c = 0; c < TSDF_TILE / ADC_WAVE; c++) {
            const int n = tile * TSDF_TILE + c * ADC_WAVE + lane;
            uint32_t w[8], index;
            int i, j, k;
            bool seen;
            if (!tsdf_lane_corners(g.x, n, lane, w, &i, &j, &k, &seen)) continue; // (uniform: no cell, no count)
            const bool cell = tsdf_corner_cell(g.x, w, seen, i, j, k, &index);
            const uint8_t* row = s_table + index * TSDF_MC_ROW;
            const uint32_t ct = cell && index != 0u && index != 255u ? (uint32_t)row[0] : 0u;
            const unsigned long long b0 = __ballot((ct & 1u) != 0), b1 = __ballot((ct & 2u) != 0), b2 = __ballot((ct & 4u) != 0);
            const uint32_t rank = base + (uint32_t)__popcll(b0 & below) + 2u * (uint32_t)__popcll(b1 & below) + 4u * (uint32_t)__popcll(b2 & below);
            base += (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1) + 4u * (uint32_t)__popcll(b2);
            for (uint32_t tr = 0; tr < ct && rank + tr < g.tcap; tr++) {
                uint32_t rec[3];
#pragma unroll
                for (int v = 0; v < 3; v++) {
                    int di, dj, dk;
                    const int axis = tsdf_edge_owner(row[1 + 3 * tr + v], &di, &dj, &dk);
                    const size_t no = (size_t)n + (size_t)di + (size_t)(dj * g.x.vol.nx) + (size_t)(dk * g.x.nxy); // (a corner of an existing cell)
                    rec[v] = tsdf_vertex_number(g.x.vol, g.x.tsdf, g.x.min_weight, g.first[no], no, i + di, j + dj, axis);
                }
                uint32_t* out = g.tris + (size_t)(rank + tr) * 3;
                out[0] = rec[0]; out[1] = rec[1]; out[2] = rec[2];
            }
        }
    }
}

static TsdfMeshArgs tsdf_mesh_args(adc_handle* h, const AdcTsdfMeshReq& r)
{
    AdcTsdfExtReq x;
    x.min_weight = r.min_weight;
    x.points = r.vertices;
    x.capacity = r.vertex_capacity;
    x.count = r.counts;
    TsdfMeshArgs g;
    g.x = tsdf_ext_args(h, x);
    g.x.rep = h->tsdf_rep + ADC_TSDF_REP_MESH;
    g.tbase_t = h->tsdf_tiles + g.x.ntiles;
    g.first = h->tsdf_first;
    g.tris = static_cast<uint32_t*>(r.triangles);
    g.tcap = r.triangles ? r.triangle_capacity : 0u;
    return g;
}

hipError_t adc_launch_tsdf_mesh_measure(adc_handle* h, const AdcTsdfMeshReq& r)
{
    if (!h->tsdf_vol || !h->tsdf_rep || !h->tsdf_tiles) return hipErrorInvalidValue;
    const TsdfMeshArgs g = tsdf_mesh_args(h, r);
    hipLaunchKernelGGL(k_tsdf_mesh_measure, dim3(tsdf_ext_blocks(g.x)), dim3(TSDF_WG), 0, h->stream, g);
    return hipGetLastError();
}

// which: 0 the crossings -> rep[1] and counts[0]; 1 the triangles -> rep[2] and counts[1]
hipError_t adc_launch_tsdf_mesh_scan(adc_handle* h, const AdcTsdfMeshReq& r, int which)
{
    const TsdfMeshArgs g = tsdf_mesh_args(h, r);
    hipLaunchKernelGGL(k_tsdf_scan, dim3(1), dim3(1024), 0, h->stream, which ? g.tbase_t : g.x.tbase, g.x.ntiles, g.x.rep + which, r.counts ? r.counts + which : nullptr);
    return hipGetLastError();
}

// the vertex records and, with_first, the per-voxel ranks the triangles need
hipError_t adc_launch_tsdf_mesh_vertices(adc_handle* h, const AdcTsdfMeshReq& r, bool with_first)
{
    const TsdfMeshArgs g = tsdf_mesh_args(h, r);
    if (with_first && !g.first) return hipErrorInvalidValue;
    if (with_first) hipLaunchKernelGGL(k_tsdf_emit<true>, dim3(tsdf_ext_blocks(g.x)), dim3(TSDF_WG), 0, h->stream, g.x, g.first);
    else hipLaunchKernelGGL(k_tsdf_emit<false>, dim3(tsdf_ext_blocks(g.x)), dim3(TSDF_WG), 0, h->stream, g.x, static_cast<uint32_t*>(nullptr));
    return hipGetLastError();
}

hipError_t adc_launch_tsdf_mesh_triangles(adc_handle* h, const AdcTsdfMeshReq& r)
{
    const TsdfMeshArgs g = tsdf_mesh_args(h, r);
    if (!g.first || !g.tris) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tsdf_mesh_emit, dim3(tsdf_ext_blocks(g.x)), dim3(TSDF_WG), 0, h->stream, g);
    return hipGetLastError();
}
