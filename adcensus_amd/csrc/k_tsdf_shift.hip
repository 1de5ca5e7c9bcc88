// k_tsdf_shift.hip -- the moving TSDF volume (include/adcensus_c_api.h: adc_tsdf_shift_device; the rule is tsdf_shift.h): the window
// shifts by whole voxels, and the crossings with a leaving endpoint are compacted in the extraction's order.
//
//   k_tsdf_shift          OUT OF PLACE, the old planes into a second pair (in place, a shift by a constant linear offset is a race
//                         between workgroups).  The form of k_tsdf_integrate: a lane owns one 16-byte group of the DESTINATION row, a
//                         wave 256 voxels of a row, and walks TSDF_ROWS_PER_WAVE rows.  The range tests are integer comparisons on
//                         the shift and come before any load: no address is formed from a source coordinate that failed them.  Every
//                         destination group is stored as one uint4 (zeros where nothing arrives).  ALIGNED (sx % 4 == 0): the source
//                         group is the destination group moved by whole groups, one uint4 load; otherwise four dwords.  The leaving
//                         voxels are counted where they LIE: the lane also owns the old group at its own place and loads it only when
//                         one of its four voxels leaves (a thin slab for a small shift).  The three counts are reduced in the wave, then
//                         over LDS, then one integer atomic per count and workgroup.  move == 0 (everything leaves; the host clears the
//                         new planes with memsets): the counts only, no source load, no store.
//   k_tsdf_leave_measure  k_tsdf_measure with the leave mask (tsdf_shift_edge_mask) on every lane's crossings; a tile that cannot hold
//   k_tsdf_leave_emit     an edge of the list (tsdf_shift_tile_relevant: uniform in the wave, integers) leaves before its first load:
//                         the measure writes its count of 0, the emit goes on.  Between them k_tsdf_scan as it is.
// Index type: a voxel index n and n + delta are int.  N <= 2^30 (tsdf_params_refusal) and |delta| < N whenever the kernel moves
// anything, because then |s_a| < n_a on every axis (tsdf_shift_all_leave is handled on the host): n + delta < 2^31 -- and it is only
// formed for a source that passed the range tests, where it is the index of a voxel.
#include "adc_internal.h"
#include "tsdf_voxel.h"
#include "tsdf_shift.h"
#include "k_tsdf_ext.h"

struct TsdfShiftArgs {
    TsdfShiftRule rule;
    const uint32_t* src;     // the old planes
    const uint32_t* src_col; // null without a colour volume
    uint32_t* dst;           // the new planes (not read with move == 0)
    uint32_t* dst_col;
    uint32_t min_weight;
    uint32_t* rep;           // [0] moved_nonempty [1] left_nonempty [2] left_seen
    int xchunks, rows;       // 256-voxel pieces of a row; rows = ny * nz
    int delta;               // the source of voxel n is n + delta = n + sx + nx * (sy + ny * sz)
    int move;
};

template <bool ALIGNED>
__global__ __launch_bounds__(TSDF_WG) void k_tsdf_shift(const TsdfShiftArgs g)
{
    __shared__ uint32_t s_cnt[3][TSDF_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const int xc = (int)(blockIdx.x % (unsigned)g.xchunks), rb = (int)(blockIdx.x / (unsigned)g.xchunks);
    const int i0 = xc * TSDF_ROW_VOXELS + lane * 4;
    const bool in = i0 < g.rule.nx; // (nx is a multiple of 4: all four voxels or none)
    const bool with_colour = g.src_col != nullptr && g.dst_col != nullptr;
    uint32_t cnt[3] = {0u, 0u, 0u};
#pragma unroll 1
    for (int r = 0; r < TSDF_ROWS_PER_WAVE; r++) {
        const int row = (rb * TSDF_WAVES + wave) * TSDF_ROWS_PER_WAVE + r;
        if (row >= g.rows || !in) continue;
        const int k = row / g.rule.ny, j = row - k * g.rule.ny;
        const int n = row * g.rule.nx + i0; // (the lane's group, in the old and in the new planes)
        // the old voxels at this place: do they leave?
        const bool row_leaves = tsdf_shift_row_leaves(g.rule, j, k);
        bool lv[4], any_leaves = false;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            lv[e] = row_leaves || tsdf_shift_out(i0 + e, g.rule.sx, g.rule.nx);
            any_leaves = any_leaves || lv[e];
        }
        if (any_leaves) {
            const uint4 o4 = *reinterpret_cast<const uint4*>(g.src + n);
            const uint32_t o[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                cnt[1] += lv[e] && o[e] != 0u ? 1u : 0u;
                cnt[2] += lv[e] && tsdf_seen(o[e], g.min_weight) ? 1u : 0u;
            }
        }
        if (!g.move) continue;
        // the new voxels at this place: what arrives?
        uint32_t w[4] = {0u, 0u, 0u, 0u}, c[4] = {0u, 0u, 0u, 0u};
        if (tsdf_shift_row_has_source(g.rule, j, k)) {
            if (ALIGNED) {
                // i0, sx and nx are multiples of 4: the four sources are one group, inside the row together or not at all
                if (tsdf_shift_in(i0, g.rule.sx, g.rule.nx)) {
                    const uint4 w4 = *reinterpret_cast<const uint4*>(g.src + (n + g.delta));
                    w[0] = w4.x; w[1] = w4.y; w[2] = w4.z; w[3] = w4.w;
                    if (with_colour) {
                        const uint4 c4 = *reinterpret_cast<const uint4*>(g.src_col + (n + g.delta));
                        c[0] = c4.x; c[1] = c4.y; c[2] = c4.z; c[3] = c4.w;
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (tsdf_shift_in(i0 + e, g.rule.sx, g.rule.nx)) {
                        w[e] = g.src[n + g.delta + e];
                        if (with_colour) c[e] = g.src_col[n + g.delta + e];
                    }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) cnt[0] += w[e] != 0u ? 1u : 0u;
        uint4 w4;
        w4.x = w[0]; w4.y = w[1]; w4.z = w[2]; w4.w = w[3];
        *reinterpret_cast<uint4*>(g.dst + n) = w4;
        if (with_colour) {
            uint4 c4;
            c4.x = c[0]; c4.y = c[1]; c4.z = c[2]; c4.w = c[3];
            *reinterpret_cast<uint4*>(g.dst_col + n) = c4;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        uint32_t v = cnt[c];
        for (int o = ADC_WAVE / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_down((int)v, o, ADC_WAVE);
        if (lane == 0) s_cnt[c][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t t = 0;
        for (int w = 0; w < TSDF_WAVES; w++) t += s_cnt[threadIdx.x][w];
        if (t) atomicAdd(&g.rep[threadIdx.x], t);
    }
}

struct TsdfLeaveArgs {
    TsdfExtArgs x;      // the OLD volume with the OLD origin; x.rep is not written by these two kernels
    TsdfShiftRule rule;
};

// the tile may hold an edge of the leaving list (uniform in the wave; the last tile ends with the volume)
__device__ __forceinline__ bool tsdf_leave_tile(const TsdfLeaveArgs& g, int tile)
{
    const int n0 = tile * TSDF_TILE, n1 = adc_imin(n0 + TSDF_TILE, g.x.N) - 1;
    return tsdf_shift_tile_relevant(g.rule, n0, n1);
}

__global__ __launch_bounds__(TSDF_WG) void k_tsdf_leave_measure(const TsdfLeaveArgs g)
{
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
#pragma unroll 1
    for (int t = 0; t < TSDF_TILES_PER_WAVE; t++) {
        const int tile = ((int)blockIdx.x * TSDF_WAVES + wave) * TSDF_TILES_PER_WAVE + t;
        if (tile >= g.x.ntiles) continue; // (uniform in the wave)
        uint32_t total = 0;
        if (tsdf_leave_tile(g, tile)) {
#pragma unroll 1
            for (int c = 0; c < TSDF_TILE / ADC_WAVE; c++) {
                const int n = tile * TSDF_TILE + c * ADC_WAVE + lane;
                uint32_t word, nb[3];
                int i, j, k;
                bool seen;
                uint32_t mask = tsdf_lane_crossings(g.x, n, lane, &word, nb, &i, &j, &k, &seen);
                if (mask) mask &= tsdf_shift_edge_mask(g.rule, i, j, k);
                const uint32_t cnt = (uint32_t)__popc(mask);
                total += (uint32_t)__popcll(__ballot((cnt & 1u) != 0)) + 2u * (uint32_t)__popcll(__ballot((cnt & 2u) != 0));
            }
        }
        if (lane == 0) g.x.tbase[tile] = total; // (the scan reads every tile's count)
    }
}

__global__ __launch_bounds__(TSDF_WG) void k_tsdf_leave_emit(const TsdfLeaveArgs g)
{
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll 1
    for (int t = 0; t < TSDF_TILES_PER_WAVE; t++) {
        const int tile = ((int)blockIdx.x * TSDF_WAVES + wave) * TSDF_TILES_PER_WAVE + t;
        if (tile >= g.x.ntiles) continue;      // (uniform in the wave)
        if (!tsdf_leave_tile(g, tile)) continue; // (uniform: no record, and the next tile's base is this one's)
        uint32_t base = g.x.tbase[tile];
        if (base >= g.x.cap) continue;         // (uniform: every record of this tile lies behind the capacity)
#pragma unroll 1
        for (int c = 0; c < TSDF_TILE / ADC_WAVE; c++) {
            const int n = tile * TSDF_TILE + c * ADC_WAVE + lane;
            uint32_t word, nb[3];
            int i, j, k;
            bool seen;
            uint32_t mask = tsdf_lane_crossings(g.x, n, lane, &word, nb, &i, &j, &k, &seen);
            if (mask) mask &= tsdf_shift_edge_mask(g.rule, i, j, k);
            const uint32_t cnt = (uint32_t)__popc(mask);
            const unsigned long long b0 = __ballot((cnt & 1u) != 0), b1 = __ballot((cnt & 2u) != 0);
            uint32_t rank = base + (uint32_t)__popcll(b0 & below) + 2u * (uint32_t)__popcll(b1 & below);
            base += (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1);
            if (!mask || rank >= g.x.cap) continue;
            const uint32_t ca = g.x.color ? g.x.color[n] : 0u;
            const int off[3] = {1, g.x.vol.nx, g.x.nxy};
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (!(mask & (1u << a))) continue;
                if (rank < g.x.cap) {
                    const uint32_t cb = g.x.color ? g.x.color[n + off[a]] : 0u; // (a crossing: the neighbour lies inside the volume)
                    uint32_t rec[4];
                    tsdf_point(g.x.vol, i, j, k, a, word, nb[a], ca, cb, rec);
                    uint4 pt;
                    pt.x = rec[0]; pt.y = rec[1]; pt.z = rec[2]; pt.w = rec[3];
                    g.x.points[rank] = pt;
                }
                rank++;
            }
        }
    }
}

static TsdfLeaveArgs tsdf_leave_args(adc_handle* h, const AdcTsdfShiftReq& r)
{
    TsdfLeaveArgs g;
    g.x.vol = tsdf_vol(h->tsdf_params);
    g.x.tsdf = h->tsdf_vol;
    g.x.color = h->tsdf_col;
    g.x.min_weight = r.min_weight;
    g.x.N = g.x.vol.nx * g.x.vol.ny * g.x.vol.nz;
    g.x.ntiles = (int)adc_tsdf_tile_count(&h->tsdf_params);
    g.x.nxy = g.x.vol.nx * g.x.vol.ny;
    g.x.rep = nullptr;
    g.x.tbase = h->tsdf_tiles;
    g.x.points = static_cast<uint4*>(r.points);
    g.x.cap = r.points ? r.capacity : 0u;
    g.x.count = r.count;
    g.rule = tsdf_shift_rule(h->tsdf_params, r.shift);
    return g;
}

static unsigned tsdf_leave_blocks(const TsdfLeaveArgs& g)
{
    const int per_wg = TSDF_WAVES * TSDF_TILES_PER_WAVE;
    return (unsigned)((g.x.ntiles + per_wg - 1) / per_wg);
}

hipError_t adc_launch_tsdf_leave_measure(adc_handle* h, const AdcTsdfShiftReq& r)
{
    if (!h->tsdf_vol || !h->tsdf_tiles) return hipErrorInvalidValue;
    const TsdfLeaveArgs g = tsdf_leave_args(h, r);
    hipLaunchKernelGGL(k_tsdf_leave_measure, dim3(tsdf_leave_blocks(g)), dim3(TSDF_WG), 0, h->stream, g);
    return hipGetLastError();
}

hipError_t adc_launch_tsdf_leave_emit(adc_handle* h, const AdcTsdfShiftReq& r)
{
    if (!h->tsdf_vol || !h->tsdf_tiles || !r.points) return hipErrorInvalidValue;
    const TsdfLeaveArgs g = tsdf_leave_args(h, r);
    hipLaunchKernelGGL(k_tsdf_leave_emit, dim3(tsdf_leave_blocks(g)), dim3(TSDF_WG), 0, h->stream, g);
    return hipGetLastError();
}

// the old planes (tsdf_vol, tsdf_col) into the second pair (tsdf_vol2, tsdf_col2); move = false: the counts of a shift by which
// everything leaves (the caller has cleared the second pair)
hipError_t adc_launch_tsdf_shift(adc_handle* h, const AdcTsdfShiftReq& r, bool move)
{
    if (!h->tsdf_vol || !h->tsdf_vol2 || !h->tsdf_shift_rep || (h->tsdf_col && !h->tsdf_col2)) return hipErrorInvalidValue;
    TsdfShiftArgs g;
    g.rule = tsdf_shift_rule(h->tsdf_params, r.shift);
    if (move && tsdf_shift_all_leave(g.rule)) return hipErrorInvalidValue; // (delta is an int only below that)
    g.src = h->tsdf_vol;
    g.src_col = h->tsdf_col;
    g.dst = h->tsdf_vol2;
    g.dst_col = h->tsdf_col ? h->tsdf_col2 : nullptr;
    g.min_weight = r.min_weight;
    g.rep = h->tsdf_shift_rep;
    g.xchunks = (g.rule.nx + TSDF_ROW_VOXELS - 1) / TSDF_ROW_VOXELS;
    g.rows = g.rule.ny * g.rule.nz;
    g.delta = move ? g.rule.sx + g.rule.nx * (g.rule.sy + g.rule.ny * g.rule.sz) : 0;
    g.move = move ? 1 : 0;
    const int rows_per_wg = TSDF_WAVES * TSDF_ROWS_PER_WAVE;
    const unsigned blocks = (unsigned)g.xchunks * (unsigned)((g.rows + rows_per_wg - 1) / rows_per_wg);
    if (move && (g.rule.sx & 3) == 0) hipLaunchKernelGGL(k_tsdf_shift<true>, dim3(blocks), dim3(TSDF_WG), 0, h->stream, g);
    else hipLaunchKernelGGL(k_tsdf_shift<false>, dim3(blocks), dim3(TSDF_WG), 0, h->stream, g);
    return hipGetLastError();
}
