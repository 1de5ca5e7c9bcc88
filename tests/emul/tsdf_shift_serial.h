// tsdf_shift_serial.h -- adcensus_amd/csrc/tsdf_shift.h walked serially over a whole volume: the moving volume of
// include/adcensus_c_api.h (adc_tsdf_shift) on the host, for tests/emul/emul_tsdf_shift.cpp and tests/sanitize/stub_capi_tsdf_shift.cpp.
// The leaving list is walked tile by tile as the kernels walk it, so that the tile test of the header is exercised: a tile it rules
// out is still searched, and an edge found there is an error of the header (false is returned).
#pragma once
#include <cstring>
#include <vector>

#include "../../adcensus_amd/csrc/tsdf_shift.h"

#define TSDF_SHIFT_SERIAL_TILE 256 // the tile of the extraction kernels

// the state of a volume that moves: its words, its parameters with the CURRENT origin, the origin at creation, the total offset
struct TsdfMovingVolume {
    adc_tsdf_params p;
    float origin0[3];
    int32_t offset[3];
    std::vector<uint32_t> tsdf, color; // color empty without ADC_TSDF_COLOR
};

// the leaving list of shift s on the volume as it is (ALL records); false: the tile test ruled out a tile that holds an edge
inline bool tsdf_leaving_serial(const TsdfMovingVolume& m, const int32_t s[3], uint32_t min_weight, std::vector<adc_point>& pts)
{
    const TsdfVol v = tsdf_vol(m.p);
    const TsdfShiftRule r = tsdf_shift_rule(m.p, s);
    const uint32_t* tsdf = m.tsdf.data();
    const uint32_t* color = m.color.empty() ? nullptr : m.color.data();
    const int N = v.nx * v.ny * v.nz;
    const int off[3] = {1, v.nx, v.nx * v.ny};
    pts.clear();
    for (int n0 = 0; n0 < N; n0 += TSDF_SHIFT_SERIAL_TILE) {
        const int n1 = (n0 + TSDF_SHIFT_SERIAL_TILE < N ? n0 + TSDF_SHIFT_SERIAL_TILE : N) - 1;
        const bool relevant = tsdf_shift_tile_relevant(r, n0, n1);
        for (int n = n0; n <= n1; n++) {
            const int row = n / v.nx, i = n - row * v.nx, k = row / v.ny, j = row - k * v.ny;
            const uint32_t edges = tsdf_shift_edge_mask(r, i, j, k);
            if (edges && !relevant) return false;
            if (!edges || !tsdf_seen(tsdf[n], min_weight)) continue;
            const bool inside[3] = {i + 1 < v.nx, j + 1 < v.ny, k + 1 < v.nz};
            for (int a = 0; a < 3; a++) {
                if (!(edges & (1u << a)) || !inside[a] || !tsdf_crossing(tsdf[n], tsdf[n + off[a]], min_weight)) continue;
                uint32_t rec[4];
                tsdf_point(v, i, j, k, a, tsdf[n], tsdf[n + off[a]], color ? color[n] : 0u, color ? color[n + off[a]] : 0u, rec);
                adc_point pt;
                memcpy(&pt, rec, sizeof(pt));
                pts.push_back(pt);
            }
        }
    }
    return true;
}

// One shift: the list (ALL records), the report, the moved words, the offset and the origin.  0, 1 = refused (nothing changed), 3 = the
// tile test of the header is wrong.
inline int tsdf_shift_serial(TsdfMovingVolume& m, const adc_tsdf_shift_params& sp, std::vector<adc_point>& pts, adc_tsdf_shift_report* rep)
{
    int32_t offset[3];
    memset(rep, 0, sizeof(*rep));
    pts.clear();
    if (tsdf_shift_params_refusal(sp) || tsdf_shift_offset_refusal(m.offset, sp.shift, offset)) return 1;
    if (tsdf_shift_is_zero(sp.shift)) return 0;
    if (!tsdf_leaving_serial(m, sp.shift, sp.min_weight, pts)) return 3;
    rep->points = (uint32_t)pts.size();
    const TsdfShiftRule r = tsdf_shift_rule(m.p, sp.shift);
    const size_t N = (size_t)r.nx * r.ny * r.nz;
    const bool all = tsdf_shift_all_leave(r);
    const long long delta = all ? 0 : (long long)r.sx + (long long)r.nx * ((long long)r.sy + (long long)r.ny * (long long)r.sz);
    std::vector<uint32_t> tsdf(N, 0u), color(m.color.empty() ? 0 : N, 0u);
    for (int k = 0; k < r.nz; k++)
        for (int j = 0; j < r.ny; j++)
            for (int i = 0; i < r.nx; i++) {
                const size_t n = ((size_t)k * r.ny + j) * r.nx + i;
                if (tsdf_shift_leaves(r, i, j, k)) {
                    rep->left_nonempty += m.tsdf[n] != 0u ? 1u : 0u;
                    rep->left_seen += tsdf_seen(m.tsdf[n], sp.min_weight) ? 1u : 0u;
                }
                if (!tsdf_shift_has_source(r, i, j, k)) continue;
                const size_t from = (size_t)((long long)n + delta);
                tsdf[n] = m.tsdf[from];
                if (!color.empty()) color[n] = m.color[from];
                rep->moved_nonempty += tsdf[n] != 0u ? 1u : 0u;
            }
    m.tsdf.swap(tsdf);
    m.color.swap(color);
    for (int a = 0; a < 3; a++) {
        m.offset[a] = offset[a];
        m.p.origin[a] = tsdf_shift_origin(m.origin0[a], offset[a], m.p.voxel);
    }
    return 0;
}
