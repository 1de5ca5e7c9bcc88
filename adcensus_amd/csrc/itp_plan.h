// itp_plan.h -- which walk the interpolation stage (K9, k_refine.hip) takes and what it allocates for it, decided as plain values.
// Host-only C++ shared by the product and the CPU tests (tests/emul/emul_itp_plan.cpp): no HIP header, no handle.  The table walk
// (k_interpolate_tab) reads a byte map of the image padded by the search range through a table of linear ray offsets; the f64 walk
// (k_interpolate_rays) needs neither.  adc_create sizes the buffer, upload_tables builds the ray table and adc_launch_interpolation
// picks the kernel -- all three from the ONE predicate below.
#pragma once
#include <cstddef>
#include "adc_device_fn.h"

// search range of the walk: max(|max_disparity|, |min_disparity|) (multistep_refiner.cpp:236), in 64 bits: |INT_MIN| has no int
inline long long adc_itp_max_search(int dmin, int dmax)
{
    const long long a = dmax < 0 ? -(long long)dmax : dmax, i = dmin < 0 ? -(long long)dmin : dmin;
    return a > i ? a : i;
}

// The table walk may run on a W x H image with search range ms:
//   ms <= 30000, W and H < 2^20   the ray table holds lround(m * sin) for integer steps: y + lround(m * sin) == lround(y + m * sin)
//                                 there as long as no entry sits on a rounding tie (upload_tables checks every entry it builds)
//   ms * pitch < 2^24             a hit's linear offset dy * pitch + dx (+ ms) is exact in float: the kernel recovers dy from it by a
//                                 float reciprocal and one correction step
//   pitch * rows < 2^31           32-bit positions in the padded map
inline bool adc_itp_table_walk_ok(int W, int H, long long ms)
{
    if (W < 1 || H < 1 || ms < 1 || ms > 30000 || W >= (1 << 20) || H >= (1 << 20)) return false;
    const long long pitch = adc_itp_code_pitch(W, (int)ms), rows = adc_itp_code_rows(H, (int)ms);
    return ms * pitch < (1LL << 24) && pitch * rows < (1LL << 31);
}

// Layout of the stage's buffer: per pass the cell / row-distance / cell-distance maps (one byte per cell of ADC_ITP_CELL x ADC_ITP_CELL
// pixels each), then -- 16-byte aligned, table walk only -- the two passes' padded code maps.
inline size_t adc_itp_cell_stride(int W, int H) { return 3 * (size_t)((W + ADC_ITP_CELL - 1) / ADC_ITP_CELL) * (size_t)((H + ADC_ITP_CELL - 1) / ADC_ITP_CELL); }
inline size_t adc_itp_code_offset(int W, int H) { return (2 * adc_itp_cell_stride(W, H) + 15) & ~(size_t)15; }
inline size_t adc_itp_code_stride(int W, int H, int ms) { return ((size_t)adc_itp_code_pitch(W, ms) * (size_t)adc_itp_code_rows(H, ms) + 64 + 15) & ~(size_t)15; }
inline size_t adc_itp_cell_maps_bytes(int W, int H) { return adc_itp_code_offset(W, H) + 64; }
// bytes adc_create allocates (and fills with ADC_ITP_OUTSIDE): without the table walk the cell maps alone
inline size_t adc_itp_alloc_bytes(int W, int H, long long ms)
{
    return adc_itp_table_walk_ok(W, H, ms) ? adc_itp_code_offset(W, H) + 2 * adc_itp_code_stride(W, H, (int)ms) + 64 : adc_itp_cell_maps_bytes(W, H);
}
