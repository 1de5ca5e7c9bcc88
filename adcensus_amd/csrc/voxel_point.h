// voxel_point.h -- per-point arithmetic of the voxel-grid filter of the cloud (k_voxel.hip; include/adcensus_c_api.h holds the
// definition in words, tests/voxel_ref.py in numpy).  Plain inline functions shared by the kernels and by a g++-compiled serial
// program (tests/emul/emul_voxel.cpp): no HIP header, no handle.
//
// IEEE binary32, one rounding per operation, nothing fused (the pragma of adc_device_fn.h; the .hip files are compiled with
// -ffp-contract=off as well), divisions correctly rounded, every expression parenthesised in the order of the definition.
// No float reaches an integer conversion unbounded: an axis is in range only with |u| < 2^20, f * 65536 lies in [0, 65536].
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/adcensus_c_api.h"
#include "adc_device_fn.h"

// the grid as the kernels take it: the caller's parameters and inv = 1.0f / leaf (one division on the host)
struct VoxGrid {
    float leaf, inv, z_min, z_max;
    uint32_t flags;
    float R[9], t[3];
};

#define VOX_CELL_BIAS 1048576     // 2^20: a cell index i in [-2^20, 2^20) is kept as i + 2^20, 21 bits
#define VOX_CELL_LIMIT 1048576.0f
#define VOX_KEY_NONE (~0ull)      // no key has bit 63 set (three 21-bit cells)

ADC_HD uint32_t vox_float_bits(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
#endif
}

// one axis: the biased cell and the 16-bit position inside it; false: out of range (NaN included)
ADC_HD bool vox_axis(float w, float inv, uint32_t* cell, uint32_t* q)
{
    const float u = w * inv;
    if (!(__builtin_fabsf(u) < VOX_CELL_LIMIT)) return false;
    const float i = __builtin_floorf(u);
    const float f = u - i; // (one rounding: exactly 1.0f for a tiny negative u)
    const uint32_t qq = (uint32_t)(f * 65536.0f);
    *q = qq < 65535u ? qq : 65535u;
    *cell = (uint32_t)((int32_t)i + VOX_CELL_BIAS);
    return true;
}

// the camera-frame point (X, Y, Z) of a cloud-valid pixel -> key and q[3]; false: cropped or out of range on an axis
ADC_HD bool vox_point(const VoxGrid& g, float X, float Y, float Z, unsigned long long* key, uint32_t q[3])
{
    if (!(g.z_min <= Z && Z <= g.z_max)) return false;
    float xw = X, yw = Y, zw = Z;
    if (g.flags & ADC_VOXEL_POSE) {
        xw = ((g.R[0] * X + g.R[1] * Y) + g.R[2] * Z) + g.t[0];
        yw = ((g.R[3] * X + g.R[4] * Y) + g.R[5] * Z) + g.t[1];
        zw = ((g.R[6] * X + g.R[7] * Y) + g.R[8] * Z) + g.t[2];
    }
    uint32_t cx, cy, cz;
    if (!vox_axis(xw, g.inv, &cx, &q[0])) return false;
    if (!vox_axis(yw, g.inv, &cy, &q[1])) return false;
    if (!vox_axis(zw, g.inv, &cz, &q[2])) return false;
    *key = ((unsigned long long)cx << 42) | ((unsigned long long)cy << 21) | (unsigned long long)cz;
    return true;
}

// rounded integer mean of a sum over n >= 1 points
ADC_HD uint32_t vox_mean(unsigned long long sum, uint32_t n) { return (uint32_t)((sum + n / 2u) / n); }

// one coordinate of a voxel's record: the biased cell and the mean position inside it -> metric (two roundings: the inner product is exact)
ADC_HD float vox_coord(uint32_t cell, uint32_t mq, float leaf)
{
    const float i = (float)((int32_t)cell - VOX_CELL_BIAS);
    return (i + (float)mq * 0x1p-16f) * leaf;
}

// the record of a voxel (adc_point as four words): coordinates, rounded mean colour, pad = min(n, 255)
ADC_HD void vox_record(unsigned long long key, uint32_t n, const unsigned long long sq[3], const unsigned long long sc[3], float leaf, uint32_t out[4])
{
    const uint32_t cell[3] = {(uint32_t)(key >> 42) & 0x1fffffu, (uint32_t)(key >> 21) & 0x1fffffu, (uint32_t)key & 0x1fffffu};
    for (int a = 0; a < 3; a++) out[a] = vox_float_bits(vox_coord(cell[a], vox_mean(sq[a], n), leaf));
    out[3] = vox_mean(sc[0], n) | (vox_mean(sc[1], n) << 8) | (vox_mean(sc[2], n) << 16) | ((n < 255u ? n : 255u) << 24);
}
