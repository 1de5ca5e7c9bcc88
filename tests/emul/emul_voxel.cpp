// emul_voxel.cpp -- the per-point arithmetic of the voxel-grid filter (adcensus_amd/csrc/voxel_point.h, the header k_voxel.hip includes)
// compiled alone under g++ into a serial program; tests/test_voxel_api.py holds its output to tests/voxel_ref.py bit for bit.
//   emul_voxel axis INV_BITS      stdin: one float per line as hex bits        -> "ok cell q" per line (vox_axis)
//   emul_voxel point LEAF_BITS ZMIN_BITS ZMAX_BITS [12 pose words]  stdin: "X Y Z" hex bits -> "kept key q0 q1 q2" (vox_point)
//   emul_voxel record LEAF_BITS   stdin: "key n sq0 sq1 sq2 sr sg sb" (decimal) -> the four words of the record in hex (vox_record)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../adcensus_amd/csrc/voxel_point.h"

static float bits_float(const char* s)
{
    const uint32_t u = (uint32_t)strtoul(s, nullptr, 16);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    char a[64], b[64], c[64];
    if (!strcmp(argv[1], "axis")) {
        const float inv = bits_float(argv[2]);
        while (scanf("%63s", a) == 1) {
            uint32_t cell = 0, q = 0;
            const bool ok = vox_axis(bits_float(a), inv, &cell, &q);
            printf("%d %u %u\n", ok ? 1 : 0, ok ? cell : 0u, ok ? q : 0u);
        }
        return 0;
    }
    if (!strcmp(argv[1], "point") && (argc == 5 || argc == 17)) {
        VoxGrid g;
        memset(&g, 0, sizeof(g));
        g.leaf = bits_float(argv[2]);
        g.inv = 1.0f / g.leaf;
        g.z_min = bits_float(argv[3]);
        g.z_max = bits_float(argv[4]);
        if (argc == 17) {
            g.flags = ADC_VOXEL_POSE;
            for (int i = 0; i < 9; i++) g.R[i] = bits_float(argv[5 + i]);
            for (int i = 0; i < 3; i++) g.t[i] = bits_float(argv[14 + i]);
        }
        while (scanf("%63s %63s %63s", a, b, c) == 3) {
            unsigned long long key = 0;
            uint32_t q[3] = {0, 0, 0};
            const bool kept = vox_point(g, bits_float(a), bits_float(b), bits_float(c), &key, q);
            if (kept) printf("1 %llu %u %u %u\n", key, q[0], q[1], q[2]);
            else printf("0 0 0 0 0\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "record")) {
        const float leaf = bits_float(argv[2]);
        unsigned long long key, sq[3], sc[3];
        unsigned n;
        while (scanf("%llu %u %llu %llu %llu %llu %llu %llu", &key, &n, &sq[0], &sq[1], &sq[2], &sc[0], &sc[1], &sc[2]) == 8) {
            uint32_t w[4];
            vox_record(key, n, sq, sc, leaf, w);
            printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
        }
        return 0;
    }
    return 2;
}
