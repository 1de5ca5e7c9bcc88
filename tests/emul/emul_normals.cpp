// emul_normals.cpp -- adcensus_amd/csrc/normals_fit.h compiled alone under g++ (tests/test_normals_api.py): the surface normals of a
// whole map, one pixel and one tap at a time, on a file the test writes, so that the header the kernel includes is held to
// tests/normals_ref.py bit for bit on the host.
//
//   emul_normals W H focal cx cy doffs radius max_diff min_points IN_DIR OUT_DIR
// IN_DIR holds map.bin (float32 [H][W]); OUT_DIR receives normals.bin (float32 [H][W][4]), normals8.bin (uint8 [H][W][4]) and
// report.bin (one adc_normals_report).  Exit 0, or 2 for an argument or file it cannot use.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../adcensus_amd/csrc/normals_fit.h"

template <class T>
static bool read_file(const std::string& path, std::vector<T>& v, size_t n)
{
    v.resize(n);
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = fread(v.data(), sizeof(T), n, f);
    const bool at_end = fgetc(f) == EOF;
    fclose(f);
    return got == n && at_end;
}

template <class T>
static bool write_file(const std::string& path, const std::vector<T>& v)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const size_t put = fwrite(v.data(), sizeof(T), v.size(), f);
    return fclose(f) == 0 && put == v.size();
}

int main(int argc, char** argv)
{
    if (argc != 12) return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]);
    if (W < 1 || H < 1 || (long long)W * H > (1LL << 30)) return 2;
    NrmCam cam;
    cam.focal = strtof(argv[3], nullptr);
    cam.cx = strtof(argv[4], nullptr);
    cam.cy = strtof(argv[5], nullptr);
    cam.doffs = strtof(argv[6], nullptr);
    const int r = atoi(argv[7]);
    const float max_diff = strtof(argv[8], nullptr);
    const int min_points = atoi(argv[9]);
    if (r < 1 || r > ADC_NORMALS_MAX_RADIUS || !(std::isfinite(max_diff) && max_diff > 0.0f && max_diff <= 64.0f)) return 2;
    if (min_points < 3 || min_points > (2 * r + 1) * (2 * r + 1)) return 2;
    const int32_t G = (int32_t)rintf(max_diff * 1024.0f);
    const std::string in = argv[10], out = argv[11];
    const size_t P = (size_t)W * (size_t)H;
    std::vector<float> map;
    if (!read_file(in + "/map.bin", map, P)) return 2;

    std::vector<int32_t> q(P);
    for (size_t i = 0; i < P; i++) q[i] = nrm_quantise(map[i]);
    std::vector<float> normals(P * 4, 0.0f);
    std::vector<uint8_t> normals8(P * 4, 0);
    std::vector<adc_normals_report> rep(1);
    rep[0].usable = rep[0].fitted = rep[0].few_points = rep[0].degenerate = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            const int32_t qc = q[p];
            if (qc == NRM_Q_NONE) continue;
            rep[0].usable++;
            NrmSums s = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int dy = -r; dy <= r; dy++)
                for (int dx = -r; dx <= r; dx++) {
                    const int tx = x + dx, ty = y + dy;
                    if (tx < 0 || tx >= W || ty < 0 || ty >= H) continue;
                    const int32_t e = q[(size_t)ty * W + tx] - qc;
                    if (nrm_gate(e, G)) nrm_add_tap(&s, dx, dy, e);
                }
            const NrmPixel o = nrm_fit(s, qc, x, y, cam, min_points);
            rep[0].fitted += o.cls == NRM_FITTED;
            rep[0].few_points += o.cls == NRM_FEW_POINTS;
            rep[0].degenerate += o.cls == NRM_DEGENERATE;
            for (int k = 0; k < 4; k++) {
                normals[p * 4 + k] = o.v[k];
                normals8[p * 4 + k] = (uint8_t)(o.bytes >> (8 * k));
            }
        }
    const bool ok = write_file(out + "/normals.bin", normals) && write_file(out + "/normals8.bin", normals8) && write_file(out + "/report.bin", rep);
    return ok ? 0 : 2;
}
