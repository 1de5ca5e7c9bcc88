// emul_mesh.cpp -- adcensus_amd/csrc/mesh_cell.h compiled alone under g++ (tests/test_mesh_api.py): the triangle mesh of a whole map,
// one cell at a time (mesh_serial.h), on files the test writes, so that the header the kernels include is held to tests/mesh_ref.py
// bit for bit on the host.
//
//   emul_mesh W H CALIBRATED focal baseline cx cy doffs max_diff step WITH_IMAGE IN_DIR OUT_DIR
// IN_DIR holds map.bin (float32 [H][W]) and, with WITH_IMAGE = 1, img.bin (uint8 [H][W][3]); OUT_DIR receives vertices.bin (adc_point
// each), vindex.bin (int32 each), triangles.bin (uint32 x 3 each) and report.bin (one adc_mesh_report).  Exit 0, or 2 for an argument or
// file it cannot use.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mesh_serial.h"

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
    const size_t put = v.empty() ? 0 : fwrite(v.data(), sizeof(T), v.size(), f);
    return fclose(f) == 0 && put == v.size();
}

int main(int argc, char** argv)
{
    if (argc != 14) return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]);
    if (W < 1 || H < 1 || (long long)W * H > (1LL << 30)) return 2;
    const int calibrated = atoi(argv[3]);
    adc_calib calib;
    calib.focal_px = strtof(argv[4], nullptr);
    calib.baseline = strtof(argv[5], nullptr);
    calib.cx = strtof(argv[6], nullptr);
    calib.cy = strtof(argv[7], nullptr);
    calib.doffs = strtof(argv[8], nullptr);
    const float max_diff = strtof(argv[9], nullptr);
    const int step = atoi(argv[10]);
    const int with_image = atoi(argv[11]);
    if (!(max_diff >= 0.0f) || step < 1 || step > ADC_MESH_MAX_STEP) return 2;
    const std::string in = argv[12], out = argv[13];
    const size_t P = (size_t)W * (size_t)H;
    std::vector<float> map;
    std::vector<uint8_t> img;
    if (!read_file(in + "/map.bin", map, P)) return 2;
    if (with_image && !read_file(in + "/img.bin", img, P * 3)) return 2;

    std::vector<adc_point> vertices;
    std::vector<int32_t> vindex;
    std::vector<uint32_t> triangles;
    std::vector<adc_mesh_report> rep(1);
    mesh_serial(map.data(), with_image ? img.data() : nullptr, W, H, calibrated ? &calib : nullptr, max_diff, step, vertices, vindex, triangles, &rep[0]);
    const bool ok = write_file(out + "/vertices.bin", vertices) && write_file(out + "/vindex.bin", vindex) && write_file(out + "/triangles.bin", triangles) &&
                    write_file(out + "/report.bin", rep);
    return ok ? 0 : 2;
}
