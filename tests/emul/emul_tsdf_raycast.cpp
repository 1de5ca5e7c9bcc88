// emul_tsdf_raycast.cpp -- adcensus_amd/csrc/tsdf_ray.h compiled alone under g++ (tests/test_tsdf_raycast_api.py): the ray cast of a
// volume, one ray at a time (tsdf_raycast_serial.h), on files the test writes, so that the header the kernel includes is held to
// tests/tsdf_raycast_ref.py bit for bit on the host.
//
//   emul_tsdf_raycast IN_DIR OUT_DIR
// IN_DIR holds case.bin: one adc_tsdf_params, then one adc_tsdf_raycast_params; tsdf.bin and, for a colour volume, color.bin (uint32
// per voxel).  OUT_DIR receives depth.bin, normals.bin, status.bin, for a colour volume bgr.bin, and report.bin (one
// adc_tsdf_raycast_report).  Exit 0, or 2 for an argument or file it cannot use.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tsdf_raycast_serial.h"

template <class T>
static bool read_file(const std::string& path, std::vector<T>& v, size_t n)
{
    v.resize(n);
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = n ? fread(v.data(), sizeof(T), n, f) : 0;
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
    if (argc != 3) return 2;
    const std::string in = argv[1], out = argv[2];
    FILE* f = fopen((in + "/case.bin").c_str(), "rb");
    if (!f) return 2;
    adc_tsdf_params p;
    adc_tsdf_raycast_params view;
    const bool ok = fread(&p, sizeof(p), 1, f) == 1 && fread(&view, sizeof(view), 1, f) == 1 && fgetc(f) == EOF;
    fclose(f);
    if (!ok || tsdf_params_refusal(p) || tsdf_raycast_refusal(view)) return 2;
    const bool colour = (p.flags & ADC_TSDF_COLOR) != 0;
    const size_t N = (size_t)p.nx * p.ny * p.nz, P = (size_t)view.width * view.height;
    std::vector<uint32_t> tsdf, color;
    if (!read_file(in + "/tsdf.bin", tsdf, N)) return 2;
    if (colour && !read_file(in + "/color.bin", color, N)) return 2;
    std::vector<float> depth(P), normals(4 * P);
    std::vector<uint8_t> bgr(colour ? 3 * P : 0), status(P);
    std::vector<adc_tsdf_raycast_report> rep(1);
    tsdf_raycast_serial(tsdf.data(), colour ? color.data() : nullptr, p, view, depth.data(), normals.data(), colour ? bgr.data() : nullptr, status.data(), &rep[0]);
    bool done = write_file(out + "/depth.bin", depth) && write_file(out + "/normals.bin", normals) && write_file(out + "/status.bin", status) &&
                write_file(out + "/report.bin", rep);
    if (colour) done = done && write_file(out + "/bgr.bin", bgr);
    return done ? 0 : 2;
}
