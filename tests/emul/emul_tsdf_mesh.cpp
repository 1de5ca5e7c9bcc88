// emul_tsdf_mesh.cpp -- adcensus_amd/csrc/tsdf_cell.h (and the generated case table) compiled alone under g++
// (tests/test_tsdf_mesh_api.py): the triangle mesh of a volume, one cell at a time (tsdf_mesh_serial.h), on files the test writes, so
// that the header the kernels include is held to tests/tsdf_mesh_ref.py bit for bit on the host.
//
//   emul_tsdf_mesh IN_DIR OUT_DIR
// IN_DIR holds case.bin: one adc_tsdf_params, then int32 min_weight; tsdf.bin and, for a colour volume, color.bin (uint32 per voxel).
// OUT_DIR receives vertices.bin (adc_point each), triangles.bin (three uint32 each) and report.bin (one adc_tsdf_mesh_report).
// Exit 0, or 2 for an argument or file it cannot use.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tsdf_mesh_serial.h"

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
    int32_t min_weight = 0;
    bool ok = fread(&p, sizeof(p), 1, f) == 1 && fread(&min_weight, sizeof(min_weight), 1, f) == 1 && fgetc(f) == EOF;
    fclose(f);
    if (!ok || min_weight < 1 || min_weight > 65535 || tsdf_params_refusal(p) || tsdf_mesh_refusal(p)) return 2;
    const bool colour = (p.flags & ADC_TSDF_COLOR) != 0;
    const size_t N = (size_t)p.nx * p.ny * p.nz;
    std::vector<uint32_t> tsdf, color;
    if (!read_file(in + "/tsdf.bin", tsdf, N)) return 2;
    if (colour && !read_file(in + "/color.bin", color, N)) return 2;
    std::vector<adc_point> vtx;
    std::vector<uint32_t> tri;
    std::vector<adc_tsdf_mesh_report> rep(1);
    tsdf_mesh_serial(tsdf.data(), colour ? color.data() : nullptr, p, (uint32_t)min_weight, vtx, tri, &rep[0]);
    return write_file(out + "/vertices.bin", vtx) && write_file(out + "/triangles.bin", tri) && write_file(out + "/report.bin", rep) ? 0 : 2;
}
