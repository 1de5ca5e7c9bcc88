// emul_tsdf.cpp -- adcensus_amd/csrc/tsdf_voxel.h compiled alone under g++ (tests/test_tsdf_api.py): frames fused into a volume and
// the volume's surface points, one voxel at a time (tsdf_serial.h), on files the test writes, so that the header the kernels
// include is held to tests/tsdf_ref.py bit for bit on the host.
//
//   emul_tsdf IN_DIR OUT_DIR
// IN_DIR holds case.bin: one adc_tsdf_params, then int32 W, H, frames, min_weight, has_init, then `frames` adc_tsdf_frame, then
// `frames` int32 (1: the frame comes with its image); maps.bin (float32 [frames][H][W]); img.bin (uint8 [frames][H][W][3]; read
// when any frame has an image); with has_init = 1 init_tsdf.bin and, for a colour volume, init_color.bin (uint32 per voxel).
// OUT_DIR receives tsdf.bin, color.bin (a colour volume only), reports.bin (one adc_tsdf_report per frame), points.bin (adc_point
// each) and xreport.bin (one adc_tsdf_extract_report).  Exit 0, or 2 for an argument or file it cannot use.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tsdf_serial.h"

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
    int32_t head[5];
    bool ok = fread(&p, sizeof(p), 1, f) == 1 && fread(head, sizeof(head), 1, f) == 1;
    const int W = ok ? head[0] : 0, H = ok ? head[1] : 0, frames = ok ? head[2] : 0;
    ok = ok && W >= 1 && H >= 1 && (long long)W * H <= (1LL << 24) && frames >= 0 && frames <= 64 && head[3] >= 1 && head[3] <= 65535 && !tsdf_params_refusal(p);
    std::vector<adc_tsdf_frame> fr(ok ? frames : 0);
    std::vector<int32_t> with_image(ok ? frames : 0);
    if (ok && frames) ok = fread(fr.data(), sizeof(adc_tsdf_frame), frames, f) == (size_t)frames && fread(with_image.data(), sizeof(int32_t), frames, f) == (size_t)frames;
    ok = ok && fgetc(f) == EOF;
    fclose(f);
    if (!ok) return 2;
    const bool colour = (p.flags & ADC_TSDF_COLOR) != 0;
    bool any_image = false;
    for (int i = 0; i < frames; i++) {
        if (tsdf_frame_refusal(fr[i]) || (with_image[i] && !colour)) return 2;
        any_image = any_image || with_image[i];
    }
    const size_t P = (size_t)W * H, N = (size_t)p.nx * p.ny * p.nz;
    std::vector<float> maps;
    std::vector<uint8_t> img;
    if (!read_file(in + "/maps.bin", maps, P * frames)) return 2;
    if (any_image && !read_file(in + "/img.bin", img, P * 3 * frames)) return 2;
    std::vector<uint32_t> tsdf(N, 0u), color(colour ? N : 0, 0u);
    if (head[4]) {
        if (!read_file(in + "/init_tsdf.bin", tsdf, N)) return 2;
        if (colour && !read_file(in + "/init_color.bin", color, N)) return 2;
    }

    std::vector<adc_tsdf_report> reps(frames);
    for (int i = 0; i < frames; i++)
        tsdf_integrate_serial(tsdf.data(), colour ? color.data() : nullptr, p, fr[i], maps.data() + P * i, with_image[i] ? img.data() + P * 3 * i : nullptr, W, H, &reps[i]);
    std::vector<adc_point> pts;
    std::vector<adc_tsdf_extract_report> xrep(1);
    tsdf_extract_serial(tsdf.data(), colour ? color.data() : nullptr, p, (uint32_t)head[3], pts, &xrep[0]);
    ok = write_file(out + "/tsdf.bin", tsdf) && (!colour || write_file(out + "/color.bin", color)) && write_file(out + "/reports.bin", reps) &&
         write_file(out + "/points.bin", pts) && write_file(out + "/xreport.bin", xrep);
    return ok ? 0 : 2;
}
