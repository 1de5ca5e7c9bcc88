// emul_tsdf_fuse.cpp -- adcensus_amd/csrc/tsdf_fuse.h compiled alone under g++ (tests/test_tsdf_fuse_api.py): observation weights
// and weighted frames fused into a volume, one pixel and one voxel at a time (tsdf_fuse_serial.h), on files the test writes, so that
// the header the kernels include is held to tests/tsdf_fuse_ref.py bit for bit on the host.
//
//   emul_tsdf_fuse IN_DIR OUT_DIR
// IN_DIR holds case.bin: one adc_tsdf_params, then int32 W, H, frames, has_init, then per frame one adc_tsdf_frame, one
// adc_tsdf_fuse_params, one adc_tsdf_weight_params and int32 with_image, weight_mode (0: no weight map, 1: the frame's plane of
// weights.bin, 2: computed from the map by the weight rule), has_prov, has_conf (read by mode 2); maps.bin (float32 [frames][H][W]);
// img.bin (uint8 [frames][H][W][3]), weights.bin, prov.bin (uint8 [frames][H][W]) and conf.bin (float32 [frames][H][W]), each read when
// a frame needs it; with has_init = 1 init_tsdf.bin and, for a colour volume, init_color.bin (uint32 per voxel).
// OUT_DIR receives tsdf.bin, color.bin (a colour volume only), reports.bin (one adc_tsdf_fuse_report per frame), wmaps.bin (uint8
// [frames][H][W]: the weight map each frame was fused with; all 1 for mode 0) and wreports.bin (one adc_tsdf_weight_report per frame,
// zero unless mode 2).  Exit 0, or 2 for an argument or file it cannot use.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tsdf_fuse_serial.h"

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

struct FrameRec {
    adc_tsdf_frame frame;
    adc_tsdf_fuse_params fuse;
    adc_tsdf_weight_params weight;
    int32_t with_image, weight_mode, has_prov, has_conf;
};

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::string in = argv[1], out = argv[2];
    FILE* f = fopen((in + "/case.bin").c_str(), "rb");
    if (!f) return 2;
    adc_tsdf_params p;
    int32_t head[4];
    bool ok = fread(&p, sizeof(p), 1, f) == 1 && fread(head, sizeof(head), 1, f) == 1;
    const int W = ok ? head[0] : 0, H = ok ? head[1] : 0, frames = ok ? head[2] : 0;
    ok = ok && W >= 1 && H >= 1 && (long long)W * H <= (1LL << 24) && frames >= 0 && frames <= 64 && !tsdf_params_refusal(p);
    std::vector<FrameRec> fr(ok ? frames : 0);
    if (ok && frames) ok = fread(fr.data(), sizeof(FrameRec), frames, f) == (size_t)frames;
    ok = ok && fgetc(f) == EOF;
    fclose(f);
    if (!ok) return 2;
    const bool colour = (p.flags & ADC_TSDF_COLOR) != 0;
    bool any_image = false, any_given = false, any_prov = false, any_conf = false;
    for (int i = 0; i < frames; i++) {
        const FrameRec& r = fr[i];
        if (tsdf_frame_refusal(r.frame) || tsdf_fuse_params_refusal(r.fuse) || (r.with_image && !colour) || r.weight_mode < 0 || r.weight_mode > 2) return 2;
        if (r.weight_mode == 2 && tsdf_weight_params_refusal(r.weight)) return 2;
        any_image = any_image || r.with_image;
        any_given = any_given || r.weight_mode == 1;
        any_prov = any_prov || (r.weight_mode == 2 && r.has_prov);
        any_conf = any_conf || (r.weight_mode == 2 && r.has_conf);
    }
    const size_t P = (size_t)W * H, N = (size_t)p.nx * p.ny * p.nz;
    std::vector<float> maps, conf;
    std::vector<uint8_t> img, given, prov;
    if (!read_file(in + "/maps.bin", maps, P * frames)) return 2;
    if (any_image && !read_file(in + "/img.bin", img, P * 3 * frames)) return 2;
    if (any_given && !read_file(in + "/weights.bin", given, P * frames)) return 2;
    if (any_prov && !read_file(in + "/prov.bin", prov, P * frames)) return 2;
    if (any_conf && !read_file(in + "/conf.bin", conf, P * frames)) return 2;
    std::vector<uint32_t> tsdf(N, 0u), color(colour ? N : 0, 0u);
    if (head[3]) {
        if (!read_file(in + "/init_tsdf.bin", tsdf, N)) return 2;
        if (colour && !read_file(in + "/init_color.bin", color, N)) return 2;
    }

    std::vector<adc_tsdf_fuse_report> reps(frames);
    std::vector<adc_tsdf_weight_report> wreps(frames);
    std::vector<uint8_t> wmaps(P * frames, (uint8_t)1);
    for (int i = 0; i < frames; i++) {
        const FrameRec& r = fr[i];
        uint8_t* w = wmaps.data() + P * i;
        memset(&wreps[i], 0, sizeof(wreps[i]));
        if (r.weight_mode == 1) memcpy(w, given.data() + P * i, P);
        if (r.weight_mode == 2)
            tsdf_weights_serial(maps.data() + P * i, r.has_prov ? prov.data() + P * i : nullptr, r.has_conf ? conf.data() + P * i : nullptr, r.frame, r.weight, W, H, w, &wreps[i]);
        tsdf_fuse_serial(tsdf.data(), colour ? color.data() : nullptr, p, r.frame, r.fuse, maps.data() + P * i, r.with_image ? img.data() + P * 3 * i : nullptr,
                         r.weight_mode ? w : nullptr, W, H, &reps[i]);
    }
    ok = write_file(out + "/tsdf.bin", tsdf) && (!colour || write_file(out + "/color.bin", color)) && write_file(out + "/reports.bin", reps) &&
         write_file(out + "/wmaps.bin", wmaps) && write_file(out + "/wreports.bin", wreps);
    return ok ? 0 : 2;
}
