// emul_tsdf_track.cpp -- adcensus_amd/csrc/tsdf_track.h compiled alone under g++ (tests/test_tsdf_track_api.py): the whole tracking
// loop, one pixel and one solve at a time (tsdf_track_serial.h), on files the test writes, so that the header the kernels include is
// held to tests/tsdf_track_ref.py bit for bit on the host.
//
//   emul_tsdf_track IN_DIR OUT_DIR
// IN_DIR holds case.bin: int32 W, H, uint32 has_frame_normals, uint32 0, then one adc_tsdf_frame, one adc_tsdf_raycast_params and one
// adc_track_params; map.bin (float32 [H][W]), fnormals.bin (float32 [H][W][4], only with has_frame_normals), mdepth.bin and
// mnormals.bin (the model view's size).  OUT_DIR receives result.bin (one adc_track_result) and sums.bin (28 int64 per reduce pass
// run).  Exit 0, or 2 for an argument, a parameter or a file it cannot use.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tsdf_track_serial.h"

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
    int32_t head[4];
    adc_tsdf_frame frame;
    adc_tsdf_raycast_params model;
    adc_track_params p;
    const bool ok = fread(head, sizeof(head), 1, f) == 1 && fread(&frame, sizeof(frame), 1, f) == 1 && fread(&model, sizeof(model), 1, f) == 1 &&
                    fread(&p, sizeof(p), 1, f) == 1 && fgetc(f) == EOF;
    fclose(f);
    const int W = head[0], H = head[1];
    if (!ok || head[3] != 0) return 2;
    if (tsdf_frame_refusal(frame) || track_model_refusal(model) || track_params_refusal(p) || track_size_refusal(W, H, p.stride)) return 2;
    const size_t P = (size_t)W * H, M = (size_t)model.width * model.height;
    std::vector<float> map, fnormals, mdepth, mnormals;
    if (!read_file(in + "/map.bin", map, P) || !read_file(in + "/mdepth.bin", mdepth, M) || !read_file(in + "/mnormals.bin", mnormals, 4 * M)) return 2;
    if (head[2] && !read_file(in + "/fnormals.bin", fnormals, 4 * P)) return 2;
    std::vector<adc_track_result> res(1);
    std::vector<long long> sums;
    tsdf_track_serial(map.data(), head[2] ? fnormals.data() : nullptr, W, H, frame, model, mdepth.data(), mnormals.data(), p, &res[0], &sums);
    return write_file(out + "/result.bin", res) && write_file(out + "/sums.bin", sums) ? 0 : 2;
}
