// emul_tsdf_shift.cpp -- adcensus_amd/csrc/tsdf_shift.h compiled alone under g++ (tests/test_tsdf_shift_api.py): a sequence of shifts
// of a volume, one voxel at a time (tsdf_shift_serial.h), and the follow rule on a list of poses, on files the test writes, so that the
// header the kernels include is held to tests/tsdf_shift_ref.py byte for byte on the host.
//
//   emul_tsdf_shift IN_DIR OUT_DIR
// IN_DIR holds case.bin: one adc_tsdf_params, then int32 shifts, follows; then `shifts` adc_tsdf_shift_params, applied one after the
// other; then `follows` records of one adc_tsdf_params, float R[9], float t[3] and one adc_tsdf_follow_params.  init_tsdf.bin and, for
// a colour volume, init_color.bin hold the volume (uint32 per voxel).
// OUT_DIR receives per shift i: tsdf_i.bin, color_i.bin (a colour volume only), points_i.bin (ALL records of the leaving list); and
// reports.bin (one adc_tsdf_shift_report per shift), state.bin (per shift int32 offset[3], float origin[3]) and follow.bin (int32
// shift[3] per record).  Exit 0; 2 for an argument, a file or a parameter it cannot use (a refused shift or follow record included); 3
// when the tile test of the header rules out a tile that holds an edge of the leaving list.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tsdf_shift_serial.h"

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

struct FollowRecord {
    adc_tsdf_params p;
    float R[9], t[3];
    adc_tsdf_follow_params f;
};

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::string ind = argv[1], outd = argv[2];
    FILE* f = fopen((ind + "/case.bin").c_str(), "rb");
    if (!f) return 2;
    TsdfMovingVolume m;
    int32_t counts[2] = {0, 0};
    bool ok = fread(&m.p, sizeof(m.p), 1, f) == 1 && fread(counts, sizeof(counts), 1, f) == 1 && counts[0] >= 0 && counts[0] <= 64 && counts[1] >= 0 && counts[1] <= 4096;
    std::vector<adc_tsdf_shift_params> shifts(ok ? counts[0] : 0);
    std::vector<FollowRecord> follows(ok ? counts[1] : 0);
    ok = ok && (shifts.empty() || fread(shifts.data(), sizeof(shifts[0]), shifts.size(), f) == shifts.size());
    ok = ok && (follows.empty() || fread(follows.data(), sizeof(follows[0]), follows.size(), f) == follows.size());
    ok = ok && fgetc(f) == EOF;
    fclose(f);
    if (!ok || tsdf_params_refusal(m.p)) return 2;
    const size_t N = (size_t)m.p.nx * m.p.ny * m.p.nz;
    if (!read_file(ind + "/init_tsdf.bin", m.tsdf, N)) return 2;
    if ((m.p.flags & ADC_TSDF_COLOR) && !read_file(ind + "/init_color.bin", m.color, N)) return 2;
    for (int a = 0; a < 3; a++) { m.origin0[a] = m.p.origin[a]; m.offset[a] = 0; }

    std::vector<adc_tsdf_shift_report> reports;
    std::vector<uint32_t> state;
    for (size_t i = 0; i < shifts.size(); i++) {
        std::vector<adc_point> pts;
        adc_tsdf_shift_report rep;
        const int rc = tsdf_shift_serial(m, shifts[i], pts, &rep);
        if (rc != 0) return rc == 3 ? 3 : 2;
        reports.push_back(rep);
        for (int a = 0; a < 3; a++) state.push_back((uint32_t)m.offset[a]);
        for (int a = 0; a < 3; a++) state.push_back(reg_float_bits(m.p.origin[a]));
        const std::string tag = "_" + std::to_string(i) + ".bin";
        if (!write_file(outd + "/tsdf" + tag, m.tsdf) || !write_file(outd + "/points" + tag, pts)) return 2;
        if (!m.color.empty() && !write_file(outd + "/color" + tag, m.color)) return 2;
    }
    std::vector<int32_t> plan;
    for (const FollowRecord& r : follows) {
        if (tsdf_params_refusal(r.p) || tsdf_follow_params_refusal(r.f)) return 2;
        int32_t s[3];
        tsdf_follow_plan(r.p, r.R, r.t, r.f, s);
        plan.insert(plan.end(), s, s + 3);
    }
    if (!write_file(outd + "/reports.bin", reports) || !write_file(outd + "/state.bin", state) || !write_file(outd + "/follow.bin", plan)) return 2;
    return 0;
}
