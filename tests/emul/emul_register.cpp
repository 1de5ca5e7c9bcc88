// emul_register.cpp -- adcensus_amd/csrc/reg_project.h compiled alone under g++ (tests/test_register_api.py): the whole registration
// run serially -- scatter by minimum, resolve, align -- on files the test writes, so that the header the kernels include is held to
// tests/register_ref.py bit for bit on the host.
//
//   emul_register W H kind splat focal baseline cx cy doffs IN_DIR OUT_DIR
// IN_DIR holds map.bin (float32 [H][W]), target.bin (one adc_reg_target) and tbgr.bin (uint8 [Ht][Wt][3]); OUT_DIR receives depth.bin,
// index.bin, report.bin (one adc_reg_report), aligned.bin and valid.bin.  Exit 0, or 2 for an argument or file it cannot use.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../adcensus_amd/csrc/reg_project.h"

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
    const int W = atoi(argv[1]), H = atoi(argv[2]), kind = atoi(argv[3]), splat = atoi(argv[4]);
    if (W < 1 || H < 1 || (long long)W * H > (1LL << 30)) return 2;
    RegSource s;
    s.kind = kind;
    s.focal = strtof(argv[5], nullptr);
    const float baseline = strtof(argv[6], nullptr);
    s.cx = strtof(argv[7], nullptr);
    s.cy = strtof(argv[8], nullptr);
    s.doffs = strtof(argv[9], nullptr);
    s.fb = s.focal * baseline;
    const std::string in = argv[10], out = argv[11];
    const size_t P = (size_t)W * (size_t)H;
    std::vector<float> map;
    std::vector<adc_reg_target> tv;
    if (!read_file(in + "/map.bin", map, P) || !read_file(in + "/target.bin", tv, 1)) return 2;
    const adc_reg_target T = tv[0];
    if (T.width < 1 || T.width > 32767 || T.height < 1 || T.height > 32767) return 2;
    const size_t Pt = (size_t)T.width * (size_t)T.height;
    std::vector<uint8_t> tbgr;
    if (!read_file(in + "/tbgr.bin", tbgr, Pt * 3)) return 2;

    // scatter by minimum
    std::vector<unsigned long long> zbuf(Pt, REG_KEY_EMPTY);
    std::vector<adc_reg_report> rep(1);
    rep[0].src_valid = rep[0].src_projected = rep[0].dst_filled = rep[0].reserved_ = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            float Z;
            if (!reg_source_z(s, map[(size_t)y * W + x], &Z)) continue;
            rep[0].src_valid++;
            RegFoot f;
            if (!reg_footprint(s, T, x, y, Z, splat != 0, &f)) continue;
            rep[0].src_projected++;
            const unsigned long long key = reg_key(f.zc, W, x, y);
            for (int i = f.i0; i <= f.i1; i++)
                for (int j = f.j0; j <= f.j1; j++) {
                    unsigned long long& z = zbuf[(size_t)i * (size_t)T.width + (size_t)j];
                    if (key < z) z = key;
                }
        }
    // resolve
    std::vector<float> depth(Pt);
    std::vector<int32_t> index(Pt);
    for (size_t i = 0; i < Pt; i++) {
        const bool hit = zbuf[i] != REG_KEY_EMPTY;
        depth[i] = hit ? reg_bits_float((uint32_t)(zbuf[i] >> 32)) : ADC_INVALID_FLOAT;
        index[i] = hit ? (int32_t)(uint32_t)zbuf[i] : -1;
        rep[0].dst_filled += hit ? 1u : 0u;
    }
    // align
    std::vector<uint8_t> aligned(P * 3, 0), valid(P, 0);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int i, j;
            const size_t p = (size_t)y * W + x;
            if (!reg_align_tap(s, T, x, y, map[p], &i, &j)) continue;
            const uint8_t* c = &tbgr[((size_t)i * (size_t)T.width + (size_t)j) * 3];
            aligned[p * 3 + 0] = c[0];
            aligned[p * 3 + 1] = c[1];
            aligned[p * 3 + 2] = c[2];
            valid[p] = 1;
        }
    const bool ok = write_file(out + "/depth.bin", depth) && write_file(out + "/index.bin", index) && write_file(out + "/report.bin", rep) &&
                    write_file(out + "/aligned.bin", aligned) && write_file(out + "/valid.bin", valid);
    return ok ? 0 : 2;
}
