// emul_itp_code.cpp -- the two padded code maps of the interpolation's table walk, built on the CPU from the rule of k_refine.hip
// (a pixel is valid in pass 0 when it holds a disparity, in pass 1 also when it is an invalid pixel of the mismatch list) and the three
// functions of adcensus_amd/csrc/adc_device_fn.h, map by map (tests/test_gpu_itp_setup.py).
//   emul_itp_code IN OUT     IN  = int32 W, H, ms; float disp[H][W]; uint8 label[H][W]
//                            OUT = uint8 code[2][rows][pitch], padding included
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../adcensus_amd/csrc/adc_device_fn.h"

static bool valid(const std::vector<float>& disp, const std::vector<uint8_t>& label, size_t p, int pass)
{
    return disp[p] != ADC_INVALID_FLOAT || (pass == 1 && label[p] == ADC_LABEL_MISMATCH);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t hdr[3];
    if (!f || fread(hdr, 4, 3, f) != 3) return 3;
    const int W = hdr[0], H = hdr[1], ms = hdr[2];
    std::vector<float> disp((size_t)W * H);
    std::vector<uint8_t> label((size_t)W * H);
    if (fread(disp.data(), 4, disp.size(), f) != disp.size() || fread(label.data(), 1, label.size(), f) != label.size()) return 3;
    fclose(f);
    const int cw = (W + ADC_ITP_CELL - 1) / ADC_ITP_CELL, ch = (H + ADC_ITP_CELL - 1) / ADC_ITP_CELL;
    const int pitch = adc_itp_code_pitch(W, ms), rows = adc_itp_code_rows(H, ms), gx = ms;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 4;
    for (int pass = 0; pass < 2; pass++) {
        std::vector<uint8_t> cell((size_t)cw * ch), rowd((size_t)cw * ch), cdist((size_t)cw * ch);
        for (int cy = 0; cy < ch; cy++)
            for (int cx = 0; cx < cw; cx++) {
                bool any = false;
                for (int r = 0; r < ADC_ITP_CELL; r++)
                    for (int q = 0; q < ADC_ITP_CELL; q++) {
                        const int y = cy * ADC_ITP_CELL + r, x = cx * ADC_ITP_CELL + q;
                        if (y < H && x < W) any = any || valid(disp, label, (size_t)y * W + x, pass);
                    }
                cell[(size_t)cy * cw + cx] = any ? 1 : 0;
            }
        for (int c = 0; c < cw * ch; c++) rowd[c] = (uint8_t)adc_itp_rowdist(cell.data(), cw, c % cw, c / cw);
        for (int c = 0; c < cw * ch; c++) cdist[c] = (uint8_t)adc_itp_coldist(rowd.data(), cw, ch, c % cw, c / cw);
        std::vector<uint8_t> code((size_t)pitch * rows, (uint8_t)ADC_ITP_OUTSIDE);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                code[(size_t)y * pitch + gx + x] = valid(disp, label, (size_t)y * W + x, pass)
                                                        ? (uint8_t)ADC_ITP_VALID
                                                        : (uint8_t)adc_itp_skip(cdist[(size_t)(y / ADC_ITP_CELL) * cw + x / ADC_ITP_CELL]);
        if (fwrite(code.data(), 1, code.size(), o) != code.size()) return 4;
    }
    return fclose(o) == 0 ? 0 : 4;
}
