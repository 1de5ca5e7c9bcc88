// emul_itp_plan.cpp -- adcensus_amd/csrc/itp_plan.h compiled alone under g++ (tests/test_emul_itp_plan.py).  Arguments: triples
// W H ms; per triple one line "W H ms ok alloc_bytes cell_maps_bytes pitch rows" (pitch / rows of the padded code map, 0 where the
// search range is beyond what the pitch is defined for).
#include <cstdio>
#include <cstdlib>

#include "../../adcensus_amd/csrc/itp_plan.h"

int main(int argc, char** argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) return 2;
    for (int i = 1; i + 2 < argc; i += 3) {
        const int W = atoi(argv[i]), H = atoi(argv[i + 1]);
        const long long ms = atoll(argv[i + 2]);
        const bool small = ms >= 1 && ms <= (1 << 24);
        printf("%d %d %lld %d %zu %zu %d %d\n", W, H, ms, adc_itp_table_walk_ok(W, H, ms) ? 1 : 0, adc_itp_alloc_bytes(W, H, ms),
               adc_itp_cell_maps_bytes(W, H), small ? adc_itp_code_pitch(W, (int)ms) : 0, small ? adc_itp_code_rows(H, (int)ms) : 0);
    }
    printf("max_search %lld %lld %lld\n", adc_itp_max_search(0, 64), adc_itp_max_search(-70, 10), adc_itp_max_search(-2147483647 - 1, -2147483647));
    return 0;
}
