/* Stub of the voxel-grid filter of the cloud (include/adcensus_c_api.h: adc_set_cloud_voxel_grid ... adc_farm_set_cloud_voxel_grid)
 * for the SANITIZER builds of the host C++ layer, next to stub_capi.c: the argument rules of the header in plain C, so that the CLI's
 * --voxel path (parsing, the set call, the report line, the voxel rows of <out>-cloud.txt) runs under ASAN / UBSAN.  The stub does not
 * filter: the cloud of stub_capi_out.c stays the plain one, and the report counts nothing.  Test infrastructure
 * (adcensus_amd/host/Makefile: `make asan`). */
#include <math.h>
#include <string.h>
#include "adcensus_c_api.h"

static int g_set;
static adc_voxel_grid g_grid;

static int grid_ok(const adc_voxel_grid* g)
{
    if (!(isfinite(g->leaf) && g->leaf > 0.0f) || !(g->z_min <= g->z_max) || (g->flags & ~ADC_VOXEL_POSE)) return 0;
    if (g->reserved[0] | g->reserved[1] | g->reserved[2] | g->reserved[3]) return 0;
    for (int i = 0; (g->flags & ADC_VOXEL_POSE) && i < 12; i++)
        if (!isfinite(i < 9 ? g->R[i] : g->t[i - 9])) return 0;
    return 1;
}

int adc_set_cloud_voxel_grid(adc_handle* h, const adc_voxel_grid* grid)
{
    if (!h || !grid || !grid_ok(grid)) return 1;
    g_grid = *grid;
    g_set = 1;
    return 0;
}

int adc_clear_cloud_voxel_grid(adc_handle* h)
{
    if (!h) return 1;
    g_set = 0;
    return 0;
}

int adc_get_voxel_report(adc_handle* h, adc_voxel_report* out)
{
    if (!h || !out) return 1;
    memset(out, 0, sizeof(*out));
    return 0;
}

int adc_farm_set_cloud_voxel_grid(adc_farm* f, const adc_voxel_grid* grid)
{
    if (!f || (grid && !grid_ok(grid))) return 1;
    g_set = grid != NULL;
    if (grid) g_grid = *grid;
    return 0;
}
