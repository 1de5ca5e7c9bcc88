/* Stub of the triangle mesh (include/adcensus_c_api.h: adc_mesh_device, adc_mesh, adc_get_mesh_report) for the SANITIZER builds of
 * the host C++ layer, next to stub_capi.c: the cell rule of adcensus_amd/csrc/mesh_cell.h run serially, one cell at a time
 * (tests/emul/mesh_serial.h), so that the CLI's --mesh path (<out>-mesh.ply) runs under ASAN / UBSAN and its file can be compared
 * with tests/mesh_ref.py.  Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../emul/mesh_serial.h"

struct adc_handle { int w, h; adc_option opt; }; /* (the layout of stub_capi.c) */
static adc_mesh_report g_report;
static int g_report_valid;

extern "C" int adc_mesh(adc_handle* h, const float* disp, const uint8_t* bgr_left, const adc_calib* c, const adc_mesh_params* params, adc_point* vertices,
                        uint64_t vertex_capacity, int32_t* vertex_index, uint32_t* triangles, uint64_t triangle_capacity, adc_mesh_report* report)
{
    const adc_mesh_params def = {1.0f, 1, 0u, {0u, 0u, 0u, 0u, 0u}};
    const adc_mesh_params p = params ? *params : def;
    if (!h || !disp || (c && (!(std::isfinite(c->focal_px) && std::isfinite(c->baseline) && std::isfinite(c->cx) && std::isfinite(c->cy) && std::isfinite(c->doffs)) ||
                              !(c->focal_px > 0.0f))) ||
        !(p.max_diff >= 0.0f) || p.step < 1 || p.step > ADC_MESH_MAX_STEP || p.flags || p.reserved_[0] || p.reserved_[1] || p.reserved_[2] || p.reserved_[3] ||
        p.reserved_[4] || (!vertices && !triangles) || (vertex_index && !vertices))
        return 1;
    std::vector<adc_point> v;
    std::vector<int32_t> vi;
    std::vector<uint32_t> t;
    adc_mesh_report rep;
    mesh_serial(disp, bgr_left, h->w, h->h, c, p.max_diff, p.step, v, vi, t, &rep);
    const size_t nv = v.size() < vertex_capacity ? v.size() : (size_t)vertex_capacity;
    const size_t nt = t.size() / 3 < triangle_capacity ? t.size() / 3 : (size_t)triangle_capacity;
    if (vertices && nv) memcpy(vertices, v.data(), nv * sizeof(adc_point));
    if (vertex_index && nv) memcpy(vertex_index, vi.data(), nv * sizeof(int32_t));
    if (triangles && nt) memcpy(triangles, t.data(), nt * 3 * sizeof(uint32_t));
    g_report = rep;
    g_report_valid = 1;
    if (report) *report = rep;
    return 0;
}

/* (no device memory in the stub: the device form is never reached by the host layer) */
extern "C" int adc_mesh_device(adc_handle* h, const void* d, const void* img, const adc_calib* c, const adc_mesh_params* p, void* v, uint64_t vc, void* vi, void* t,
                               uint64_t tc, void* n)
{
    (void)h; (void)d; (void)img; (void)c; (void)p; (void)v; (void)vc; (void)vi; (void)t; (void)tc; (void)n;
    return 1;
}

extern "C" int adc_get_mesh_report(adc_handle* h, adc_mesh_report* out)
{
    if (!h || !out || !g_report_valid) return 1;
    *out = g_report;
    return 0;
}
