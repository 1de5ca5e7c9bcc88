/* Stub of the TSDF volume (include/adcensus_c_api.h: adc_tsdf_*) for the SANITIZER builds of the host C++ layer, next to stub_capi.c:
 * the voxel rule of adcensus_amd/csrc/tsdf_voxel.h run serially, one voxel at a time (tests/emul/tsdf_serial.h), on a volume in host
 * memory, so that the CLI's --tsdf path (<out>-tsdf.ply) runs under ASAN / UBSAN and its file can be compared with tests/tsdf_ref.py.
 * Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../emul/tsdf_serial.h"

struct adc_handle { int w, h; adc_option opt; }; /* (the layout of stub_capi.c) */
static struct {
    int set, irep_valid, xrep_valid;
    adc_tsdf_params p;
    std::vector<uint32_t> tsdf, color;
    adc_tsdf_report irep;
    adc_tsdf_extract_report xrep;
} g;

static size_t voxels() { return (size_t)g.p.nx * g.p.ny * g.p.nz; }

extern "C" int adc_tsdf_create(adc_handle* h, const adc_tsdf_params* params)
{
    if (!h || !params || tsdf_params_refusal(*params)) return 1;
    g.p = *params;
    g.tsdf.assign(voxels(), 0u);
    g.color.assign((params->flags & ADC_TSDF_COLOR) ? voxels() : 0, 0u);
    g.set = 1;
    return 0;
}

extern "C" int adc_tsdf_reset(adc_handle* h)
{
    if (!h || !g.set) return 1;
    g.tsdf.assign(voxels(), 0u);
    g.color.assign(g.color.size(), 0u);
    return 0;
}

extern "C" int adc_tsdf_destroy(adc_handle* h)
{
    if (!h) return 1;
    g.tsdf = std::vector<uint32_t>();
    g.color = std::vector<uint32_t>();
    g.set = 0;
    return 0;
}

extern "C" int adc_tsdf_integrate(adc_handle* h, const float* map, const uint8_t* bgr_left, const adc_tsdf_frame* frame, adc_tsdf_report* report)
{
    if (!h || !map || !frame || tsdf_frame_refusal(*frame) || !g.set || (bgr_left && g.color.empty())) return 1;
    tsdf_integrate_serial(g.tsdf.data(), g.color.empty() ? nullptr : g.color.data(), g.p, *frame, map, bgr_left, h->w, h->h, &g.irep);
    g.irep_valid = 1;
    if (report) *report = g.irep;
    return 0;
}

extern "C" int adc_tsdf_extract(adc_handle* h, const adc_tsdf_extract_params* params, adc_point* points, uint64_t capacity, adc_tsdf_extract_report* report)
{
    const uint32_t min_weight = params ? params->min_weight : 1u;
    if (!h || min_weight < 1u || min_weight > 65535u || (!points && capacity) || !g.set) return 1;
    if (params)
        for (int i = 0; i < 7; i++)
            if (params->reserved_[i]) return 1;
    std::vector<adc_point> pts;
    tsdf_extract_serial(g.tsdf.data(), g.color.empty() ? nullptr : g.color.data(), g.p, min_weight, pts, &g.xrep);
    const size_t n = pts.size() < capacity ? pts.size() : (size_t)capacity;
    if (points && n) memcpy(points, pts.data(), n * sizeof(adc_point));
    g.xrep_valid = 1;
    if (report) *report = g.xrep;
    return 0;
}

extern "C" int adc_get_tsdf_report(adc_handle* h, adc_tsdf_report* integrate_report, adc_tsdf_extract_report* extract_report)
{
    if (!h || (!integrate_report && !extract_report) || (integrate_report && !g.irep_valid) || (extract_report && !g.xrep_valid)) return 1;
    if (integrate_report) *integrate_report = g.irep;
    if (extract_report) *extract_report = g.xrep;
    return 0;
}

/* (no device memory in the stub: the device forms are never reached by the host layer) */
extern "C" int adc_tsdf_integrate_device(adc_handle* h, const void* m, const void* img, const adc_tsdf_frame* f) { (void)h; (void)m; (void)img; (void)f; return 1; }
extern "C" int adc_tsdf_extract_device(adc_handle* h, const adc_tsdf_extract_params* p, void* pts, uint64_t cap, void* n) { (void)h; (void)p; (void)pts; (void)cap; (void)n; return 1; }
extern "C" int adc_tsdf_get_volume_device(adc_handle* h, void** t, void** c, adc_tsdf_params* p) { (void)h; (void)t; (void)c; (void)p; return 1; }

extern "C" int adc_tsdf_download(adc_handle* h, uint32_t* tsdf, uint32_t* color)
{
    if (!h || !tsdf || !g.set || (color && g.color.empty())) return 1;
    memcpy(tsdf, g.tsdf.data(), voxels() * sizeof(uint32_t));
    if (color) memcpy(color, g.color.data(), voxels() * sizeof(uint32_t));
    return 0;
}

extern "C" int adc_tsdf_upload(adc_handle* h, const uint32_t* tsdf, const uint32_t* color)
{
    if (!h || !tsdf || !g.set || (color && g.color.empty())) return 1;
    memcpy(g.tsdf.data(), tsdf, voxels() * sizeof(uint32_t));
    if (color) memcpy(g.color.data(), color, voxels() * sizeof(uint32_t));
    return 0;
}
