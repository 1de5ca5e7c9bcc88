/* Stub of the TSDF volume's triangle mesh (include/adcensus_c_api.h: adc_tsdf_mesh) for the SANITIZER builds of the host C++ layer,
 * next to stub_capi_tsdf.cpp: the cell rule of adcensus_amd/csrc/tsdf_cell.h run serially, one cell at a time
 * (tests/emul/tsdf_mesh_serial.h), on the stub's host volume, so that the CLI's --tsdf-mesh path (<out>-tsdf-mesh.ply) runs under
 * ASAN / UBSAN and its file can be compared with tests/tsdf_mesh_ref.py.  The volume of stub_capi_tsdf.cpp is file-local there: its
 * words come through adc_tsdf_download, its parameters through a wrapper around adc_tsdf_create that the asan link line installs
 * (-Wl,--wrap=adc_tsdf_create), which keeps a copy and calls the real function.
 * Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <cstring>
#include <vector>

#include "../emul/tsdf_mesh_serial.h"

static struct {
    int set, rep_valid;
    adc_tsdf_params p;
    adc_tsdf_mesh_report rep;
} m;

extern "C" int __real_adc_tsdf_create(adc_handle* h, const adc_tsdf_params* params);
extern "C" int __wrap_adc_tsdf_create(adc_handle* h, const adc_tsdf_params* params)
{
    const int rc = __real_adc_tsdf_create(h, params);
    m.set = rc == 0;
    if (rc == 0) m.p = *params;
    return rc;
}

extern "C" int adc_tsdf_mesh(adc_handle* h, const adc_tsdf_extract_params* params, adc_point* vertices, uint64_t vertex_capacity, uint32_t* triangles,
                             uint64_t triangle_capacity, adc_tsdf_mesh_report* report)
{
    const uint32_t min_weight = params ? params->min_weight : 1u;
    if (!h || min_weight < 1u || min_weight > 65535u || (!vertices && !triangles) || (!vertices && vertex_capacity) || (!triangles && triangle_capacity) || !m.set ||
        tsdf_mesh_refusal(m.p))
        return 1;
    if (params)
        for (int i = 0; i < 7; i++)
            if (params->reserved_[i]) return 1;
    const size_t N = (size_t)m.p.nx * m.p.ny * m.p.nz;
    const bool colour = (m.p.flags & ADC_TSDF_COLOR) != 0;
    std::vector<uint32_t> tsdf(N), color(colour ? N : 0);
    if (adc_tsdf_download(h, tsdf.data(), colour ? color.data() : nullptr) != 0) return 1;
    std::vector<adc_point> vtx;
    std::vector<uint32_t> tri;
    tsdf_mesh_serial(tsdf.data(), colour ? color.data() : nullptr, m.p, min_weight, vtx, tri, &m.rep);
    const size_t nv = vtx.size() < vertex_capacity ? vtx.size() : (size_t)vertex_capacity;
    const size_t nt = tri.size() / 3 < triangle_capacity ? tri.size() / 3 : (size_t)triangle_capacity;
    if (vertices && nv) memcpy(vertices, vtx.data(), nv * sizeof(adc_point));
    if (triangles && nt) memcpy(triangles, tri.data(), nt * 3 * sizeof(uint32_t));
    m.rep_valid = 1;
    if (report) *report = m.rep;
    return 0;
}

extern "C" int adc_get_tsdf_mesh_report(adc_handle* h, adc_tsdf_mesh_report* out)
{
    if (!h || !out || !m.rep_valid) return 1;
    *out = m.rep;
    return 0;
}

/* (no device memory in the stub: the device form is never reached by the host layer) */
extern "C" int adc_tsdf_mesh_device(adc_handle* h, const adc_tsdf_extract_params* p, void* v, uint64_t vc, void* t, uint64_t tc, void* n)
{
    (void)h; (void)p; (void)v; (void)vc; (void)t; (void)tc; (void)n;
    return 1;
}
