/* Stub of the TSDF volume's ray cast (include/adcensus_c_api.h: adc_tsdf_raycast) for the SANITIZER builds of the host C++ layer, next
 * to stub_capi_tsdf.cpp and stub_capi_tsdf_mesh.cpp: the ray rule of adcensus_amd/csrc/tsdf_ray.h run serially, one ray at a time
 * (tests/emul/tsdf_raycast_serial.h), on the stub's host volume, so that the CLI's --tsdf-raycast path (<out>-ray.pfm, <out>-ray-n.png)
 * runs under ASAN / UBSAN and its files can be compared with tests/tsdf_raycast_ref.py.  The volume of stub_capi_tsdf.cpp is file-local
 * there: its words come through adc_tsdf_download; its parameters through this file's adc_tsdf_create, which keeps a copy and calls
 * the one of stub_capi_tsdf.cpp (the asan build compiles that file with -Dadc_tsdf_create=adc_tsdf_create_base).
 * Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <cstring>
#include <vector>

#include "../emul/tsdf_raycast_serial.h"

static struct {
    int set, rep_valid;
    adc_tsdf_params p;
    adc_tsdf_raycast_report rep;
} r;

extern "C" int adc_tsdf_create_base(adc_handle* h, const adc_tsdf_params* params);
extern "C" int adc_tsdf_create(adc_handle* h, const adc_tsdf_params* params)
{
    const int rc = adc_tsdf_create_base(h, params);
    r.set = rc == 0;
    if (rc == 0) r.p = *params;
    return rc;
}

extern "C" int adc_tsdf_raycast(adc_handle* h, const adc_tsdf_raycast_params* params, float* depth, float* normals, uint8_t* bgr, uint8_t* status,
                                adc_tsdf_raycast_report* report)
{
    if (!h || !params || tsdf_raycast_refusal(*params) || (!depth && !normals && !bgr && !status) || !r.set) return 1;
    const bool colour = (r.p.flags & ADC_TSDF_COLOR) != 0;
    if (bgr && !colour) return 1;
    const size_t N = (size_t)r.p.nx * r.p.ny * r.p.nz;
    std::vector<uint32_t> tsdf(N), color(colour ? N : 0);
    if (adc_tsdf_download(h, tsdf.data(), colour ? color.data() : nullptr) != 0) return 1;
    tsdf_raycast_serial(tsdf.data(), colour ? color.data() : nullptr, r.p, *params, depth, normals, bgr, status, &r.rep);
    r.rep_valid = 1;
    if (report) *report = r.rep;
    return 0;
}

extern "C" int adc_get_tsdf_raycast_report(adc_handle* h, adc_tsdf_raycast_report* out)
{
    if (!h || !out || !r.rep_valid) return 1;
    *out = r.rep;
    return 0;
}

/* (no device memory in the stub: the device form is never reached by the host layer) */
extern "C" int adc_tsdf_raycast_device(adc_handle* h, const adc_tsdf_raycast_params* p, void* d, void* n, void* c, void* s)
{
    (void)h; (void)p; (void)d; (void)n; (void)c; (void)s;
    return 1;
}
