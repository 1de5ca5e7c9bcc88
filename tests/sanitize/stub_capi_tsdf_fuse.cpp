/* Stub of the stereo-aware TSDF fusion (include/adcensus_c_api.h: adc_tsdf_weights, adc_tsdf_fuse) for the SANITIZER builds of the host
 * C++ layer, next to stub_capi_tsdf.cpp: the rules of adcensus_amd/csrc/tsdf_fuse.h run serially (tests/emul/tsdf_fuse_serial.h) on the
 * stub's host volume, so that the CLI's --tsdf-fuse path runs under ASAN / UBSAN and its files can be compared with
 * tests/tsdf_fuse_ref.py.  The volume of stub_capi_tsdf.cpp is file-local there: its words come and go through adc_tsdf_download /
 * adc_tsdf_upload, its parameters through this file's adc_tsdf_create, which keeps a copy and calls the one of
 * stub_capi_tsdf_track.cpp (the asan build compiles that file with -Dadc_tsdf_create=adc_tsdf_create_trk).  There is no device memory
 * in the stub, so the device forms are refused.  Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <cstring>
#include <vector>

#include "../emul/tsdf_fuse_serial.h"

struct adc_handle { int w, h; adc_option opt; }; /* (the layout of stub_capi.c) */

static struct {
    int set, frep_valid, wrep_valid;
    adc_tsdf_params p;
    adc_tsdf_fuse_report frep;
    adc_tsdf_weight_report wrep;
} u;

extern "C" int adc_tsdf_create_trk(adc_handle* h, const adc_tsdf_params* params);
extern "C" int adc_tsdf_create(adc_handle* h, const adc_tsdf_params* params)
{
    const int rc = adc_tsdf_create_trk(h, params);
    u.set = rc == 0;
    if (rc == 0) u.p = *params;
    return rc;
}

extern "C" int adc_tsdf_weights(adc_handle* h, const float* map, const uint8_t* provenance, const float* confidence, const adc_tsdf_frame* frame,
                                const adc_tsdf_weight_params* params, uint8_t* weight, adc_tsdf_weight_report* report)
{
    const adc_tsdf_weight_params p = params ? *params : TSDF_WEIGHT_DEFAULT;
    if (!h || !map || !weight || !frame || tsdf_frame_refusal(*frame) || tsdf_weight_params_refusal(p)) return 1;
    tsdf_weights_serial(map, provenance, confidence, *frame, p, h->w, h->h, weight, &u.wrep);
    u.wrep_valid = 1;
    if (report) *report = u.wrep;
    return 0;
}

extern "C" int adc_tsdf_fuse(adc_handle* h, const float* map, const uint8_t* bgr_left, const uint8_t* weight, const adc_tsdf_frame* frame,
                             const adc_tsdf_fuse_params* params, adc_tsdf_fuse_report* report)
{
    const adc_tsdf_fuse_params p = params ? *params : TSDF_FUSE_DEFAULT;
    const bool colour = u.set && (u.p.flags & ADC_TSDF_COLOR) != 0;
    if (!h || !map || !frame || tsdf_frame_refusal(*frame) || tsdf_fuse_params_refusal(p) || !u.set || (bgr_left && !colour)) return 1;
    const size_t N = (size_t)u.p.nx * u.p.ny * u.p.nz;
    std::vector<uint32_t> tsdf(N), color(colour ? N : 0);
    if (adc_tsdf_download(h, tsdf.data(), colour ? color.data() : nullptr) != 0) return 1;
    tsdf_fuse_serial(tsdf.data(), colour ? color.data() : nullptr, u.p, *frame, p, map, bgr_left, weight, h->w, h->h, &u.frep);
    if (adc_tsdf_upload(h, tsdf.data(), colour ? color.data() : nullptr) != 0) return 1;
    u.frep_valid = 1;
    if (report) *report = u.frep;
    return 0;
}

extern "C" int adc_get_tsdf_fuse_report(adc_handle* h, adc_tsdf_fuse_report* fuse_report, adc_tsdf_weight_report* weight_report)
{
    if (!h || (!fuse_report && !weight_report) || (fuse_report && !u.frep_valid) || (weight_report && !u.wrep_valid)) return 1;
    if (fuse_report) *fuse_report = u.frep;
    if (weight_report) *weight_report = u.wrep;
    return 0;
}

/* (no device memory in the stub: the device forms are never reached by the host layer) */
extern "C" int adc_tsdf_weights_device(adc_handle* h, const void* m, const void* pr, const void* cf, const adc_tsdf_frame* f, const adc_tsdf_weight_params* p, void* w)
{
    (void)h; (void)m; (void)pr; (void)cf; (void)f; (void)p; (void)w;
    return 1;
}
extern "C" int adc_tsdf_fuse_device(adc_handle* h, const void* m, const void* img, const void* w, const adc_tsdf_frame* f, const adc_tsdf_fuse_params* p)
{
    (void)h; (void)m; (void)img; (void)w; (void)f; (void)p;
    return 1;
}
