/* Stub of the moving TSDF volume (include/adcensus_c_api.h: adc_tsdf_shift) for the SANITIZER builds of the host C++ layer, next to
 * stub_capi_tsdf.cpp: the rule of adcensus_amd/csrc/tsdf_shift.h runs serially (tests/emul/tsdf_shift_serial.h) on the stub's host
 * volume, so that the CLI's --tsdf-shift path runs under ASAN / UBSAN and its files can be compared with tests/tsdf_shift_ref.py.  The
 * volume of stub_capi_tsdf.cpp is file-local there: its words come and go through adc_tsdf_download / adc_tsdf_upload; its parameters
 * through this file's adc_tsdf_create, which keeps a copy and calls the one of stub_capi_tsdf_fuse.cpp (the asan build compiles that
 * file with -Dadc_tsdf_create=adc_tsdf_create_fuse).  A shift changes the origin every stub of the chain keeps a copy of: the shifted
 * volume is created anew through the head of the chain (the wrapper of stub_capi_tsdf_mesh.cpp) with the new origin, and the moved
 * words are uploaded.  There is no device memory in the stub, so the device form is refused.
 * Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <cstring>
#include <vector>

#include "../emul/tsdf_shift_serial.h"

struct adc_handle { int w, h; adc_option opt; }; /* (the layout of stub_capi.c) */

static struct {
    int set, rep_valid, moving; /* moving: adc_tsdf_create is called by a shift, the offset stays */
    TsdfMovingVolume m;
    adc_tsdf_shift_report rep;
} s;

extern "C" int adc_tsdf_create_fuse(adc_handle* h, const adc_tsdf_params* params);
extern "C" int __wrap_adc_tsdf_create(adc_handle* h, const adc_tsdf_params* params);
extern "C" int adc_tsdf_create(adc_handle* h, const adc_tsdf_params* params)
{
    const int rc = adc_tsdf_create_fuse(h, params);
    if (s.moving) return rc;
    s.set = rc == 0;
    if (rc == 0) {
        s.m.p = *params;
        for (int a = 0; a < 3; a++) { s.m.origin0[a] = params->origin[a]; s.m.offset[a] = 0; }
    }
    return rc;
}

extern "C" int adc_tsdf_shift(adc_handle* h, const adc_tsdf_shift_params* params, adc_point* points, uint64_t capacity, adc_tsdf_shift_report* report)
{
    if (!h || !params || !s.set || (!points && capacity != 0)) return 1;
    const bool colour = (s.m.p.flags & ADC_TSDF_COLOR) != 0;
    const size_t N = (size_t)s.m.p.nx * s.m.p.ny * s.m.p.nz;
    s.m.tsdf.assign(N, 0u);
    s.m.color.assign(colour ? N : 0, 0u);
    if (adc_tsdf_download(h, s.m.tsdf.data(), colour ? s.m.color.data() : nullptr) != 0) return 1;
    std::vector<adc_point> pts;
    if (tsdf_shift_serial(s.m, *params, pts, &s.rep) != 0) return 1;
    if (!tsdf_shift_is_zero(params->shift)) {
        s.moving = 1;
        const int rc = __wrap_adc_tsdf_create(h, &s.m.p); /* (the new origin reaches every stub's copy) */
        s.moving = 0;
        if (rc != 0 || adc_tsdf_upload(h, s.m.tsdf.data(), colour ? s.m.color.data() : nullptr) != 0) return 2;
    }
    for (size_t i = 0; i < pts.size() && i < capacity; i++) points[i] = pts[i];
    s.rep_valid = 1;
    if (report) *report = s.rep;
    return 0;
}

extern "C" int adc_get_tsdf_shift_report(adc_handle* h, adc_tsdf_shift_report* out)
{
    if (!h || !out || !s.rep_valid) return 1;
    *out = s.rep;
    return 0;
}

extern "C" int adc_tsdf_get_offset(adc_handle* h, int32_t offset[3], float origin0[3])
{
    if (!h || (!offset && !origin0) || !s.set) return 1;
    for (int a = 0; a < 3; a++) {
        if (offset) offset[a] = s.m.offset[a];
        if (origin0) origin0[a] = s.m.origin0[a];
    }
    return 0;
}

extern "C" int adc_tsdf_follow_plan(const adc_tsdf_params* params, const float R[9], const float t[3], const adc_tsdf_follow_params* follow_params, int32_t shift_out[3])
{
    if (!params || !R || !t || !follow_params || !shift_out || tsdf_params_refusal(*params) || tsdf_follow_params_refusal(*follow_params)) return 1;
    tsdf_follow_plan(*params, R, t, *follow_params, shift_out);
    return 0;
}

/* (no device memory in the stub: the device form is never reached by the host layer) */
extern "C" int adc_tsdf_shift_device(adc_handle* h, const adc_tsdf_shift_params* p, void* pts, uint64_t cap, void* cnt)
{
    (void)h; (void)p; (void)pts; (void)cap; (void)cnt;
    return 1;
}
