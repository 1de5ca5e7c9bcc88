/* Stub of frame-to-model tracking (include/adcensus_c_api.h: adc_tsdf_track) for the SANITIZER builds of the host C++ layer, next to
 * stub_capi_tsdf_raycast.cpp: the rule of adcensus_amd/csrc/tsdf_track.h run serially (tests/emul/tsdf_track_serial.h) against the
 * stub's own ray cast of the stub's host volume, so that the CLI's --tsdf-track path (<out>-track.txt, the report line) runs under
 * ASAN / UBSAN and can be compared with tests/tsdf_track_ref.py.  The volume's parameters are file-local to the other stubs: they come
 * through this file's adc_tsdf_create, which keeps a copy and calls the one of stub_capi_tsdf_raycast.cpp (the asan build compiles
 * that file with -Dadc_tsdf_create=adc_tsdf_create_ray).  There is no device memory in the stub, so the device form is refused.
 * Test infrastructure (adcensus_amd/host/Makefile: `make asan`). */
#include <cstring>
#include <vector>

#include "../emul/tsdf_track_serial.h"

struct adc_handle { int w, h; adc_option opt; }; /* (the layout of stub_capi.c) */

static struct {
    int set, valid;
    adc_tsdf_params p;
    adc_track_result res;
} k;

extern "C" int adc_tsdf_create_ray(adc_handle* h, const adc_tsdf_params* params);
extern "C" int adc_tsdf_create(adc_handle* h, const adc_tsdf_params* params)
{
    const int rc = adc_tsdf_create_ray(h, params);
    k.set = rc == 0;
    if (rc == 0) k.p = *params;
    return rc;
}

/* as adc_tsdf_track of capi.hip: the volume as the frame's own camera sees it from the guess, then the track against those maps */
extern "C" int adc_tsdf_track(adc_handle* h, const float* map, const adc_tsdf_frame* frame, const adc_track_params* params, adc_track_result* result)
{
    if (!h || !map || !frame || !k.set) return 1;
    const adc_track_params p = params ? *params : TRACK_DEFAULT;
    if (tsdf_frame_refusal(*frame) || track_params_refusal(p) || track_size_refusal(h->w, h->h, p.stride)) return 1;
    adc_tsdf_raycast_params view;
    memset(&view, 0, sizeof(view));
    view.width = h->w; view.height = h->h;
    view.focal_px = frame->calib.focal_px; view.cx = frame->calib.cx; view.cy = frame->calib.cy;
    memcpy(view.R, frame->R, sizeof(view.R));
    memcpy(view.t, frame->t, sizeof(view.t));
    view.z_near = k.p.voxel;
    view.z_far = 3.0e38f;
    view.step = k.p.voxel * 0.5f;
    const float half = k.p.trunc * 0.5f;
    view.skip = half > view.step ? half : view.step;
    view.min_weight = 1u;
    view.max_steps = 16384u;
    const size_t P = (size_t)h->w * h->h;
    std::vector<float> depth(P), normals(4 * P);
    if (adc_tsdf_raycast(h, &view, depth.data(), normals.data(), nullptr, nullptr, nullptr) != 0) return 1;
    tsdf_track_serial(map, nullptr, h->w, h->h, *frame, view, depth.data(), normals.data(), p, &k.res, nullptr);
    k.valid = 1;
    if (result) *result = k.res;
    return 0;
}

extern "C" int adc_get_track_result(adc_handle* h, adc_track_result* out)
{
    if (!h || !out || !k.valid) return 1;
    *out = k.res;
    return 0;
}

/* (no device memory in the stub: the device form is never reached by the host layer) */
extern "C" int adc_track_device(adc_handle* h, const void* d_map, const void* d_frame_normals, const adc_tsdf_frame* frame, const adc_tsdf_raycast_params* model_view,
                                const void* d_model_depth, const void* d_model_normals, const adc_track_params* params, void* d_result)
{
    (void)h; (void)d_map; (void)d_frame_normals; (void)frame; (void)model_view; (void)d_model_depth; (void)d_model_normals; (void)params; (void)d_result;
    return 1;
}
