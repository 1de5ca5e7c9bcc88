// ADCensusStereo.cpp -- C++ facade over the C ABI (include/adcensus_c_api.h).  Host C++ only: every
// device operation happens behind adc_* (HIP, gfx950).  Mirrors the reference's error behaviour
// (ADCensusStereo.cpp:21-144): bool returns, no exceptions.
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"

#include <math.h>
#include <stdlib.h>
#include <new>
#include <vector>

// what SetRectifyMaps / SetRectifyModel were given for one side: applied by Initialize, and again by every Reset
struct ADCensusStereo::RectifySide {
    adc_raw_format raw;
    bool is_model;
    bool convert_only; // SetInputFormat: no maps at all
    adc_camera_model model;
    std::vector<float> map_x, map_y;
    sint32 map_w, map_h;
};

static adc_option to_c(const ADCensusOption& o)
{
    adc_option c;
    adc_option_default(&c);
    c.min_disparity = o.min_disparity;  c.max_disparity = o.max_disparity;
    c.lambda_ad = o.lambda_ad;          c.lambda_census = o.lambda_census;
    c.cross_L1 = o.cross_L1;            c.cross_L2 = o.cross_L2;
    c.cross_t1 = o.cross_t1;            c.cross_t2 = o.cross_t2;
    c.so_p1 = o.so_p1;                  c.so_p2 = o.so_p2;            c.so_tso = o.so_tso;
    c.irv_ts = o.irv_ts;                c.irv_th = o.irv_th;          c.lrcheck_thres = o.lrcheck_thres;
    c.do_lr_check = o.do_lr_check ? 1 : 0;
    c.do_filling = o.do_filling ? 1 : 0;
    c.do_discontinuity_adjustment = o.do_discontinuity_adjustment ? 1 : 0;
    return c;
}

// The reference's Match always prints its six stage-timing lines (ADCensusStereo.cpp:88-129): the look-alike facade does
// too; ADC_VERBOSE=0 in the environment or SetVerbose(false) switches them off (the C ABI underneath, which
// the benchmarks use, prints nothing unless asked).
static bool default_verbose()
{
    const char* e = getenv("ADC_VERBOSE");
    return e ? atoi(e) != 0 : true;
}
ADCensusStereo::ADCensusStereo() : impl_(nullptr), device_(-1), verbose_(default_verbose()), profiling_(false), paper_(0), speckle_size_(0), speckle_diff_(0.0f), width_(0), height_(0)
{
    rect_[0] = rect_[1] = nullptr;
}
ADCensusStereo::~ADCensusStereo()
{
    Release();
    delete rect_[0];
    delete rect_[1];
}

void ADCensusStereo::Release()
{
    if (impl_) adc_destroy(impl_);
    impl_ = nullptr;
}

bool ADCensusStereo::Initialize(const sint32& width, const sint32& height, const ADCensusOption& option)
{
    Release(); // the reference leaks here when called twice without Reset (ADCensusStereo.cpp:43-44); we do not
    const adc_option c = to_c(option);
    impl_ = adc_create(width, height, &c, device_);
    if (!impl_) return false;
    width_ = width; height_ = height;
    if (profiling_) adc_set_profiling(impl_, 1);
    if (verbose_) adc_set_verbose(impl_, 1);
    if (paper_ && adc_set_paper_modes(impl_, paper_) != 0) return false;
    if (speckle_size_ > 0 && adc_set_speckle_filter(impl_, speckle_size_, speckle_diff_) != 0) return false;
    for (int side = 0; side < 2; side++)
        if (rect_[side] && !ApplyRectify(side)) return false;
    return true;
}

bool ADCensusStereo::Match(const uint8* img_left, const uint8* img_right, float32* disp_left)
{
    if (!impl_) return false;                                    // ADCensusStereo.cpp:71-73
    if (!img_left || !img_right || !disp_left) return false;     // :74-76
    return adc_match(impl_, img_left, img_right, disp_left) == 0;
}

bool ADCensusStereo::Reset(const uint32& width, const uint32& height, const ADCensusOption& option)
{
    Release();
    return Initialize(static_cast<sint32>(width), static_cast<sint32>(height), option);
}

void ADCensusStereo::SetVerbose(bool on)
{
    verbose_ = on;
    if (impl_) adc_set_verbose(impl_, on ? 1 : 0);
}
void ADCensusStereo::SetProfiling(bool on)
{
    profiling_ = on;
    if (impl_) adc_set_profiling(impl_, on ? 1 : 0);
}
bool ADCensusStereo::StageMilliseconds(float ms[6]) const { return impl_ && adc_get_stage_ms(impl_, ms, 6) == 0; }
bool ADCensusStereo::MatchAsync(const uint8* l, const uint8* r, float32* d)
{
    if (!impl_ || !l || !r || !d) return false;
    return adc_match_async(impl_, l, r, d) == 0;
}
bool ADCensusStereo::MatchEx(const uint8* l, const uint8* r, float32* d, uint8* provenance, float32* confidence)
{
    if (!impl_ || !l || !r || !d) return false;
    return adc_match_ex(impl_, l, r, d, provenance, confidence) == 0;
}
bool ADCensusStereo::MatchOut(const uint8* l, const uint8* r, float32* d, const adc_outputs* outputs)
{
    if (!impl_ || !l || !r || !d) return false;
    return adc_match_out(impl_, l, r, d, outputs) == 0;
}
unsigned long long ADCensusStereo::CloudCount() const
{
    uint64_t n = 0;
    return impl_ && adc_get_cloud_count(impl_, &n) == 0 ? n : 0;
}
bool ADCensusStereo::MatchProducts(const uint8* l, const uint8* r, float32* d, const adc_products* products)
{
    if (!impl_ || !l || !r || !d) return false;
    return adc_match_products(impl_, l, r, d, products) == 0;
}
bool ADCensusStereo::MatchAsyncProducts(const uint8* l, const uint8* r, float32* d, const adc_products* products)
{
    if (!impl_ || !l || !r || !d) return false;
    return adc_match_async_products(impl_, l, r, d, products) == 0;
}
bool ADCensusStereo::Wait() { return impl_ && adc_wait(impl_) == 0; }
bool ADCensusStereo::SetPaperModes(unsigned modes)
{
    paper_ = modes;
    return impl_ ? adc_set_paper_modes(impl_, modes) == 0 : true; // (before Initialize: applied there)
}
bool ADCensusStereo::SetSpeckleFilter(int max_size, float max_diff)
{
    if (impl_ && adc_set_speckle_filter(impl_, max_size, max_diff) != 0) return false;
    if (!impl_ && !(max_diff >= 0.0f && max_diff <= 3.402823466e38f)) return false; // (before Initialize: checked here, applied there)
    speckle_size_ = max_size > 0 ? max_size : 0;
    speckle_diff_ = max_size > 0 ? max_diff : 0.0f;
    return true;
}

// the argument rules of the set calls (include/adcensus_c_api.h), checked here as well: before Initialize there is no library state to ask
static long long raw_image_bytes(const adc_raw_format* f)
{
    const long long luma = (long long)f->height * f->pitch_bytes;
    return (f->format & 0xff) == ADC_PIX_NV12 ? luma / 2 * 3 : luma;
}
static bool raw_format_ok(const adc_raw_format* f)
{
    if (!f || f->format < 0 || f->format > 0xffff) return false;
    const int c = f->format & 0xff, bits = (f->format >> 8) & 0xff;
    const bool bayer8 = c >= ADC_PIX_BAYER_RGGB8 && c <= ADC_PIX_BAYER_BGGR8, bayer16 = c >= ADC_PIX_BAYER_RGGB16 && c <= ADC_PIX_BAYER_BGGR16;
    const bool wide = c == ADC_PIX_GRAY16 || bayer16, yuv = c == ADC_PIX_YUYV || c == ADC_PIX_UYVY || c == ADC_PIX_NV12;
    int bpp = 0;
    if (c == ADC_PIX_BGR8 || c == ADC_PIX_RGB8) bpp = 3;
    else if (c == ADC_PIX_BGRA8) bpp = 4;
    else if (c == ADC_PIX_GRAY8 || c == ADC_PIX_NV12 || bayer8) bpp = 1;
    else if (wide || c == ADC_PIX_YUYV || c == ADC_PIX_UYVY) bpp = 2;
    if (bpp == 0 || (bits != 0 && !(wide && bits >= 9 && bits <= 16))) return false;
    if (!(f->width >= 1 && f->width <= 32767 && f->height >= 1 && f->height <= 32767 && (long long)f->pitch_bytes >= (long long)f->width * bpp)) return false;
    if ((wide && (f->pitch_bytes & 1)) || ((bayer8 || bayer16) && (f->width < 2 || f->height < 2))) return false;
    if ((yuv && (f->width & 1)) || (c == ADC_PIX_NV12 && (f->height & 1))) return false;
    return raw_image_bytes(f) <= 2147483647LL;
}
bool ADCensusStereo::ApplyRectify(int side)
{
    const RectifySide& r = *rect_[side];
    if (r.convert_only) return adc_set_input_format(impl_, side, &r.raw) == 0; // (refuses a geometry other than width_ x height_)
    if (r.is_model) return adc_set_rectify_model(impl_, side, &r.raw, &r.model) == 0;
    if (r.map_w != width_ || r.map_h != height_) return false; // (the maps have the rectified size)
    return adc_set_rectify_maps(impl_, side, &r.raw, r.map_x.data(), r.map_y.data()) == 0;
}
bool ADCensusStereo::SetRectifyMaps(int side, const adc_raw_format* raw, const float32* map_x, const float32* map_y, sint32 map_width, sint32 map_height)
{
    if ((side != ADC_SIDE_LEFT && side != ADC_SIDE_RIGHT) || !raw_format_ok(raw) || !map_x || !map_y || map_width < 1 || map_height < 1) return false;
    if (impl_ && (map_width != width_ || map_height != height_)) return false;
    RectifySide* r = new (std::nothrow) RectifySide();
    if (!r) return false;
    const size_t n = (size_t)map_width * (size_t)map_height;
    r->raw = *raw; r->is_model = false; r->convert_only = false; r->map_w = map_width; r->map_h = map_height;
    r->map_x.assign(map_x, map_x + n);
    r->map_y.assign(map_y, map_y + n);
    RectifySide* old = rect_[side];
    rect_[side] = r;
    if (impl_ && !ApplyRectify(side)) { rect_[side] = old; delete r; return false; } // (the library's state for this side is unchanged or unset; see adc_last_error)
    delete old;
    return true;
}
bool ADCensusStereo::SetRectifyModel(int side, const adc_raw_format* raw, const adc_camera_model* model)
{
    if ((side != ADC_SIDE_LEFT && side != ADC_SIDE_RIGHT) || !raw_format_ok(raw) || !model) return false;
    const float* v = &model->fx;
    for (size_t i = 0; i < sizeof(adc_camera_model) / sizeof(float); i++)
        if (!std::isfinite(v[i])) return false;
    if (model->fx == 0.0f || model->fy == 0.0f || model->new_fx == 0.0f || model->new_fy == 0.0f) return false;
    RectifySide* r = new (std::nothrow) RectifySide();
    if (!r) return false;
    r->raw = *raw; r->is_model = true; r->convert_only = false; r->model = *model; r->map_w = r->map_h = 0;
    RectifySide* old = rect_[side];
    rect_[side] = r;
    if (impl_ && !ApplyRectify(side)) { rect_[side] = old; delete r; return false; }
    delete old;
    return true;
}
bool ADCensusStereo::SetInputFormat(int side, const adc_raw_format* raw)
{
    if ((side != ADC_SIDE_LEFT && side != ADC_SIDE_RIGHT) || !raw_format_ok(raw)) return false;
    if (impl_ && (raw->width != width_ || raw->height != height_)) return false;
    RectifySide* r = new (std::nothrow) RectifySide();
    if (!r) return false;
    r->raw = *raw; r->is_model = false; r->convert_only = true; r->map_w = r->map_h = 0;
    RectifySide* old = rect_[side];
    rect_[side] = r;
    if (impl_ && !ApplyRectify(side)) { rect_[side] = old; delete r; return false; }
    delete old;
    return true;
}
bool ADCensusStereo::ClearRectify()
{
    if (impl_ && adc_clear_rectify(impl_) != 0) return false;
    delete rect_[0];
    delete rect_[1];
    rect_[0] = rect_[1] = nullptr;
    return true;
}
bool ADCensusStereo::Rectify(int side, const uint8* raw, uint8* bgr_out)
{
    if (!impl_ || !raw || !bgr_out || (side != ADC_SIDE_LEFT && side != ADC_SIDE_RIGHT) || !rect_[side]) return false;
    const size_t n_raw = (size_t)raw_image_bytes(&rect_[side]->raw), n_out = (size_t)width_ * (size_t)height_ * 3;
    void* d_raw = adc_device_malloc(n_raw);
    void* d_out = adc_device_malloc(n_out);
    const bool ok = d_raw && d_out && adc_memcpy_h2d(d_raw, raw, n_raw) == 0 && adc_rectify_device(impl_, side, d_raw, d_out) == 0 && adc_wait(impl_) == 0 &&
                    adc_memcpy_d2h(bgr_out, d_out, n_out) == 0;
    adc_device_free(d_raw);
    adc_device_free(d_out);
    return ok;
}
bool ADCensusStereo::SetGroundTruth(const adc_gt* left, const adc_gt* right, const uint8* nonocc, float32 occ_thres)
{
    return impl_ && adc_set_ground_truth(impl_, left, right, nonocc, occ_thres) == 0;
}
bool ADCensusStereo::ClearGroundTruth() { return impl_ && adc_clear_ground_truth(impl_) == 0; }
bool ADCensusStereo::Evaluate(const float32* disp, const uint8* provenance, const float32* confidence, const adc_eval_params* params, float32* err,
                              uint8* eval_class, adc_eval_report* report)
{
    return impl_ && adc_evaluate(impl_, disp, provenance, confidence, params, err, eval_class, report) == 0;
}
bool ADCensusStereo::EvalReport(adc_eval_report* report) const { return impl_ && adc_get_eval_report(impl_, report) == 0; }
bool ADCensusStereo::SetRegisterTarget(const adc_reg_target* target) { return impl_ && adc_set_register_target(impl_, target) == 0; }
bool ADCensusStereo::ClearRegisterTarget() { return impl_ && adc_clear_register_target(impl_) == 0; }
bool ADCensusStereo::RegisterDepth(const float32* map, int input_kind, const adc_calib* calib, unsigned flags, float32* depth, sint32* index,
                                   adc_reg_report* report)
{
    return impl_ && adc_register_depth(impl_, map, input_kind, calib, flags, depth, index, report) == 0;
}
bool ADCensusStereo::AlignColor(const float32* map, int input_kind, const adc_calib* calib, const uint8* target_bgr, uint8* bgr_out, uint8* valid)
{
    return impl_ && adc_align_color(impl_, map, input_kind, calib, target_bgr, bgr_out, valid) == 0;
}
bool ADCensusStereo::Normals(const float32* disp, const adc_calib* calib, const adc_normals_params* params, float32* normals, uint8* normals8,
                             adc_normals_report* report)
{
    return impl_ && adc_normals(impl_, disp, calib, params, normals, normals8, report) == 0;
}
bool ADCensusStereo::GetNormalsReport(adc_normals_report* report) { return impl_ && adc_get_normals_report(impl_, report) == 0; }
bool ADCensusStereo::Mesh(const float32* disp, const uint8* bgr_left, const adc_calib* calib, const adc_mesh_params* params, adc_point* vertices,
                          uint64 vertex_capacity, sint32* vertex_index, uint32* triangles, uint64 triangle_capacity, adc_mesh_report* report)
{
    return impl_ && adc_mesh(impl_, disp, bgr_left, calib, params, vertices, vertex_capacity, vertex_index, triangles, triangle_capacity, report) == 0;
}
bool ADCensusStereo::GetMeshReport(adc_mesh_report* report) { return impl_ && adc_get_mesh_report(impl_, report) == 0; }

bool ADCensusStereo::TsdfCreate(const adc_tsdf_params* params) { return impl_ && adc_tsdf_create(impl_, params) == 0; }
bool ADCensusStereo::TsdfReset() { return impl_ && adc_tsdf_reset(impl_) == 0; }
bool ADCensusStereo::TsdfIntegrate(const float32* map, const uint8* bgr_left, const adc_tsdf_frame* frame, adc_tsdf_report* report)
{
    return impl_ && adc_tsdf_integrate(impl_, map, bgr_left, frame, report) == 0;
}
bool ADCensusStereo::TsdfExtract(const adc_tsdf_extract_params* params, adc_point* points, uint64 capacity, adc_tsdf_extract_report* report)
{
    return impl_ && adc_tsdf_extract(impl_, params, points, capacity, report) == 0;
}
bool ADCensusStereo::GetTsdfReport(adc_tsdf_report* integrate_report, adc_tsdf_extract_report* extract_report)
{
    return impl_ && adc_get_tsdf_report(impl_, integrate_report, extract_report) == 0;
}
bool ADCensusStereo::TsdfMesh(const adc_tsdf_extract_params* params, adc_point* vertices, uint64 vertex_capacity, uint32* triangles, uint64 triangle_capacity,
                              adc_tsdf_mesh_report* report)
{
    return impl_ && adc_tsdf_mesh(impl_, params, vertices, vertex_capacity, triangles, triangle_capacity, report) == 0;
}
bool ADCensusStereo::GetTsdfMeshReport(adc_tsdf_mesh_report* report) { return impl_ && adc_get_tsdf_mesh_report(impl_, report) == 0; }
bool ADCensusStereo::TsdfRaycast(const TsdfRaycastParams* view, float32* depth, float32* normals, uint8* bgr, uint8* status, adc_tsdf_raycast_report* report)
{
    return impl_ && adc_tsdf_raycast(impl_, view, depth, normals, bgr, status, report) == 0;
}
bool ADCensusStereo::GetTsdfRaycastReport(adc_tsdf_raycast_report* report) { return impl_ && adc_get_tsdf_raycast_report(impl_, report) == 0; }
bool ADCensusStereo::Track(const void* d_map, const void* d_frame_normals, const adc_tsdf_frame* frame, const TsdfRaycastParams* model_view, const void* d_model_depth,
                           const void* d_model_normals, const TrackParams* params, void* d_result)
{
    return impl_ && adc_track_device(impl_, d_map, d_frame_normals, frame, model_view, d_model_depth, d_model_normals, params, d_result) == 0;
}
bool ADCensusStereo::TsdfTrack(const float32* map, const adc_tsdf_frame* frame, const TrackParams* params, TrackResult* result)
{
    return impl_ && adc_tsdf_track(impl_, map, frame, params, result) == 0;
}
bool ADCensusStereo::GetTrackResult(TrackResult* result) { return impl_ && adc_get_track_result(impl_, result) == 0; }
bool ADCensusStereo::TsdfWeights(const float32* map, const uint8* provenance, const float32* confidence, const adc_tsdf_frame* frame, const adc_tsdf_weight_params* params,
                                 uint8* weight, adc_tsdf_weight_report* report)
{
    return impl_ && adc_tsdf_weights(impl_, map, provenance, confidence, frame, params, weight, report) == 0;
}
bool ADCensusStereo::TsdfFuse(const float32* map, const uint8* bgr_left, const uint8* weight, const adc_tsdf_frame* frame, const adc_tsdf_fuse_params* params,
                              adc_tsdf_fuse_report* report)
{
    return impl_ && adc_tsdf_fuse(impl_, map, bgr_left, weight, frame, params, report) == 0;
}
bool ADCensusStereo::GetTsdfFuseReport(adc_tsdf_fuse_report* fuse_report, adc_tsdf_weight_report* weight_report)
{
    return impl_ && adc_get_tsdf_fuse_report(impl_, fuse_report, weight_report) == 0;
}
bool ADCensusStereo::TsdfShift(const adc_tsdf_shift_params* params, adc_point* points, uint64 capacity, adc_tsdf_shift_report* report)
{
    return impl_ && adc_tsdf_shift(impl_, params, points, capacity, report) == 0;
}
bool ADCensusStereo::GetTsdfShiftReport(adc_tsdf_shift_report* report) { return impl_ && adc_get_tsdf_shift_report(impl_, report) == 0; }
bool ADCensusStereo::TsdfGetOffset(sint32 offset[3], float32 origin0[3]) { return impl_ && adc_tsdf_get_offset(impl_, offset, origin0) == 0; }
bool ADCensusStereo::TsdfFollowPlan(const adc_tsdf_params* params, const float32 R[9], const float32 t[3], const adc_tsdf_follow_params* follow_params, sint32 shift_out[3])
{
    return adc_tsdf_follow_plan(params, R, t, follow_params, shift_out) == 0;
}
bool ADCensusStereo::SetCloudVoxelGrid(const adc_voxel_grid* grid) { return impl_ && grid && adc_set_cloud_voxel_grid(impl_, grid) == 0; }
bool ADCensusStereo::ClearCloudVoxelGrid() { return impl_ && adc_clear_cloud_voxel_grid(impl_) == 0; }
bool ADCensusStereo::GetVoxelReport(adc_voxel_report* report) const { return impl_ && report && adc_get_voxel_report(impl_, report) == 0; }
const char* ADCensusStereo::LastError() const { return adc_last_error(); }
