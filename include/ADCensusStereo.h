/*
 * ADCensusStereo.h -- drop-in C++ facade of the MI355X-native AD-Census matcher.
 *
 * Same public surface as the reference's class (ADCensusStereo.h:14-41):
 *     bool Initialize(const sint32& width, const sint32& height, const ADCensusOption& option);
 *     bool Match(const uint8* img_left, const uint8* img_right, float32* disp_left);
 *     bool Reset(const uint32& width, const uint32& height, const ADCensusOption& option);
 * so the reference's caller (main.cpp:80-118) compiles unchanged.  The private part is a pimpl over
 * the C ABI of include/adcensus_c_api.h (HIP kernels for gfx950); there is no CPU path.
 *
 * Additive members (no reference counterpart): SetDevice, SetVerbose (prints the reference's six stage
 * timing lines, ADCensusStereo.cpp:88-129: ON by default like the reference, ADC_VERBOSE=0 or SetVerbose(false) turns them off), StageMilliseconds, MatchAsync/Wait,
 * MatchEx (per-pixel provenance and confidence maps next to the disparity), MatchOut (depth, point cloud and 8-bit image computed
 * on the device from the final map), SetSpeckleFilter (optional removal of small disparity islands on the device, off by default),
 * SetRectifyMaps / SetRectifyModel / ClearRectify / Rectify (optional rectification of raw camera images on the device, off by default),
 * SetGroundTruth / ClearGroundTruth / Evaluate / EvalReport (optional scoring of a map against ground truth on the device),
 * SetRegisterTarget / ClearRegisterTarget / RegisterDepth / AlignColor (optional registration of depth into a second camera on the device),
 * Normals / GetNormalsReport (optional camera-facing surface normals from a disparity map on the device),
 * Mesh / GetMeshReport (optional triangle mesh from a disparity map on the device),
 * TsdfCreate / TsdfReset / TsdfIntegrate / TsdfExtract / GetTsdfReport (optional TSDF volume on the device: maps of many frames fused, surface points),
 * TsdfMesh / GetTsdfMeshReport (the volume's surface as a triangle mesh),
 * TsdfRaycast / GetTsdfRaycastReport (the volume seen from a camera pose: depth, normal, colour and status maps),
 * Track / TsdfTrack / GetTrackResult (frame-to-model camera tracking against the ray cast's maps: the pose the next TsdfIntegrate needs),
 * TsdfWeights / TsdfFuse / GetTsdfFuseReport (stereo-aware fusion: per-pixel observation weights, gated bilinear reading of the map),
 * TsdfShift / GetTsdfShiftReport / TsdfGetOffset / TsdfFollowPlan (moving volume: the window shifts by whole voxels, the surface that leaves is handed out once),
 * MatchProducts / MatchAsyncProducts (every optional product of one Match through one request, synchronous or completed by Wait).
 */
#pragma once

#include "adcensus_types.h"

struct adc_handle;
struct adc_outputs; // include/adcensus_c_api.h
struct adc_products;
struct adc_raw_format;
struct adc_camera_model;
struct adc_gt;
struct adc_eval_params;
struct adc_eval_report;
struct adc_calib;
struct adc_reg_target;
struct adc_reg_report;
struct adc_voxel_grid;
struct adc_voxel_report;
struct adc_normals_params;
struct adc_normals_report;
struct adc_mesh_params;
struct adc_mesh_report;
struct adc_tsdf_params;
struct adc_tsdf_frame;
struct adc_tsdf_report;
struct adc_tsdf_extract_params;
struct adc_tsdf_weight_params;
struct adc_tsdf_weight_report;
struct adc_tsdf_fuse_params;
struct adc_tsdf_fuse_report;
struct adc_tsdf_shift_params;
struct adc_tsdf_shift_report;
struct adc_tsdf_follow_params;
struct adc_tsdf_extract_report;
struct adc_tsdf_mesh_report;
struct adc_tsdf_raycast_params;
struct adc_tsdf_raycast_report;
typedef adc_tsdf_raycast_params TsdfRaycastParams; // the view of TsdfRaycast: include/adcensus_c_api.h holds its fields
struct adc_track_params;
struct adc_track_result;
typedef adc_track_params TrackParams;   // include/adcensus_c_api.h holds the fields
typedef adc_track_result TrackResult;
struct adc_point;

class ADCensusStereo {
public:
    ADCensusStereo();
    ~ADCensusStereo();
    ADCensusStereo(const ADCensusStereo&) = delete;
    ADCensusStereo& operator=(const ADCensusStereo&) = delete;

    /** Allocates all device buffers once. false: width/height <= 0, empty disparity range
     *  (ADCensusStereo.cpp:31-40), range > ADC_MAX_DISP_RANGE (2047), W*H > 2^30, or a HIP failure. */
    bool Initialize(const sint32& width, const sint32& height, const ADCensusOption& option);

    /** Left-view sub-pixel disparity map of the pair (uint8 [H][W][3] BGR each) into the caller's
     *  float32 [H][W].  false: not initialised or a null pointer (ADCensusStereo.cpp:71-76), HIP failure. */
    bool Match(const uint8* img_left, const uint8* img_right, float32* disp_left);

    /** Release + Initialize (ADCensusStereo.cpp:134-144). */
    bool Reset(const uint32& width, const uint32& height, const ADCensusOption& option);

    // ---- additive API ----
    void SetDevice(int device) { device_ = device; }
    void SetVerbose(bool on);
    /** ms of the 6 stages of the last Match (cost, arms, aggregate, scanline, wta, refine); needs SetProfiling(true). */
    void SetProfiling(bool on);
    bool StageMilliseconds(float ms[6]) const;
    bool MatchAsync(const uint8* img_left, const uint8* img_right, float32* disp_left);
    /** Match plus optional per-pixel maps (adc_match_ex, include/adcensus_c_api.h): provenance uint8 [H][W], code = lr | fill << 2
     *  (ADC_LR_* / ADC_FILL_*), and confidence float32 [H][W] in [0, 1]; either may be null (both null: exactly Match).  false
     *  where Match is false, and when a map is requested with paper modes set. */
    bool MatchEx(const uint8* img_left, const uint8* img_right, float32* disp_left, uint8* provenance, float32* confidence);
    /** Match plus the outputs computed on the device from the final map (adc_match_out, include/adcensus_c_api.h: adc_outputs with
     *  host pointers): metric depth float32 [H][W] (needs a calibration), the point cloud of the valid pixels in raster order, the
     *  min-max normalised 8-bit image.  A null request or one that asks for nothing is exactly Match.  false where Match is
     *  false, and when the request is refused (depth without a calibration, focal_px <= 0, a non-finite calibration field). */
    bool MatchOut(const uint8* img_left, const uint8* img_right, float32* disp_left, const adc_outputs* outputs);
    /** Valid pixels of the last MatchOut that asked for a cloud (whatever the capacity was). */
    unsigned long long CloudCount() const;
    /** Match plus every optional product through ONE request (adc_match_products, include/adcensus_c_api.h: adc_products with host
     *  pointers): provenance and confidence of MatchEx, depth / cloud / 8-bit image of MatchOut, and the map in 16-bit fixed point
     *  (disp16, scale 256 = KITTI's encoding), all from the same Match.  A null request or one that asks for nothing is exactly
     *  Match.  false where Match is false, and when the request is refused (what MatchEx and MatchOut refuse, a disp16_scale that is
     *  not finite or <= 0, a Match pending). */
    bool MatchProducts(const uint8* img_left, const uint8* img_right, float32* disp_left, const adc_products* products);
    /** The same, only enqueued (adc_match_async_products): the images may be reused at once, Wait delivers the map and every
     *  product; the product buffers belong to the library until then. */
    bool MatchAsyncProducts(const uint8* img_left, const uint8* img_right, float32* disp_left, const adc_products* products);
    bool Wait();
    /** Opt-in paper features the reference declares / stores but does not implement (bit 0: 5x5 census, adcensus_types.h:39-42;
     *  bit 1: averaged instead of chained scanline paths; bit 2: right-image arms, cross_aggregator.h:91).  0 (default) = the
     *  reference's behaviour; anything else changes the results by definition.  Call after Initialize. */
    bool SetPaperModes(unsigned modes);
    /** Optional speckle filter (adc_set_speckle_filter, include/adcensus_c_api.h): every later Match / MatchAsync / MatchEx / MatchOut
     *  delivers the map with every 4-connected component (neighbours within max_diff) of at most max_size pixels set to
     *  Invalid_Float; the outputs of MatchOut come from the filtered map.  max_size <= 0 (default) = off.  false: max_diff negative
     *  or not finite, a Match pending, or a HIP failure.  May be called before Initialize (applied there). */
    bool SetSpeckleFilter(int max_size, float max_diff);
    /** Optional rectification on the device (adc_set_rectify_maps / adc_set_rectify_model, include/adcensus_c_api.h).  Once BOTH sides
     *  (ADC_SIDE_LEFT, ADC_SIDE_RIGHT) are set, every Match / MatchAsync / MatchEx / MatchOut takes img_left / img_right as RAW images
     *  of the declared geometry (raw->height * raw->pitch_bytes bytes each) and matches their rectified W x H versions.  The maps are
     *  float32 [map_height][map_width] source coordinates and must have the size given to Initialize.  false: a refused argument, a
     *  Match pending, a HIP failure.  May be called before Initialize: checked as far as possible, copied, applied there
     *  (Initialize then returns false when the library refuses them). */
    bool SetRectifyMaps(int side, const adc_raw_format* raw, const float32* map_x, const float32* map_y, sint32 map_width, sint32 map_height);
    bool SetRectifyModel(int side, const adc_raw_format* raw, const adc_camera_model* model);
    /** Conversion only, for cameras whose frames are already rectified (adc_set_input_format): declares the frames of one side as `raw`
     *  -- any ADC_PIX_* layout: Bayer, YUYV / UYVY, NV12, 16-bit, or an 8-bit one; raw->width / height must be the size given to
     *  Initialize -- without maps.  It sets the side like the two calls above (any mix works).  May be called before Initialize: checked
     *  as far as possible, kept, applied there. */
    bool SetInputFormat(int side, const adc_raw_format* raw);
    /** Both sides unset: Match takes rectified W x H BGR images again. */
    bool ClearRectify();
    /** The remap alone, host to host: raw image of the side's geometry -> uint8 [H][W][3] BGR.  Needs Initialize and the side set. */
    bool Rectify(int side, const uint8* raw, uint8* bgr_out);
    /** Optional evaluation against ground truth on the device (adc_set_ground_truth / adc_evaluate, include/adcensus_c_api.h): the
     *  ground truth of the left view, optionally of the right view (occlusion by cross-check within occ_thres) or a non-occlusion
     *  mask, all host arrays.  Needs Initialize; Initialize / Reset drop it (it belongs to the matcher object underneath).  false: a
     *  refused argument, a Match pending, a HIP failure. */
    bool SetGroundTruth(const adc_gt* left, const adc_gt* right, const uint8* nonocc, float32 occ_thres);
    bool ClearGroundTruth();
    /** Scores a float32 [H][W] host map (any map of this geometry: a Match result, a filtered one, another matcher's) against the
     *  ground truth set: integer report (bad pixels per threshold, error sums, histograms; all / non-occluded / per provenance fill
     *  class / per confidence bin), optionally the per-pixel error and class maps.  provenance, confidence, params (one threshold of
     *  1.0), err, eval_class and report may be null.  false where the library refuses (no ground truth, confidence without
     *  provenance, a bad threshold) and on a HIP failure. */
    bool Evaluate(const float32* disp, const uint8* provenance, const float32* confidence, const adc_eval_params* params, float32* err,
                  uint8* eval_class, adc_eval_report* report);
    /** The report of the last evaluation completed on this object. */
    bool EvalReport(adc_eval_report* report) const;
    /** Optional registration of depth into a second camera on the device ("align depth to colour"; adc_set_register_target /
     *  adc_register_depth / adc_align_color, include/adcensus_c_api.h holds the definition).  The target -- size, intrinsics, distortion,
     *  R and t from the left rectified camera -- is state of the matcher object underneath: needs Initialize, and Initialize / Reset
     *  drop it.  false: a refused target (a size outside [1, 32767], a non-finite field, fx or fy == 0), a Match pending, a HIP failure. */
    bool SetRegisterTarget(const adc_reg_target* target);
    bool ClearRegisterTarget();
    /** Registers a float32 [H][W] host map (input_kind ADC_REG_FROM_DISPARITY or ADC_REG_FROM_DEPTH, calib the rectified left camera)
     *  into the target: depth float32 [Ht][Wt] (+inf where nothing landed) and index int32 [Ht][Wt] (source raster index, -1), either
     *  may be null, not both; flags: ADC_REG_NO_SPLAT.  report may be null. */
    bool RegisterDepth(const float32* map, int input_kind, const adc_calib* calib, unsigned flags, float32* depth, sint32* index,
                       adc_reg_report* report);
    /** The other direction: bgr_out uint8 [H][W][3] takes, per source pixel, the colour of target_bgr uint8 [Ht][Wt][3] at the pixel's
     *  projection (0 and valid = 0 where there is none); valid uint8 [H][W] may be null. */
    bool AlignColor(const float32* map, int input_kind, const adc_calib* calib, const uint8* target_bgr, uint8* bgr_out, uint8* valid);
    /** Optional surface normals from a float32 [H][W] host disparity map on the device (adc_normals, include/adcensus_c_api.h holds the
     *  definition: a windowed plane fit in disparity space, solved exactly in integers).  calib the rectified left camera; params may be
     *  null (r = 2, max_diff = 1.0, min_points = 5).  normals float32 [H][W][4] = the unit normal facing the camera and the support
     *  count, zeros where there is none; normals8 uint8 [H][W][4] = the same as a normal-map image; either may be null, not both.
     *  report may be null. */
    bool Normals(const float32* disp, const adc_calib* calib, const adc_normals_params* params, float32* normals, uint8* normals8,
                 adc_normals_report* report);
    bool GetNormalsReport(adc_normals_report* report);
    /** Optional triangle mesh from a float32 [H][W] host disparity map on the device (adc_mesh, include/adcensus_c_api.h holds the
     *  definition: gated grid cells over the lattice of every step-th pixel).  bgr_left uint8 [H][W][3] may be null (colours 0), calib
     *  may be null (vertices (x, y, |d|)), params may be null (max_diff = 1.0, step = 1).  vertices takes the first
     *  min(count, vertex_capacity) adc_point records, vertex_index (may be null) their source raster indices, triangles the first
     *  min(count, triangle_capacity) records of three uint32 vertex numbers; vertices or triangles may be null, not both.  report may
     *  be null. */
    bool Mesh(const float32* disp, const uint8* bgr_left, const adc_calib* calib, const adc_mesh_params* params, adc_point* vertices,
              uint64 vertex_capacity, sint32* vertex_index, uint32* triangles, uint64 triangle_capacity, adc_mesh_report* report);
    bool GetMeshReport(adc_mesh_report* report);
    /** Optional TSDF volume on the device (adc_tsdf_*, include/adcensus_c_api.h holds the definition).  TsdfCreate allocates and
     *  zeroes a volume (a second call replaces it; adc_tsdf_params: size, voxel, origin, trunc, crop, max_weight, ADC_TSDF_COLOR),
     *  TsdfReset empties it.  TsdfIntegrate fuses one float32 [H][W] host map (a disparity or a depth map, frame->kind) seen from
     *  frame->R, frame->t (WORLD -> camera); bgr_left uint8 [H][W][3] may be null and needs a colour volume; report may be null.
     *  TsdfExtract writes the first min(points, capacity) surface points (adc_point, world frame) and reports how many there are;
     *  params may be null (min_weight = 1), points may be null with capacity 0 (counts only), report may be null.  GetTsdfReport: the
     *  reports of the last completed calls; either may be null. */
    bool TsdfCreate(const adc_tsdf_params* params);
    bool TsdfReset();
    bool TsdfIntegrate(const float32* map, const uint8* bgr_left, const adc_tsdf_frame* frame, adc_tsdf_report* report);
    bool TsdfExtract(const adc_tsdf_extract_params* params, adc_point* points, uint64 capacity, adc_tsdf_extract_report* report);
    bool GetTsdfReport(adc_tsdf_report* integrate_report, adc_tsdf_extract_report* extract_report);
    /** The volume's surface as a triangle mesh (adc_tsdf_mesh: marching cubes on the device).  The vertices are the points of
     *  TsdfExtract in the same order; a triangle is three uint32 vertex numbers.  The first min(count, capacity) records of each list
     *  are written; a list whose pointer is null is not wanted (at least one must be), a capacity of 0 counts only; params and report
     *  may be null.  GetTsdfMeshReport: the report of the last completed call. */
    bool TsdfMesh(const adc_tsdf_extract_params* params, adc_point* vertices, uint64 vertex_capacity, uint32* triangles, uint64 triangle_capacity,
                  adc_tsdf_mesh_report* report);
    bool GetTsdfMeshReport(adc_tsdf_mesh_report* report);
    /** The volume seen from a camera pose (adc_tsdf_raycast: one ray per pixel marched through the volume on the device).  Host
     *  buffers of the VIEW's size, each may be null (at least one must not be): depth float32 [height][width] (0 where no surface is
     *  hit), normals float32 [height][width][4] in the camera frame, bgr uint8 [height][width][3] (needs a colour volume), status uint8
     *  [height][width] (ADC_TSDF_RAY_*); report may be null.  GetTsdfRaycastReport: the report of the last completed call. */
    bool TsdfRaycast(const TsdfRaycastParams* view, float32* depth, float32* normals, uint8* bgr, uint8* status, adc_tsdf_raycast_report* report);
    bool GetTsdfRaycastReport(adc_tsdf_raycast_report* report);
    /** Frame-to-model camera tracking (adc_track_device, point-to-plane ICP whose iterations stay on the device).  Track: DEVICE
     *  addresses -- the frame's float32 [H][W] map, optionally its normals (float32 [H][W][4], may be null), the model's depth and
     *  normals as adc_tsdf_raycast_device wrote them for `model_view`; frame->R, t are the initial guess; params may be null
     *  (defaults); d_result (8-byte aligned, may be null) receives the record on the stream.  Asynchronous: Wait() completes it,
     *  GetTrackResult reads the result of the last completed call.  TsdfTrack: a HOST map against the handle's volume, ray cast from the
     *  frame's guess; synchronous; result may be null.  result->R, t go into the adc_tsdf_frame of the next TsdfIntegrate. */
    bool Track(const void* d_map, const void* d_frame_normals, const adc_tsdf_frame* frame, const TsdfRaycastParams* model_view, const void* d_model_depth,
               const void* d_model_normals, const TrackParams* params, void* d_result);
    bool TsdfTrack(const float32* map, const adc_tsdf_frame* frame, const TrackParams* params, TrackResult* result);
    bool GetTrackResult(TrackResult* result);
    /** Stereo-aware fusion (adc_tsdf_weights / adc_tsdf_fuse): HOST pointers, synchronous.  TsdfWeights turns a map (with optional
     *  provenance and confidence maps of the same Match) into a uint8 [H][W] observation weight per pixel; params may be null (the
     *  defaults), report may be null; it needs no volume.  TsdfFuse is TsdfIntegrate with that weight map (null: 1 everywhere) and an
     *  optional gated bilinear reading of the map (params, may be null).  GetTsdfFuseReport: the reports of the last completed calls,
     *  either may be null. */
    bool TsdfWeights(const float32* map, const uint8* provenance, const float32* confidence, const adc_tsdf_frame* frame, const adc_tsdf_weight_params* params,
                     uint8* weight, adc_tsdf_weight_report* report);
    bool TsdfFuse(const float32* map, const uint8* bgr_left, const uint8* weight, const adc_tsdf_frame* frame, const adc_tsdf_fuse_params* params,
                  adc_tsdf_fuse_report* report);
    bool GetTsdfFuseReport(adc_tsdf_fuse_report* fuse_report, adc_tsdf_weight_report* weight_report);
    /** Moving volume (adc_tsdf_shift: HOST pointers, synchronous).  TsdfShift moves the volume's window by params->shift voxels on the
     *  device -- the origin moves along, so every other call goes on as before -- and writes the first min(points, capacity) surface
     *  points whose voxels leave (the records of TsdfExtract, each handed out at most once over a session); points may be null with
     *  capacity 0, report may be null.  GetTsdfShiftReport: the report of the last completed call.  TsdfGetOffset: the sum of all
     *  shifts in voxels and the origin given to TsdfCreate; either may be null.  TsdfFollowPlan (no object needed): the shift that keeps
     *  a point of the camera frame near the volume's centre for the pose R, t (WORLD -> camera); params holds the CURRENT origin. */
    bool TsdfShift(const adc_tsdf_shift_params* params, adc_point* points, uint64 capacity, adc_tsdf_shift_report* report);
    bool GetTsdfShiftReport(adc_tsdf_shift_report* report);
    bool TsdfGetOffset(sint32 offset[3], float32 origin0[3]);
    static bool TsdfFollowPlan(const adc_tsdf_params* params, const float32 R[9], const float32 t[3], const adc_tsdf_follow_params* follow_params, sint32 shift_out[3]);
    /** Optional voxel-grid filter of the cloud on the device (adc_set_cloud_voxel_grid, include/adcensus_c_api.h holds the definition):
     *  every later cloud of MatchOut / MatchProducts / MatchAsyncProducts holds one point per occupied voxel of edge `leaf` (mean
     *  position and colour, pad = min(points, 255)), in the order of the voxels' first pixels; CloudCount counts voxels.  A cloud then
     *  needs a calibration.  State of the matcher object underneath: needs Initialize, and Initialize / Reset drop it.  false: a refused
     *  grid (leaf not finite or <= 0, z_min > z_max or NaN, a non-finite pose), a Match pending, a HIP failure. */
    bool SetCloudVoxelGrid(const adc_voxel_grid* grid);
    bool ClearCloudVoxelGrid();
    /** Valid points, points kept after crop and range, and voxels of the last voxel cloud completed on this object. */
    bool GetVoxelReport(adc_voxel_report* report) const;
    const char* LastError() const;

private:
    void Release();
    adc_handle* impl_;
    int device_;
    bool verbose_, profiling_;
    unsigned paper_;
    int speckle_size_;
    float speckle_diff_;
    struct RectifySide; // what was set for a side (kept for Initialize / Reset)
    RectifySide* rect_[2];
    sint32 width_, height_;
    bool ApplyRectify(int side);
};
