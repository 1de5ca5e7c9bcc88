/*
 * adcensus_c_api.h -- C ABI of the MI355X-native AD-Census stereo matcher.
 *
 * This is the drop-in boundary underneath the C++ facade `ADCensusStereo`
 * (include/ADCensusStereo.h).  Everything crossing it is plain C: pointers, sizes, PODs.
 * No torch / HIP types appear in any signature (a stream is passed as an opaque void*).
 *
 * Each entry point names the reference interface it replaces
 * (paths are relative to the reference checkout, AD-Census/...):
 *
 *   adc_option            <- struct ADCensusOption            adcensus_types.h:45-75
 *   adc_create            <- ADCensusStereo::Initialize        ADCensusStereo.cpp:21-67
 *   adc_match             <- ADCensusStereo::Match             ADCensusStereo.cpp:69-132
 *   adc_destroy           <- ~ADCensusStereo / Release         ADCensusStereo.cpp:15-19,312-316
 *   (Reset == adc_destroy + adc_create                         ADCensusStereo.cpp:134-144)
 *
 * Additive entry points (no reference counterpart; they do not change Match semantics):
 *   adc_match_device      device-resident in/out buffers (bench: inputs already in HBM)
 *   adc_match_ex /        the same Matches with two optional per-pixel maps next to the disparity:
 *   adc_match_device_ex   provenance (measured or filled, ADC_LR_* / ADC_FILL_*) and confidence
 *   adc_match_out /       the same Matches with outputs computed on the device from the final map: metric depth, a point
 *   adc_match_device_out  cloud in raster order, the min-max normalised 8-bit image; adc_reproject_device: the same from any map
 *   adc_match_async/wait  several objects in flight from one host thread
 *   adc_match_products /  every optional product above from ONE Match through one request struct (adc_products), synchronous,
 *   adc_match_async_products / adc_match_device_products / adc_farm_submit_products   asynchronous, device-resident and through the
 *                         farm; plus a 16-bit fixed-point disparity map (adc_disp16_device: that kernel on any map)
 *   adc_set_register_target / adc_register_depth_device / adc_align_color_device   depth registered into a second camera on the
 *                         device (z-buffered scatter), and that camera's colours gathered into the left view
 *   adc_normals_device /  camera-facing surface normals from any disparity map: a windowed plane fit in disparity space, solved
 *   adc_normals           exactly in integers (float32 x 4 and / or a normal-map image of 4 bytes per pixel)
 *   adc_mesh_device /     a triangle mesh from any disparity map: gated grid cells over a lattice of every step-th pixel, vertices
 *   adc_mesh              as cloud points, triangles as vertex numbers, both compacted in raster order
 *   adc_tsdf_create / adc_tsdf_integrate_device / adc_tsdf_extract_device / ...   a TSDF volume in the handle: the maps of many
 *                         frames fused per voxel in integers, and the volume's surface points in voxel order
 *   adc_tsdf_mesh_device / the volume's surface as a triangle mesh (marching cubes): the surface points as vertices, triangles as
 *   adc_tsdf_mesh         vertex numbers in cell order
 *   adc_tsdf_raycast_device / the volume's surface as seen from a camera pose: depth, normal, colour and status maps of a view, one
 *   adc_tsdf_raycast      ray per pixel marched through the volume
 *   adc_tsdf_weights_device / per-pixel observation weights of a stereo map (fill class, confidence, depth) and the integrate that
 *   adc_tsdf_fuse_device    applies them and may read the map by a gated bilinear interpolation
 *   adc_get_stage_ms      HIP-event stage timers (the reference printf()s stage times,
 *                         ADCensusStereo.cpp:81-129)
 *   adc_debug_*           per-stage entry points used ONLY by the parity tests
 *
 * Image format (cost_computor.cpp:66-68, main.cpp:65-76): tightly packed row-major
 * uint8[H][W][3], channel order B,G,R.  Output: float32[H][W] left-view disparity.
 */
#ifndef ADCENSUS_C_API_H_
#define ADCENSUS_C_API_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Plain-C mirror of ADCensusOption (adcensus_types.h:45-75); same fields, same order,
 * same defaults (adc_option_default).  bools are uint8_t. */
typedef struct adc_option {
    int32_t min_disparity;               /* default 0   */
    int32_t max_disparity;               /* default 64  */
    int32_t lambda_ad;                   /* default 10  */
    int32_t lambda_census;               /* default 30  */
    int32_t cross_L1;                    /* default 34  */
    int32_t cross_L2;                    /* default 17  */
    int32_t cross_t1;                    /* default 20  */
    int32_t cross_t2;                    /* default 6   */
    float   so_p1;                       /* default 1.0 */
    float   so_p2;                       /* default 3.0 */
    int32_t so_tso;                      /* default 15  */
    int32_t irv_ts;                      /* default 20  */
    float   irv_th;                      /* default 0.4 */
    float   lrcheck_thres;               /* default 1.0 */
    uint8_t do_lr_check;                 /* default 1   */
    uint8_t do_filling;                  /* default 1   */
    uint8_t do_discontinuity_adjustment; /* default 0   */
    uint8_t reserved_;
} adc_option;

typedef struct adc_handle adc_handle;

/* Fills *opt with the reference defaults (adcensus_types.h:67-74). */
void adc_option_default(adc_option* opt);

/* Library / device info. Returns number of visible HIP devices (<=0: none / error). */
int adc_device_count(void);
const char* adc_version(void);
/* Last error text of the calling thread ("" if none). */
const char* adc_last_error(void);

/*
 * Initialize.  Returns NULL when the reference's Initialize returns false
 * (width<=0 || height<=0, ADCensusStereo.cpp:31-33; max_disparity-min_disparity<=0, :38-40),
 * on a HIP failure (including out of memory), or when the disparity range exceeds ADC_MAX_DISP_RANGE
 * (2047 = 32 disparities per lane and the 11-bit histogram bins of the voting state map; the reference accepts any positive range
 * its host memory holds -- at 2047 a 1080p cost volume is 17 GB --, larger ones return NULL here).
 * device < 0 means "current device".  All device scratch is allocated here, once.
 */
#define ADC_MAX_DISP_RANGE 2047
adc_handle* adc_create(int32_t width, int32_t height, const adc_option* opt, int device);
void adc_destroy(adc_handle* h);

/*
 * Match (synchronous).  Host pointers.  0 = ok; nonzero = the reference's `false`
 * (any pointer NULL, ADCensusStereo.cpp:74-76) or a HIP error.
 * Does H2D (2 x 3*W*H bytes), the kernels, D2H (4*W*H bytes) on the handle's stream.
 */
int adc_match(adc_handle* h, const uint8_t* bgr_left, const uint8_t* bgr_right, float* disp_left);

/* Same pipeline, device-resident buffers (already in HBM); asynchronous on the handle's stream: the call only ENQUEUES
 * (no host synchronisation anywhere in the pipeline) and returns; call adc_wait() before reading d_disp_left.  The two
 * image buffers are BORROWED until adc_wait returns (not copied: the caller must not overwrite or free them before; after
 * adc_wait the handle holds no pointer to them).  Where the reference would decide something on the
 * host in mid-pipeline, the device decides or verifies: the aggregation uses the ring depth of the previous Match of the
 * handle and checks it on the device; the region voting is a kernel chain driven by a device-side state machine with a
 * launch budget adapted from the previous Match.  adc_wait completes whatever such an assumption left open (redo with
 * the full aggregation ring, continuation of the voting chain) -- slower for that one call, identical results always.
 * To overlap several pairs on one GPU, keep several handles in flight from ONE host thread (bench.py --inflight N,
 * adc_farm_* below). */
int adc_match_device(adc_handle* h, const void* d_bgr_left, const void* d_bgr_right, void* d_disp_left);

/* -------------------------------------------------------------------------------------------
 * Optional per-pixel outputs: which disparities were measured and which were filled, and how distinct the measured minimum is.
 *
 * provenance  uint8 [H][W]:  code = lr | (fill << ADC_PROV_FILL_SHIFT)
 *   lr   (code & ADC_PROV_LR_MASK)   the LR check's outcome (multistep_refiner.cpp:90-151): ADC_LR_CONSISTENT (also: no LR check
 *        made), ADC_LR_MISMATCH (includes a winner-takes-all result of +inf), ADC_LR_OCCLUSION
 *   fill (code >> ADC_PROV_FILL_SHIFT)  where the value came from: ADC_FILL_WTA the pixel's own winner-takes-all disparity (lr ==
 *        0 and that result finite); ADC_FILL_VOTING region voting; ADC_FILL_INTERPOLATION proper interpolation (lr != 0 with
 *        do_filling, voting left it +inf); ADC_FILL_NONE nothing filled it (lr != 0 without do_filling; with do_lr_check = 0 a
 *        winner-takes-all result of +inf, code 12).  The discontinuity adjustment and the median do not change the code.
 * confidence  float32 [H][W]:  0 wherever fill != ADC_FILL_WTA.  Otherwise, over the pixel's scanline-optimised costs C[d]: c1 =
 *   min C, d1 = the lowest d with C[d] == c1 (the winner-takes-all's first minimum), c2 = min { C[d] : |d - d1| >= 2 };
 *   confidence = (c2 - c1) / c2 in f32 (correctly rounded), 0 when c2 == 0, 1 when that set is empty (D == 3, d1 == 1).  In
 *   [0, 1]; 0 = another disparity at least two steps away is just as good.
 *
 * Either map pointer may be NULL; with both NULL the calls are exactly adc_match / adc_match_device.  Return codes are theirs,
 * plus 1 (with adc_last_error) when a map is requested on a handle with paper modes set.  adc_match_ex allocates device scratch
 * for the maps on the first call that needs it (freed by adc_destroy).  adc_match_device_ex writes the caller's device buffers
 * directly and, like adc_match_device, is completed by adc_wait.  adc_match_async_products and adc_farm_submit_products (below) deliver the maps on the asynchronous paths.
 * ------------------------------------------------------------------------------------------- */
#define ADC_LR_CONSISTENT 0
#define ADC_LR_MISMATCH 1
#define ADC_LR_OCCLUSION 2
#define ADC_FILL_WTA 0
#define ADC_FILL_VOTING 1
#define ADC_FILL_INTERPOLATION 2
#define ADC_FILL_NONE 3
#define ADC_PROV_LR_MASK 3
#define ADC_PROV_FILL_SHIFT 2
int adc_match_ex(adc_handle* h, const uint8_t* bgr_left, const uint8_t* bgr_right, float* disp_left, uint8_t* provenance,
                 float* confidence);
int adc_match_device_ex(adc_handle* h, const void* d_bgr_left, const void* d_bgr_right, void* d_disp_left, void* d_provenance,
                        void* d_confidence);

/* -------------------------------------------------------------------------------------------
 * Outputs computed on the device from the final left-view disparity map (behind the median): what the reference's demo derives
 * on the host after every Match (main.cpp:180-230), plus metric depth.  d = the pixel's final disparity, a = |d| (both reference
 * functions take abs first).  All arithmetic is IEEE binary32, one rounding per operation, nothing fused, divisions correctly
 * rounded; tests/outputs_ref.py holds the same definitions in numpy.
 *
 * adc_calib  Middlebury calib.txt convention, Z = baseline * focal_px / (d + doffs).  fb = focal_px * baseline is one f32 multiply.
 * disp8   uint8 [H][W], SaveDisparityMap's image: mn = float(W), mx = -float(W), then min / max of a over the pixels with
 *         a != +inf; pixel = uint8((a - mn) / (mx - mn) * 255) (truncating), 0 where a == +inf, 0 everywhere when !(mx > mn).
 *         Does not look at the calibration.
 * depth   float32 [H][W], needs a calibration: s = a + doffs; valid <=> a finite and s > 0; valid: fb / s, otherwise +inf
 *         (Invalid_Float).
 * cloud   adc_point per valid pixel, in raster order (row by row, then by column: SaveDisparityCloud's rows).  r, g, b from the left
 *         image (stored B,G,R), pad = 0.  Without a calibration: (x, y, z) = (float(x), float(y), a), valid <=> a != +inf -- the
 *         reference's rows.  With one: validity and Z as for depth, X = ((float(x) - cx) * Z) / focal_px, Y = ((float(y) - cy) * Z) /
 *         focal_px (a pixel stays valid where fb / s overflows).  The first min(count, cloud_capacity) points are written and
 *         nothing behind them; W * H points always suffice.  count = valid pixels, whatever the capacity: adc_get_cloud_count
 *         after adc_wait, and -- when cloud_count is given -- a uint32 at that device address, written on the stream (a GPU
 *         consumer need not synchronise).  cloud_capacity = 0 with a non-NULL cloud counts only.
 *
 * Any output pointer may be NULL (cloud_count is looked at only with a cloud); with a NULL request or none of depth / cloud /
 * disp8 the Match calls are exactly adc_match / adc_match_device.  Refused with 1 and adc_last_error, before anything is
 * enqueued: depth without a calibration; a calibration with focal_px <= 0 or a non-finite field; a device cloud address that is
 * not 16-byte aligned.  Paper modes do not matter.  Otherwise the return codes are those of adc_match / adc_match_device.
 *
 * adc_match_device_out  asynchronous, completed by adc_wait; the pointers of the request are DEVICE addresses, written directly;
 *                       the borrow rules of adc_match_device (the request struct itself is read before the call returns).
 * adc_match_out         synchronous, HOST pointers; device scratch is allocated on the first call that needs it (freed by
 *                       adc_destroy); copies out min(count, capacity) points; cloud_count is a host uint32 here.
 * adc_reproject_device  the same kernels on any device-resident float32 [H][W] map of the handle's geometry, without a Match
 *                       (d_bgr_left is needed for a cloud only); completed by adc_wait.  Refused while a Match with outputs is
 *                       pending.  A caller of adc_match_device_ex gets depth and points this way.
 * Every redo adc_wait can take rewrites the outputs from the map it delivers.  adc_match_async_products and
 * adc_farm_submit_products (below) deliver them on the asynchronous paths.
 * ------------------------------------------------------------------------------------------- */
typedef struct adc_calib {
    float focal_px, baseline, cx, cy, doffs;
} adc_calib;
typedef struct adc_point {
    float x, y, z;
    uint8_t r, g, b, pad;
} adc_point; /* 16 bytes */
typedef struct adc_outputs {
    const adc_calib* calib; /* NULL: no calibration */
    float* depth;
    adc_point* cloud;
    uint64_t cloud_capacity; /* points */
    uint32_t* cloud_count;
    uint8_t* disp8;
} adc_outputs;
int adc_match_out(adc_handle* h, const uint8_t* bgr_left, const uint8_t* bgr_right, float* disp_left, const adc_outputs* out);
int adc_match_device_out(adc_handle* h, const void* d_bgr_left, const void* d_bgr_right, void* d_disp_left, const adc_outputs* out);
int adc_reproject_device(adc_handle* h, const void* d_disp, const void* d_bgr_left, const adc_outputs* out);
/* Valid pixels of the last cloud request on this handle that adc_wait (or adc_match_out) has completed. */
int adc_get_cloud_count(adc_handle* h, uint64_t* count);

/* -------------------------------------------------------------------------------------------
 * Optional speckle filter on the device: drops the small islands of the final left-view map (OpenCV's filterSpeckles, the
 * speckleWindowSize / speckleRange pair of StereoBM / SGBM), behind the median and in front of the copy of the map to the caller
 * and of the outputs above -- depth, cloud and disp8 of a filtered Match come from the filtered map.  OFF by default: without a
 * call of adc_set_speckle_filter every Match is exactly what it was.  tests/speckle_ref.py holds the definition in numpy:
 *
 *   valid      a pixel whose value is finite (+inf is Invalid_Float; NaN and -inf of a caller's own map are invalid too and are
 *              left untouched)
 *   joined     two 4-neighbours p, q, both valid, with fabsf(d[p] - d[q]) <= max_diff (one binary32 subtraction; signs kept)
 *   component  a class of the transitive closure of "joined" (a smooth ramp is ONE component however far its ends are apart)
 *   label      int32: raster index y * W + x of the component's first pixel in raster order; -1 at invalid pixels
 *   filter     every pixel of a component of size <= max_size becomes +inf; everything else keeps its bits
 *   stats      components, removed components, removed pixels (uint32 each)
 * Integer logic over one exact float comparison: results are defined bit for bit.
 *
 * adc_set_speckle_filter      handle state, like adc_set_paper_modes: every later Match through every entry point (adc_match,
 *                             _async, _device, _ex, _device_ex, _out, _device_out) delivers the filtered map, also behind every
 *                             redo adc_wait can take.  max_size <= 0 switches the filter off again.  Device scratch (12 bytes per
 *                             pixel) is allocated by the first call that switches it on and freed by adc_destroy.  With the filter
 *                             on, adc_match_ex / adc_match_device_ex set ADC_PROV_SPECKLE in the provenance code of the pixels
 *                             the filter removed (confidence is left as computed).  Paper modes do not matter.
 * adc_filter_speckles_device  the same kernels on any device-resident float32 [H][W] map of the handle's geometry, IN PLACE,
 *                             asynchronous on the handle's stream, completed by adc_wait (the counterpart of
 *                             adc_reproject_device).  d_labels: int32 [H][W] device buffer for the labels, or NULL.  max_size <= 0
 *                             with d_labels labels without filtering (without d_labels: nothing to do, 0).
 * adc_get_speckle_stats       of the last filtered Match / filter call that adc_wait has completed; any pointer may be NULL.
 * adc_farm_set_speckle_filter all pipelines of a farm.
 * Return codes: 0; 1 with adc_last_error and nothing enqueued or changed (NULL handle / map, max_diff negative or not finite,
 * the setters while a Match / a pair is in flight); 2 on a HIP failure.
 * ------------------------------------------------------------------------------------------- */
#define ADC_PROV_SPECKLE (0x10) /* above the four bits of lr and fill */
int adc_set_speckle_filter(adc_handle* h, int32_t max_size, float max_diff);
int adc_filter_speckles_device(adc_handle* h, void* d_disp_inout, int32_t max_size, float max_diff, void* d_labels);
int adc_get_speckle_stats(adc_handle* h, uint32_t* components, uint32_t* removed_components, uint32_t* removed_pixels);

/* -------------------------------------------------------------------------------------------
 * Optional voxel-grid filter of the cloud on the device (k_voxel.hip), in front of the cloud's compaction: one adc_point per occupied
 * voxel instead of one per valid pixel (PCL's VoxelGrid with integer means).  OFF by default: without a call of
 * adc_set_cloud_voxel_grid every cloud is exactly what it was (same kernels, same launches, pad = 0).  tests/voxel_ref.py holds the
 * definition in numpy; all float arithmetic is IEEE binary32, one rounding per operation, nothing fused, divisions correctly rounded.
 *
 *   parameters leaf (finite, > 0, in the unit of the calibration's baseline); z_min <= z_max (not NaN; z_max may be +inf); flags
 *              (ADC_VOXEL_POSE); R row-major and t, looked at only with the flag and finite then; reserved words, all 0.
 *              inv = 1.0f / leaf is computed once on the host.
 *   point      validity and (X, Y, Z) of a pixel are exactly those of adc_outputs.cloud WITH a calibration; the colour is the left
 *              image's.  A cloud request without a calibration while a grid is set is refused with 1.
 *   crop       a pixel is kept iff z_min <= Z && Z <= z_max (the camera-frame Z, before any pose)
 *   pose       with the flag Xw = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0], rows 1 and 2 likewise; without it Xw = X, ...
 *   voxel      per axis u = Xw * inv; in range iff fabsf(u) < 1048576.0f (NaN fails; a point out of range on any axis is dropped);
 *              i = floorf(u); f = u - i (one rounding: exactly 1.0f for a tiny negative u); q = min((uint32_t)(f * 65536.0f), 65535)
 *              key = (uint64)(ix + 2^20) << 42 | (uint64)(iy + 2^20) << 21 | (uint64)(iz + 2^20)
 *   aggregate  over the kept points of a voxel: n, the sums of q per axis, the sums of r, g, b, and leader = the lowest raster
 *              index y * W + x among them.  Every sum is an integer (64 bits): the order of arrival cannot matter.
 *   record     mq = (Sq + n / 2) / n in integers; x = ((float)ix + (float)mq * 0x1p-16f) * leaf (the inner product is exact: two
 *              roundings), y and z likewise; r, g, b = (S + n / 2) / n; pad = min(n, 255)
 *   order      voxels in ascending order of leader (the raster order of their first pixels).  count = voxels, whatever the capacity;
 *              the first min(count, cloud_capacity) records are written and nothing behind them.  cloud_count and
 *              adc_get_cloud_count report voxels.
 *   report     adc_voxel_report: points_valid (cloud-valid pixels), points_kept (after crop and range), voxels
 *
 * adc_set_cloud_voxel_grid      handle state, like the speckle filter: every later cloud through every entry point (adc_match_out,
 *                               _device_out, adc_reproject_device, adc_match_products, _async_products, _device_products,
 *                               adc_farm_submit_products) is the voxel cloud, also behind every redo adc_wait can take.  Depth and
 *                               disp8 are not touched.  Device scratch (a hash table of 64-byte slots, the smallest power of two
 *                               >= 2 * W * H of them, and 4 bytes per pixel) is allocated by the first call and freed by adc_destroy.
 *                               The struct is read before the call returns.
 * adc_clear_cloud_voxel_grid    every later cloud is the plain cloud again.
 * adc_get_voxel_report          of the last voxel cloud that adc_wait or a synchronous call has completed on this handle.
 * adc_farm_set_cloud_voxel_grid all pipelines of a farm; a NULL grid clears it.
 * Return codes: 0; 1 with adc_last_error and nothing changed (NULL handle / grid / report, a bad parameter, the setters while a
 * Match / a pair is in flight); 2 on a HIP failure (the grid is then unset, the handle stays usable).
 * ------------------------------------------------------------------------------------------- */
#define ADC_VOXEL_POSE (0x1u) /* R, t take the camera-frame point into the frame of the grid */
typedef struct adc_voxel_grid {
    float leaf;
    float z_min, z_max;
    uint32_t flags;
    float R[9];
    float t[3];
    uint32_t reserved[4]; /* 0 */
} adc_voxel_grid; /* 80 bytes */
typedef struct adc_voxel_report {
    uint32_t points_valid, points_kept, voxels;
} adc_voxel_report;
int adc_set_cloud_voxel_grid(adc_handle* h, const adc_voxel_grid* grid);
int adc_clear_cloud_voxel_grid(adc_handle* h);
int adc_get_voxel_report(adc_handle* h, adc_voxel_report* out);

/* Host buffers, asynchronous (pinned staging inside the handle); adc_wait() completes it and
 * copies the result to disp_left given here. */
int adc_match_async(adc_handle* h, const uint8_t* bgr_left, const uint8_t* bgr_right, float* disp_left);
int adc_wait(adc_handle* h);

/* Opt-in for host callers that keep their buffers alive: page-lock a host range (hipHostRegister) and tell the library.
 * Images / disparity maps passed to adc_match / adc_match_async / adc_farm_submit that lie inside a registered range are
 * then transferred by DMA straight from / to the caller's memory -- no pinned staging copies (2 x 6.2 MB in, 8.3 MB out
 * per 1080p pair).  INPUT images are read in place only by the synchronous adc_match (which returns after the copy);
 * adc_match_async and adc_farm_submit keep their contract "the images may be reused as soon as the call returns" and still
 * stage them.  A registered OUTPUT map is written in place by every entry point (it belongs to the library until adc_wait /
 * adc_farm_wait has delivered it).  The caller must adc_host_unregister(ptr) BEFORE freeing the memory.  Process-wide, thread-safe.
 * 0 ok, 1 bad argument / unknown pointer, 2 HIP failure. */
int adc_host_register(void* ptr, size_t bytes);
int adc_host_unregister(void* ptr);

/* -------------------------------------------------------------------------------------------
 * Pair farm: a persistent set of `pipelines` matcher objects of one geometry on one device, each
 * with its own stream and pinned staging buffers (the ring), fed round-robin.  adc_farm_submit copies the pair into the
 * next pipeline's pinned slot and enqueues the whole Match asynchronously -- it blocks only when that pipeline is still
 * busy with an earlier pair, and then exactly until that pair is done and delivered.  Results arrive in the caller's
 * `disp_left` buffers in submission order; adc_farm_wait(ticket) / adc_farm_drain complete them.  Match semantics are
 * those of adc_match (same values, same error codes); the caller's image buffers may be reused as soon as submit returns.
 * ------------------------------------------------------------------------------------------- */
typedef struct adc_farm adc_farm;
adc_farm* adc_farm_create(int32_t width, int32_t height, const adc_option* opt, int device, int pipelines);
void adc_farm_destroy(adc_farm* f);
/* Returns 0 and the ticket (1, 2, 3, ...) of the pair; 1 on bad arguments, 2 on a HIP failure (nothing enqueued);
 * ADC_FARM_PREVIOUS_FAILED when the pair that occupied the pipeline before (ticket - pipelines) failed while it was
 * collected: the NEW pair was enqueued all the same and *ticket is valid; adc_last_error() names the failed ticket. */
#define ADC_FARM_PREVIOUS_FAILED 3
int adc_farm_submit(adc_farm* f, const uint8_t* bgr_left, const uint8_t* bgr_right, float* disp_left, uint64_t* ticket);
/* Blocks until the pair with this ticket (and every earlier pair of its pipeline) has been delivered. */
int adc_farm_wait(adc_farm* f, uint64_t ticket);
/* Completes everything submitted so far; returns the number of pairs delivered since creation, negative on failure. */
int64_t adc_farm_drain(adc_farm* f);
/* adc_set_speckle_filter on every pipeline of the farm (above); 1 while a pair is in flight (adc_farm_drain first). */
int adc_farm_set_speckle_filter(adc_farm* f, int32_t max_size, float max_diff);
/* adc_set_cloud_voxel_grid on every pipeline of the farm (above), NULL: adc_clear_cloud_voxel_grid; 1 while a pair is in flight. */
int adc_farm_set_cloud_voxel_grid(adc_farm* f, const adc_voxel_grid* grid);

/* -------------------------------------------------------------------------------------------
 * Optional rectification of raw camera images on the device (k_rectify.hip), off by default.  Handle state like the speckle filter:
 * once BOTH sides are set, EVERY match entry point (adc_match, _async, _device, _ex, _device_ex, _out, _device_out,
 * adc_farm_submit) takes its left / right arguments as RAW source images of the declared geometry -- height * pitch_bytes bytes each,
 * host or device like the entry point's images were -- remaps each into the handle's own W x H BGR buffers and matches those.
 * Everything downstream (the map, depth, cloud colours, 8-bit image, speckle filter, every redo of adc_wait) sees the rectified
 * pair.  With exactly one side set a Match is refused (1).  A handle that never had a side set does exactly what it did before.
 *
 * The remap, per destination pixel, from float32 maps map_x / map_y [H][W] (source coordinates, as cv::initUndistortRectifyMap
 * produces them): outside (B = G = R = 0, valid = 0) when !(fabsf(mx) < 32768) or !(fabsf(my) < 32768), NaN and +-inf included;
 * otherwise X = (int)rintf(mx * 32), xi = X >> 5, ax = X & 31, Y / yi / ay likewise; taps (yi, xi), (yi, xi+1), (yi+1, xi), (yi+1, xi+1)
 * with the integer weights (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax*ay; a tap outside the source contributes 0 (constant border);
 * out = (sum of w * p + 512) >> 10 per channel; valid = 1 iff every tap with a nonzero weight is inside.  Integer arithmetic behind
 * the two float operations: tests/rectify_ref.py is the definition, the kernels match it bit for bit.  By construction these are the
 * weights of cv::remap with INTER_LINEAR and BORDER_CONSTANT (INTER_BITS = 5).
 *
 * adc_set_rectify_model computes the maps on the device from one camera: xn = (u - new_cx) / new_fx, yn = (v - new_cy) / new_fy;
 * (X, Y, Wc) = R^T (xn, yn, 1); x = X / Wc, y = Y / Wc; r2 = x*x + y*y; rad = 1 + r2 (k1 + r2 (k2 + r2 k3));
 * xd = (x rad + (2 p1) x y) + p2 (r2 + 2 x*x); yd = (y rad + p1 (r2 + 2 y*y)) + (2 p2) x y; mx = fx xd + cx, my = fy yd + cy --
 * float32, one rounding per operation, in that order (Brown-Conrady, R the rectifying rotation, row-major).  Deriving R and the new
 * intrinsics from a stereo calibration is the caller's business.
 *
 * Set calls return 0; 1 for a NULL argument, a bad side or format, width / height outside [1, 32767], pitch_bytes < width * bytes per
 * pixel, an image larger than 2^31 - 1 bytes, a parity rule of the layout (below) broken, a model with a non-finite value or fx, fy, new_fx, new_fy == 0, or a Match pending
 * (adc_wait first); 2 for a HIP failure (that side is then unset, the handle stays usable).  Synchronous.  The first set call
 * allocates the feature's buffers (adc_create allocates none of them); adc_destroy frees them.
 * ------------------------------------------------------------------------------------------- */
#define ADC_PIX_BGR8 0   /* 3 bytes per pixel: B, G, R */
#define ADC_PIX_RGB8 1   /* 3 bytes per pixel: R, G, B */
#define ADC_PIX_GRAY8 2  /* 1 byte per pixel: B = G = R */
#define ADC_PIX_BGRA8 3  /* 4 bytes per pixel: B, G, R, alpha (ignored) */
/* Camera layouts (codes 4..15 stay invalid).  Each is DECODED to the virtual 8-bit B, G, R source image V the remap takes its taps
 * from; the tap weights, the rounding, the constant border and the valid map are those above.  All integer, >> arithmetic:
 *   16-bit samples  little-endian; s = min(255, v >> (bits - 8)), bits = the significant bits given with ADC_PIX_BITS (9..16, 0 = 16);
 *                   everything below works on s.  pitch_bytes must be even, a device address of such an image must be even
 *   GRAY16          B = G = R = s
 *   BAYER_*         the four letters are the colours of pixels (0,0), (0,1), (1,0), (1,1); width, height >= 2.  Bilinear: S(y, x) is
 *                   the sample at coordinates reflected into the image without repeating the edge (-1 -> 1, n -> n - 2).  Red / blue
 *                   site: own colour S(y,x), green (S(y-1,x) + S(y+1,x) + S(y,x-1) + S(y,x+1) + 2) >> 2, the other colour the same of
 *                   the four diagonal neighbours.  Green site: green S(y,x), the colour of the left / right neighbours
 *                   (S(y,x-1) + S(y,x+1) + 1) >> 1, of the upper / lower neighbours (S(y-1,x) + S(y+1,x) + 1) >> 1.  The reflection
 *                   belongs to the decode of a tap INSIDE the source; a tap outside still contributes 0
 *   YUYV, UYVY      row bytes Y0 U Y1 V / U Y0 V Y1 per pixel pair, width even.  BT.601 limited range, the pair's own chroma:
 *                   c = Y - 16, d = U - 128, e = V - 128; R = clip8((298c + 409e + 128) >> 8),
 *                   G = clip8((298c - 100d - 208e + 128) >> 8), B = clip8((298c + 516d + 128) >> 8)
 *   NV12            luma plane [height][pitch_bytes], at byte offset height * pitch_bytes the chroma plane [height / 2][pitch_bytes]
 *                   of U, V pairs: pixel (y, x) reads U = C[y >> 1][2 * (x >> 1)] and V behind it; width and height even; the image
 *                   is height * pitch_bytes * 3 / 2 bytes (that product is what must stay <= 2^31 - 1).  Same matrix as YUYV */
#define ADC_PIX_GRAY16 0x10       /* 2 bytes per pixel */
#define ADC_PIX_BAYER_RGGB8 0x20  /* 1 byte per pixel */
#define ADC_PIX_BAYER_GRBG8 0x21
#define ADC_PIX_BAYER_GBRG8 0x22
#define ADC_PIX_BAYER_BGGR8 0x23
#define ADC_PIX_BAYER_RGGB16 0x30 /* 2 bytes per pixel */
#define ADC_PIX_BAYER_GRBG16 0x31
#define ADC_PIX_BAYER_GBRG16 0x32
#define ADC_PIX_BAYER_BGGR16 0x33
#define ADC_PIX_YUYV 0x40         /* 2 bytes per pixel */
#define ADC_PIX_UYVY 0x41         /* 2 bytes per pixel */
#define ADC_PIX_NV12 0x42         /* 1 byte per pixel of luma (pitch_bytes >= width), plus the chroma plane */
/* the format word of a 16-bit layout with its significant bits (9..16; 0 = 16); any nonzero value on an 8-bit layout is refused */
#define ADC_PIX_BITS(fmt, bits) ((fmt) | ((bits) << 8))
#define ADC_SIDE_LEFT 0
#define ADC_SIDE_RIGHT 1
typedef struct adc_raw_format { int32_t width, height, pitch_bytes, format; } adc_raw_format;
typedef struct adc_camera_model {
    float fx, fy, cx, cy;          /* intrinsics of the raw camera */
    float k1, k2, p1, p2, k3;      /* Brown-Conrady distortion */
    float R[9];                    /* rectifying rotation, row-major */
    float new_fx, new_fy, new_cx, new_cy; /* intrinsics of the rectified W x H image */
} adc_camera_model;
/* map_x / map_y: host float32 [H][W] (H, W of adc_create); they may hold anything, NaN and inf included. */
int adc_set_rectify_maps(adc_handle* h, int side, const adc_raw_format* raw, const float* map_x, const float* map_y);
int adc_set_rectify_model(adc_handle* h, int side, const adc_raw_format* raw, const adc_camera_model* model);
/* Both sides unset: the entry points take rectified W x H BGR images again.  1: NULL handle or a Match pending. */
int adc_clear_rectify(adc_handle* h);
/* The float maps in use for a side (the caller's, or the model's) and the valid map, to host buffers [H][W]; any may be NULL.
 * Synchronous.  1: NULL handle, bad side, side not set; 2: HIP failure. */
int adc_get_rectify_maps(adc_handle* h, int side, float* map_x, float* map_y, uint8_t* valid);
/* The remap alone: device-resident raw image of the side's geometry -> device-resident [H][W][3] BGR.  Asynchronous on the handle's
 * stream (adc_wait completes it); both buffers are the caller's.  1: NULL argument, bad side, side not set; 2: HIP failure. */
int adc_rectify_device(adc_handle* h, int side, const void* d_raw, void* d_bgr_out);
/* The same setters on every pipeline of a farm; 1 while a pair is in flight (adc_farm_drain first). */
int adc_farm_set_rectify_maps(adc_farm* f, int side, const adc_raw_format* raw, const float* map_x, const float* map_y);
int adc_farm_set_rectify_model(adc_farm* f, int side, const adc_raw_format* raw, const adc_camera_model* model);
int adc_farm_clear_rectify(adc_farm* f);
/* Conversion only, for cameras whose frames are already rectified: declares the frames of one side as `raw` (any ADC_PIX_* layout;
 * raw->width / height must be the handle's W / H) without maps.  It sets the side like the two calls above (any mix of the three
 * works, each side has its own layout); for such a side the handle's image is the decoded V itself -- bit for bit what the remap
 * delivers under the identity map -- computed by a kernel that reads no map records and writes no valid map.  adc_rectify_device on
 * such a side runs the conversion alone, adc_get_rectify_maps returns 1 (there are no maps), adc_clear_rectify unsets it.  Returns as
 * the set calls above; 1 also for a geometry other than the handle's. */
int adc_set_input_format(adc_handle* h, int side, const adc_raw_format* raw);
int adc_farm_set_input_format(adc_farm* f, int side, const adc_raw_format* raw);

/* -------------------------------------------------------------------------------------------
 * Optional evaluation of a disparity map against ground truth on the device (k_eval.hip): Middlebury's evaldisp figures -- bad-pixel
 * counts, error sums, all pixels and non-occluded pixels -- split by the provenance classes and binned by the confidence of
 * adc_match_ex.  Off by default: a handle that never gets ground truth does exactly what it did before.  Every result is an integer;
 * tests/eval_ref.py holds the same definition in numpy and the kernels match it bit for bit.  All float arithmetic is IEEE binary32,
 * one rounding per operation, nothing fused, divisions correctly rounded.
 *
 * Ground truth g [H][W] of a side, from the caller's array (adc_gt: address, format, row pitch in bytes, scale):
 *   ADC_GT_U8 / ADC_GT_U16  value v == 0: unknown; otherwise g = float(v) / scale (the Middlebury PNG convention: scale 4 for Cone,
 *                           2 for Cloth3 and Wood2; ADC_GT_U16 with scale 256 is KITTI's encoding)
 *   ADC_GT_F32              g = v / scale (PFM ground truth, scale 1)
 *   In every format a quotient that is not finite (a v that is NaN or +-inf, an overflow) is unknown.  Unknown is stored as +inf.
 *   scale must be finite and > 0, pitch_bytes >= W * bytes per value (0: tightly packed), H * pitch_bytes <= 2^31 - 1.
 * Occlusion is defined only with right-view ground truth gr or a caller mask:
 *   with gr:    a known pixel (x, y) is non-occluded iff r = rintf(g) (ties to even) has |r| <= 2^30, xr = x - (int)r lies in [0, W),
 *               gr[y][xr] is known and fabsf(gr[y][xr] - g) <= occ_thres
 *   otherwise:  a caller-given uint8 [H][W] mask (tightly packed), nonzero = non-occluded
 *   masks:      all = known; nonocc = known and non-occluded (empty when neither source is present)
 * Per pixel, with d the evaluated map (signed, not |d|): valid = d finite; for a known and valid pixel e = fabsf(d - g) and
 *   eq = (uint32)rintf(fminf(e, 2048.0f) * 1024.0f)   (1/1024 pixel, clamped at 2048 pixels: the product is exact, rintf is the only
 *   rounding, and the means agree with float arithmetic to four digits)
 * Report (adc_eval_report; uint64 counters):
 *   all, nonocc     pixels of the mask; invalid = those with !valid; bad[k] = valid ones with e > thresholds[k] (a float compare on e,
 *                   e == t is not bad; unused k: 0); sum_err_q = sum of eq and sum_sq_err_q = sum of eq * eq (modulo 2^64) over the
 *                   valid ones; err_hist[min(eq >> 8, 255)] (bins of 1/4 pixel, the last one open) over the valid ones
 *   by_fill[f]      pixels, invalid, bad[k], sum_err_q as above over the `all` mask, for the pixels whose provenance code has
 *                   fill = (code >> ADC_PROV_FILL_SHIFT) & 3 equal to f (ADC_FILL_*); all zero without a provenance map.  A pixel
 *                   with ADC_PROV_SPECKLE stays in its fill class and also counts in speckle_removed_known (if known)
 *   conf_pixels[b], conf_bad[b]   over the pixels that are known, valid and fill == ADC_FILL_WTA: c = confidence * 256.0f,
 *                   b = 0 when !(c >= 0), 255 when c >= 255, otherwise (int)c; conf_bad counts e > thresholds[0].  All zero unless
 *                   BOTH a provenance and a confidence map are given
 *   and an echo: the thresholds, occ_thres, which inputs were present
 * Per-pixel outputs, both optional:
 *   err    float32 [H][W]: e, +inf where unknown or !valid
 *   class  uint8 [H][W]: ADC_EVAL_KNOWN | ADC_EVAL_VALID (d finite, known or not) | ADC_EVAL_BAD (known, valid, e > thresholds[0]) |
 *          ADC_EVAL_OCCLUDED (known, occlusion defined, not non-occluded)
 * Rates, mean (sum_err_q / 1024 / valid pixels), RMS and the sparsification curve of the confidence are the caller's arithmetic on these
 * integers (adcensus_amd/evaluation.py: summarize; the CLI's table); they are not part of the ABI.
 *
 * adc_set_ground_truth   HOST pointers, synchronous: uploads, decodes, builds the occlusion byte map.  right may be NULL, nonocc may be
 *                        NULL (right wins when both are given); occ_thres finite and >= 0 (Middlebury: 1.0).  The first call on a
 *                        handle allocates the feature's device buffers (adc_create allocates none of them), adc_destroy frees them.
 * adc_clear_ground_truth back to "no ground truth" (the buffers stay until adc_destroy).
 * adc_evaluate_device    scores any device-resident float32 [H][W] map of the handle's geometry; d_provenance (uint8 [H][W]),
 *                        d_confidence (float32 [H][W]), d_err, d_class are device addresses or NULL; params NULL = one threshold, 1.0.
 *                        Asynchronous on the handle's stream, completed by adc_wait (the report travels through a pinned read-back
 *                        behind the kernel).  REFUSED while a Match is pending: a redo of adc_wait would rewrite the map behind the
 *                        evaluation (adc_wait first).
 * adc_evaluate           the same with HOST pointers, synchronous; device scratch is allocated on the first call that needs it (freed
 *                        by adc_destroy); out may be NULL.
 * adc_get_eval_report    the report of the last evaluation that adc_wait (or adc_evaluate) has completed.
 * Return codes: 0; 1 with adc_last_error and nothing enqueued or changed (NULL handle / map / left ground truth, an unknown format, a
 * bad scale, occ_thres or pitch, more than ADC_EVAL_MAX_THRESHOLDS thresholds, a threshold negative or not finite, a confidence map
 * without a provenance map, no ground truth set, a Match pending); 2 on a HIP failure (a failed set call leaves ground truth unset,
 * the handle stays usable).  The farm has no evaluation entry point: ground truth differs per pair (every other product goes
 * through adc_farm_submit_products).
 * ------------------------------------------------------------------------------------------- */
#define ADC_GT_U8 0
#define ADC_GT_U16 1
#define ADC_GT_F32 2
#define ADC_EVAL_MAX_THRESHOLDS 4
#define ADC_EVAL_ERR_BINS 256
#define ADC_EVAL_CONF_BINS 256
#define ADC_EVAL_KNOWN 1
#define ADC_EVAL_VALID 2
#define ADC_EVAL_BAD 4
#define ADC_EVAL_OCCLUDED 8
typedef struct adc_gt {
    const void* data;
    int32_t format;      /* ADC_GT_* */
    int32_t pitch_bytes; /* 0: tightly packed rows */
    float scale;
    int32_t reserved_;
} adc_gt;
typedef struct adc_eval_params {
    int32_t n_thresholds; /* 0 .. ADC_EVAL_MAX_THRESHOLDS */
    float thresholds[ADC_EVAL_MAX_THRESHOLDS];
} adc_eval_params;
typedef struct adc_eval_mask_stats {
    uint64_t pixels, invalid, bad[ADC_EVAL_MAX_THRESHOLDS], sum_err_q, sum_sq_err_q;
    uint64_t err_hist[ADC_EVAL_ERR_BINS];
} adc_eval_mask_stats;
typedef struct adc_eval_fill_stats {
    uint64_t pixels, invalid, bad[ADC_EVAL_MAX_THRESHOLDS], sum_err_q;
} adc_eval_fill_stats;
typedef struct adc_eval_report {
    adc_eval_mask_stats all, nonocc;
    adc_eval_fill_stats by_fill[4]; /* ADC_FILL_WTA, _VOTING, _INTERPOLATION, _NONE */
    uint64_t speckle_removed_known;
    uint64_t conf_pixels[ADC_EVAL_CONF_BINS], conf_bad[ADC_EVAL_CONF_BINS];
    /* echo of the request */
    float thresholds[ADC_EVAL_MAX_THRESHOLDS];
    int32_t n_thresholds;
    float occ_thres;
    uint8_t has_right_gt, has_nonocc_mask, has_provenance, has_confidence;
    int32_t reserved_;
} adc_eval_report;
int adc_set_ground_truth(adc_handle* h, const adc_gt* left, const adc_gt* right, const uint8_t* nonocc, float occ_thres);
int adc_clear_ground_truth(adc_handle* h);
int adc_evaluate_device(adc_handle* h, const void* d_disp, const void* d_provenance, const void* d_confidence,
                        const adc_eval_params* params, void* d_err, void* d_class);
int adc_evaluate(adc_handle* h, const float* disp, const uint8_t* provenance, const float* confidence, const adc_eval_params* params,
                 float* err, uint8_t* eval_class, adc_eval_report* out);
int adc_get_eval_report(adc_handle* h, adc_eval_report* out);

/* -------------------------------------------------------------------------------------------
 * Every optional product of a Match through ONE request, on every path: synchronous, asynchronous, device-resident, pair farm.
 *
 * adc_products  provenance / confidence as in adc_match_ex, an embedded adc_outputs (calib, depth, cloud, cloud_capacity,
 *               cloud_count, disp8) with the meaning of adc_match_out, and
 * disp16        uint16 [H][W], the delivered map in 16-bit fixed point (k_outputs.hip: k_disp16; tests/products_ref.py holds the
 *               definition in numpy, all binary32): a = fabsf(d); a not finite (+inf, -inf, NaN) -> 0; otherwise p = a * disp16_scale
 *               (one rounding), q = fminf(fmaxf(p, 1.0f), 65535.0f), pixel = (uint16_t)q (truncating).  0 means "invalid" and nothing
 *               else: a valid disparity of exactly 0 becomes 1, products above 65535 saturate.  It is the inverse of the ADC_GT_U16
 *               decode (g = v / scale, 0 unknown): a map written with scale 256 can be scored as KITTI-encoded ground truth, and
 *               wherever 1 < q < 65535 it decodes back within 1 / scale.  2 bytes per pixel instead of 4 on the way to the host.
 *
 * Any product pointer may be NULL.  A NULL request, or one that asks for nothing, makes each call exactly its plain entry point
 * (adc_match, adc_match_async, adc_match_device, adc_farm_submit).  The request struct and *calib are read before the call returns.
 * All products describe the DELIVERED map: with the speckle filter on they come from the filtered map and ADC_PROV_SPECKLE is set,
 * with rectification / an input format on the cloud colours come from the rectified left image, and every redo adc_wait can take
 * rewrites them.
 *
 * adc_match_products         HOST pointers, synchronous.
 * adc_match_async_products   HOST pointers, only enqueues; adc_wait completes it and delivers every product.  The images may be reused
 *                            as soon as the call returns; the product buffers belong to the library until adc_wait returns.  Each
 *                            product travels device -> pinned staging on the stream (allocated by the first call that needs it,
 *                            freed by adc_destroy) and is copied to the caller by adc_wait; a destination inside an
 *                            adc_host_register'ed range is written in place.  The cloud is copied by adc_wait once the count is
 *                            known: min(count, capacity) points and nothing behind them; cloud_count is a host uint32 here.
 * adc_match_device_products  DEVICE addresses, written directly; completed by adc_wait; the borrow rules of adc_match_device.
 * adc_farm_submit_products   adc_farm_submit with a request: ordered delivery by adc_farm_wait, adc_farm_drain or the next submit on
 *                            the pipeline, the same return codes (ADC_FARM_PREVIOUS_FAILED included).  With a cloud, cloud_count (a
 *                            host uint32, written at delivery) is required: the farm has no per-ticket getter.
 * adc_disp16_device          the disp16 kernel alone on any device-resident float32 [H][W] map of the handle's geometry; asynchronous
 *                            on the handle's stream, completed by adc_wait (the counterpart of adc_reproject_device).
 * Refused with 1 and adc_last_error, nothing enqueued, the handle stays usable: everything adc_match_ex and adc_match_out refuse
 * (maps with paper modes set, depth without a calibration, a bad calibration, an unaligned device cloud address), a disp16 request
 * whose disp16_scale is not finite or <= 0, an odd device address for disp16, a farm cloud without cloud_count, a products call
 * while a Match is pending on the handle (adc_wait first).  2 on a HIP failure.
 * ------------------------------------------------------------------------------------------- */
typedef struct adc_products {
    uint8_t* provenance; /* uint8 [H][W] or NULL */
    float* confidence;   /* float32 [H][W] or NULL */
    adc_outputs out;     /* depth / cloud / disp8, as in adc_match_out */
    uint16_t* disp16;    /* uint16 [H][W] or NULL */
    float disp16_scale;  /* looked at only with disp16: finite and > 0 (256: KITTI's encoding) */
    uint32_t reserved_;
} adc_products;
int adc_match_products(adc_handle* h, const uint8_t* bgr_left, const uint8_t* bgr_right, float* disp_left, const adc_products* products);
int adc_match_async_products(adc_handle* h, const uint8_t* bgr_left, const uint8_t* bgr_right, float* disp_left, const adc_products* products);
int adc_match_device_products(adc_handle* h, const void* d_bgr_left, const void* d_bgr_right, void* d_disp_left, const adc_products* products);
int adc_farm_submit_products(adc_farm* f, const uint8_t* bgr_left, const uint8_t* bgr_right, float* disp_left, const adc_products* products,
                             uint64_t* ticket);
int adc_disp16_device(adc_handle* h, const void* d_disp, float scale, void* d_disp16);

/* -------------------------------------------------------------------------------------------
 * Registration of depth into a second camera on the device ("align depth to colour"; k_register.hip, the arithmetic is
 * adcensus_amd/csrc/reg_project.h, tests/register_ref.py holds the same definition in numpy and the kernels match it bit for bit).
 * All arithmetic is IEEE binary32, one rounding per operation, nothing fused, divisions correctly rounded, in the order written.
 *
 * Source: a device-resident float32 [H][W] map of the handle's geometry and an adc_calib of the rectified LEFT camera;
 * fb = focal_px * baseline (one multiply on the host).
 *   ADC_REG_FROM_DISPARITY  a = fabsf(d), s = a + doffs, valid <=> a finite and s > 0, Z = fb / s (the rule of adc_outputs.depth)
 *   ADC_REG_FROM_DEPTH      Z = v, valid <=> v finite and v > 0
 * Target camera (adc_reg_target): width, height in [1, 32767]; fx, fy, cx, cy; Brown-Conrady k1, k2, p1, p2, k3; R row-major maps
 * left-rectified coordinates to target coordinates; t in the unit of baseline.
 * Projection of a source point (xs, ys, Z):
 *   X = ((xs - cx) * Z) / focal_px, Y = ((ys - cy) * Z) / focal_px
 *   Xt = ((R0*X + R1*Y) + R2*Z) + t0, Yt = ((R3*X + R4*Y) + R5*Z) + t1, Zt = ((R6*X + R7*Y) + R8*Z) + t2
 *   in front <=> Zt finite and Zt > 0;  x = Xt / Zt, y = Yt / Zt
 *   x2 = x*x, y2 = y*y, r2 = x2 + y2, xy = x*y; rad = 1 + r2 (k1 + r2 (k2 + r2 k3));
 *   xd = (x rad + (2 p1) xy) + p2 (r2 + 2 x2); yd = (y rad + p1 (r2 + 2 y2)) + (2 p2) xy   (as in adc_set_rectify_model)
 *   u = fx xd + cx_t, v = fy yd + cy_t;  in range <=> fabsf(u) < 32768 and fabsf(v) < 32768 (NaN fails)
 * Footprint of a source pixel (x, y) with valid Z: three projections, all with the pixel's own Z -- the centre (float(x), float(y))
 * giving Zc = Zt and (uc, vc), corner A (float(x) - 0.5, float(y) - 0.5), corner B (float(x) + 0.5, float(y) + 0.5).  The pixel is
 * dropped unless all three are in front and in range.  With splat (the default): j0 = (int)ceilf(fminf(uA, uB)),
 * j1 = (int)ceilf(fmaxf(uA, uB)) - 1 (the target centres in [lo, hi)), i0 / i1 the same from v; without (ADC_REG_NO_SPLAT):
 * j0 = j1 = (int)floorf(uc + 0.5f), rows likewise.  Then in integers: j0 = max(j0, 0), j1 = min(j1, width - 1),
 * j1 = min(j1, j0 + ADC_REG_MAX_SPLAT - 1), rows likewise; an empty footprint writes nothing.  No float reaches an address.
 * Z-buffer: every target pixel of the footprint receives the key ((uint64)bits(Zc) << 32) | (uint32)(y * W + x) and keeps the MINIMUM
 * key (one 64-bit unsigned atomic minimum): for positive floats the bit order is the value order, so the nearest surface wins and among
 * equal Zc the lowest raster index; the result does not depend on the order of arrival.
 * Because the corners use the pixel's own Z, the footprints of a smooth slanted surface tile the target only approximately: small
 * cracks (target pixels no footprint covers) are part of the definition, not an error.
 * Outputs, device addresses, each may be NULL (not both):
 *   depth  float32 [Ht][Wt]: Zc of the winner, +inf where nothing landed
 *   index  int32 [Ht][Wt]: the winner's source raster index y * W + x, -1 where nothing landed (gather anything else through it)
 *   adc_reg_report: src_valid = source pixels with a valid Z, src_projected = those with a non-empty footprint, dst_filled = target
 *   pixels that received a key; read back through a pinned block behind the kernels, available after adc_wait
 * With R = I, t = 0, the source's intrinsics, no distortion and ADC_REG_FROM_DEPTH, depth equals the input bit for bit at every valid
 * pixel and index is the raster index.
 *
 * The other direction (colour aligned to depth): for every source pixel the centre projection only, j = (int)floorf(uc + 0.5f),
 * i = (int)floorf(vc + 0.5f); if Z is valid, the projection in front and in range and (i, j) inside the target:
 * out[y][x] = target_bgr[i][j] (3 bytes) and valid[y][x] = 1, otherwise the three bytes are 0 and valid is 0.  target_bgr is a tightly
 * packed uint8 [Ht][Wt][3], out uint8 [H][W][3] -- exactly what adc_reproject_device takes as d_bgr_left -- valid uint8 [H][W] or NULL.
 *
 * adc_set_register_target    validates and stores the target; the first call allocates the z-buffer (8 * Wt * Ht bytes) and the report
 *                            words, a larger target regrows the z-buffer (adc_create allocates none of them, adc_destroy frees them).
 *                            Synchronous.
 * adc_clear_register_target  back to "no target" (the buffers stay until adc_destroy).
 * adc_register_depth_device  asynchronous on the handle's stream, completed by adc_wait.  flags: ADC_REG_NO_SPLAT;
 *                            ADC_REG_PRETEST (measurement only: look at the z-buffer word with a plain load first and skip an atomic
 *                            that cannot win, instead of issuing every atomic -- the same result bit for bit).
 * adc_align_color_device     asynchronous, completed by adc_wait.
 * adc_register_depth /       the same with HOST pointers, synchronous; device scratch is allocated on the first call that needs it
 * adc_align_color            (freed by adc_destroy); report may be NULL.
 * adc_get_register_report    the report of the last registration that adc_wait (or adc_register_depth) has completed.
 * Return codes: 0; 1 with adc_last_error and nothing enqueued or changed (a NULL handle, map or calib, an unknown input kind or flag, a
 * calibration adc_match_out would refuse, a target with a non-finite field or fx or fy == 0, a size outside [1, 32767], no target
 * set, no output requested, a Match pending -- adc_wait first, for the reason given at adc_evaluate_device); 2 on a HIP failure (the
 * handle stays usable, a failed set call leaves the target unset).  The registered map is not a product of adc_products or the farm.
 * ------------------------------------------------------------------------------------------- */
#define ADC_REG_FROM_DISPARITY 0
#define ADC_REG_FROM_DEPTH 1
#define ADC_REG_NO_SPLAT 1u
#define ADC_REG_PRETEST 2u
#define ADC_REG_MAX_SPLAT 8
typedef struct adc_reg_target {
    int32_t width, height;
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3;
    float R[9];
    float t[3];
} adc_reg_target;
typedef struct adc_reg_report {
    uint32_t src_valid, src_projected, dst_filled;
    uint32_t reserved_;
} adc_reg_report;
int adc_set_register_target(adc_handle* h, const adc_reg_target* target);
int adc_clear_register_target(adc_handle* h);
int adc_register_depth_device(adc_handle* h, const void* d_map, int input_kind, const adc_calib* calib, uint32_t flags, void* d_depth,
                              void* d_index);
int adc_align_color_device(adc_handle* h, const void* d_map, int input_kind, const adc_calib* calib, const void* d_target_bgr,
                           void* d_bgr_out, void* d_valid);
int adc_register_depth(adc_handle* h, const float* map, int input_kind, const adc_calib* calib, uint32_t flags, float* depth,
                       int32_t* index, adc_reg_report* report);
int adc_align_color(adc_handle* h, const float* map, int input_kind, const adc_calib* calib, const uint8_t* target_bgr, uint8_t* bgr_out,
                    uint8_t* valid);
int adc_get_register_report(adc_handle* h, adc_reg_report* out);

/* -------------------------------------------------------------------------------------------
 * Surface normals from a disparity map on the device (a windowed plane fit in disparity space; k_normals.hip, the arithmetic is
 * adcensus_amd/csrc/normals_fit.h, tests/normals_ref.py holds the same definition in numpy and the kernel matches it bit for bit).
 * A plane in space is a plane in (x, y, disparity): the fit needs nine integer sums per pixel, its normal equations solve exactly in
 * 64-bit integers and the 3D normal follows in closed form; every sum is an integer, so the result does not depend on the order of
 * evaluation.  All float arithmetic is IEEE binary32, one rounding per operation, nothing fused, divisions and sqrtf correctly
 * rounded, in the order written.
 *
 * Input: a float32 [H][W] map d of the handle's geometry (signed; a = fabsf(d)) and an adc_calib of the rectified LEFT camera.  Only
 * focal_px, cx, cy and doffs enter the arithmetic; baseline is validated as elsewhere but cancels out.
 * Parameters (adc_normals_params): radius r in [1, 7]; max_diff finite, in (0, 64] pixels; min_points in [3, (2r+1)^2]; flags = 0 and
 * the reserved words 0.  The host computes G = (int32)rintf(max_diff * 1024.0f) once.
 * Usable pixel: a finite and a < 32768.0f (+inf, -inf, NaN and huge values of a caller's own map are not usable); its fixed-point
 * disparity is q = (int32)rintf(a * 1024.0f).
 * Support of a usable centre (x, y): the taps (dx, dy) in [-r, r]^2 that lie inside the image, are usable and satisfy |e| <= G with
 * e = q_tap - q_centre.  The centre is always a tap.  The gate keeps a window from fitting across a depth step.
 * Sums (integers): n; Sx = sum dx, Sy = sum dy; Sxx, Sxy, Syy; Se = sum e, Sxe = sum dx*e, Sye = sum dy*e.  With r <= 7 and
 * G <= 65536 every one of them fits int32.
 * Solve, exact in int64: M = [[Sxx, Sxy, Sx], [Sxy, Syy, Sy], [Sx, Sy, n]]; Dt = det M (a Gram determinant: >= 0, and 0 when the taps
 * are collinear); Na, Nb, Nc the determinants with column 0, 1 or 2 replaced by (Sxe, Sye, Se); |N*| < 2^57.  A fit exists iff
 * n >= min_points and Dt > 0.
 * Floats (each int64 -> float conversion is ONE rounding to nearest even):
 *   Df = (float)Dt;  ga = ((float)Na / Df) * 0x1p-10f, gb likewise from Nb
 *   dc = ((float)q_centre * 0x1p-10f) + (((float)Nc / Df) * 0x1p-10f);  s = dc + doffs; a fit needs s > 0
 *   nx = ga * focal_px, ny = gb * focal_px, nz = ((ga * (cx - (float)x)) + (gb * (cy - (float)y))) + s
 *   L = sqrtf(((nx*nx) + (ny*ny)) + (nz*nz)); it must be finite and > 0
 * Why this is the normal: the fitted plane d = ga x' + gb y' + c maps to the 3D plane (ga f) X + (gb f) Y + nz Z = f B, and
 * (nx, ny, nz) dotted with the pixel's viewing ray has the sign of s, so -(nx, ny, nz) / L always faces the camera.
 * Outputs, device addresses, each optional but at least one:
 *   normals   float32 [H][W][4], 16-byte aligned: (-nx/L, -ny/L, -nz/L, (float)n); (0, 0, 0, 0) where there is no normal
 *   normals8  uint8 [H][W][4], 4-byte aligned: per component (uint8)((int)rintf(v * 127.0f) + 128), the fourth byte 255;
 *             0, 0, 0, 0 where there is no normal (what a normal-map image holds)
 *   adc_normals_report: usable, fitted, few_points (usable centre, n < min_points), degenerate (enough points but Dt == 0, s <= 0, or
 *   L not finite or 0); usable = fitted + few_points + degenerate.  Read back through the handle's pinned block behind the kernel,
 *   available after adc_wait.
 *
 * adc_normals_device      asynchronous on the handle's stream, completed by adc_wait.  params NULL: r = 2, max_diff = 1.0,
 *                         min_points = 5.  The first call allocates the four report words (adc_create allocates nothing of this).
 * adc_normals             the same with HOST pointers, synchronous; device scratch is allocated on the first call that needs it
 *                         (freed by adc_destroy); report may be NULL.
 * adc_get_normals_report  the report of the last call that adc_wait (or adc_normals) has completed.
 * Return codes: 0; 1 with adc_last_error and nothing enqueued (a NULL handle, map or calib, a calibration adc_match_out would refuse,
 * a parameter out of range, a nonzero flag or reserved word, no output requested, a misaligned device address, a Match pending --
 * adc_wait first, for the reason given at adc_evaluate_device); 2 on a HIP failure (the handle stays usable).  The normals are not a
 * product of adc_products or the farm.
 * ------------------------------------------------------------------------------------------- */
#define ADC_NORMALS_MAX_RADIUS 7
typedef struct adc_normals_params {
    int32_t radius;      /* r in [1, 7]: the window is (2r+1) x (2r+1) */
    float max_diff;      /* the gate in pixels of disparity, (0, 64] */
    int32_t min_points;  /* [3, (2r+1)^2] */
    uint32_t flags;      /* 0 */
    uint32_t reserved_[4];
} adc_normals_params;
typedef struct adc_normals_report {
    uint32_t usable, fitted, few_points, degenerate;
} adc_normals_report;
int adc_normals_device(adc_handle* h, const void* d_disp, const adc_calib* calib, const adc_normals_params* params, void* d_normals,
                       void* d_normals8);
int adc_normals(adc_handle* h, const float* disp, const adc_calib* calib, const adc_normals_params* params, float* normals,
                uint8_t* normals8, adc_normals_report* report);
int adc_get_normals_report(adc_handle* h, adc_normals_report* out);

/* -------------------------------------------------------------------------------------------
 * Triangle mesh from a disparity map on the device (gated grid cells; k_mesh.hip, the cell rule is adcensus_amd/csrc/mesh_cell.h,
 * tests/mesh_ref.py holds the same definition in numpy and the kernels match it bit for bit, in whatever order the waves run).
 * All float arithmetic is IEEE binary32, one rounding per operation, nothing fused.
 *
 * Input: a float32 [H][W] map d of the handle's geometry, a = fabsf(d); an optional adc_calib (NULL: no calibration); an optional left
 * image uint8 [H][W][3] in B,G,R order (NULL: colours 0).
 * Parameters (adc_mesh_params, 32 bytes): float max_diff, not NaN and >= 0 (+inf is allowed and means no gate); int32_t step in
 * [1, 16]; uint32_t flags = 0; uint32_t reserved_[5] = 0.  NULL params: max_diff = 1.0, step = 1.
 * Lattice: columns x = i * step for i in [0, Wl), Wl = (W - 1) / step + 1; rows y = j * step for j in [0, Hl), Hl = (H - 1) / step + 1.
 * A lattice pixel's validity, position and colour are exactly those of adc_outputs.cloud: with a calibration valid <=> a finite and
 * a + doffs > 0, Z = fb / s, X = ((x - cx) * Z) / focal_px, Y = ((y - cy) * Z) / focal_px; without one valid <=> a != +inf, point
 * (x, y, a); r, g, b from the left image; pad = 0.
 * Edge: two lattice pixels p, q are joined iff both are valid and fabsf(a_p - a_q) <= max_diff (one subtraction; a NaN fails).
 * Cell (i, j) for i < Wl - 1, j < Hl - 1, corners A = lattice (i, j), B = (i+1, j), C = (i, j+1), D = (i+1, j+1):
 *   four valid corners: the diagonal is AD iff fabsf(a_A - a_D) <= fabsf(a_B - a_C) (ties go to AD; a NaN comparison is false, so BC).
 *                       With AD the candidates are T0 = (A, C, D) and T1 = (A, D, B); with BC T0 = (A, C, B) and T1 = (B, C, D).
 *   exactly three:      one candidate -- D missing: (A, C, B); A missing: (B, C, D); B missing: (A, C, D); C missing: (A, D, B).
 *   fewer:              no candidate.
 *   A candidate is emitted iff all three of its edges are joined.  Every listed winding has the same sign in pixel coordinates (x
 *   right, y down); with Z > 0 the geometric normal (v1 - v0) x (v2 - v0) of a fronto-parallel patch points at the camera, which agrees
 *   with adc_normals.
 * Triangles: cells in raster order (j, then i), within a cell T0 before T1; a record is three uint32 vertex numbers; `triangles` is
 * the number of all of them.
 * Vertices: the lattice pixels that are a corner of at least one emitted triangle, in raster order; a record is one adc_point
 * (16 bytes).  vertex_index (optional), int32 per vertex: the source raster index y * W + x -- gather anything else through it
 * (normals, confidence, provenance).  The vertex numbers in the triangles are positions in this full list.
 * Capacities: the first min(vertices, vertex_capacity) vertex records and vertex_index words are written and nothing behind them; the
 * first min(triangles, triangle_capacity) triangle records are written and nothing behind them; triangles keep their true vertex
 * numbers whatever the vertex capacity.  Wl * Hl vertices and 2 (Wl - 1)(Hl - 1) triangles always suffice.  A capacity of 0 with a
 * non-NULL pointer counts only.
 * Report (adc_mesh_report, uint32 each): lattice_valid, vertices, triangles, cells_two, cells_one (cells that emit two triangles /
 * one), three reserved words; triangles = 2 * cells_two + cells_one.  Read back through the handle's pinned block behind the
 * kernels, available after adc_wait.  d_counts (optional): uint32[2] = {vertices, triangles}, written on the stream, so that a GPU
 * consumer need not synchronise.
 *
 * adc_mesh_device      asynchronous on the handle's stream, completed by adc_wait.  d_vertices (16-byte aligned), d_vertex_index,
 *                      d_triangles, d_counts (4-byte aligned) are device addresses; at least one of d_vertices / d_triangles.  Only what
 *                      was asked for runs.  The first call allocates the scratch (adc_create allocates nothing of this).
 * adc_mesh             the same with HOST pointers, synchronous; device scratch is allocated on the first call that needs it (freed
 *                      by adc_destroy); copies out only min(count, capacity) records; report may be NULL.
 * adc_get_mesh_report  the report of the last call that adc_wait (or adc_mesh) has completed.
 * Return codes: 0; 1 with adc_last_error and nothing enqueued (a NULL handle or map, a calibration adc_match_out would refuse, a bad
 * parameter, flag or reserved word, neither vertices nor triangles requested, a vertex_index without vertices, d_vertices not
 * 16-byte aligned or any other device address not 4-byte aligned, a Match pending -- adc_wait first, for the reason given at
 * adc_evaluate_device); 2 on a HIP failure (the handle stays usable).  The mesh is not a product of adc_products or the farm.
 * ------------------------------------------------------------------------------------------- */
#define ADC_MESH_MAX_STEP 16
typedef struct adc_mesh_params {
    float max_diff;      /* the gate in pixels of disparity: not NaN, >= 0; +inf = no gate */
    int32_t step;        /* [1, 16]: every step-th column and row forms the lattice */
    uint32_t flags;      /* 0 */
    uint32_t reserved_[5];
} adc_mesh_params;
typedef struct adc_mesh_report {
    uint32_t lattice_valid, vertices, triangles, cells_two, cells_one;
    uint32_t reserved_[3];
} adc_mesh_report;
int adc_mesh_device(adc_handle* h, const void* d_disp, const void* d_bgr_left, const adc_calib* calib, const adc_mesh_params* params,
                    void* d_vertices, uint64_t vertex_capacity, void* d_vertex_index, void* d_triangles, uint64_t triangle_capacity,
                    void* d_counts);
int adc_mesh(adc_handle* h, const float* disp, const uint8_t* bgr_left, const adc_calib* calib, const adc_mesh_params* params,
             adc_point* vertices, uint64_t vertex_capacity, int32_t* vertex_index, uint32_t* triangles, uint64_t triangle_capacity,
             adc_mesh_report* report);
int adc_get_mesh_report(adc_handle* h, adc_mesh_report* out);

/* -------------------------------------------------------------------------------------------
 * TSDF volume on the device: depth maps of many frames fused into one truncated signed distance volume, and the surface points of
 * that volume (k_tsdf.hip; the voxel rule is adcensus_amd/csrc/tsdf_voxel.h, tests/tsdf_ref.py holds the same definition in numpy and
 * the kernels match it bit for bit, in whatever order the waves run: one thread owns a voxel, every accumulated quantity is an
 * integer).  Optional and off by default: the volume is handle state, adc_create allocates nothing of it, and no Match path changes.
 * All float arithmetic is IEEE binary32, one rounding per operation, nothing fused, parenthesised as written.
 *
 * Parameters (adc_tsdf_params, 64 bytes): int32 nx, ny, nz, each in [4, 2048], nx a multiple of 4, nx * ny * nz <= 2^30; float voxel
 * (the edge of a voxel), finite and > 0; float origin[3], finite, the world position of the CORNER of voxel (0, 0, 0); float trunc,
 * finite and > 0; float z_min, z_max, not NaN, 0 <= z_min <= z_max, z_max may be +inf; uint32 max_weight in [1, 65535]; uint32 flags:
 * ADC_TSDF_COLOR allocates a colour word per voxel; uint32 reserved_[4] = 0.  The host computes inv_trunc = 1.0f / trunc once.
 * Voxel (i, j, k) has the index n = (k * ny + j) * nx + i and is one uint32 word (uint16)(int16)t | w << 16: t in [-32767, 32767] is
 * the distance in units of trunc / 32767, w the weight (a stored t of -32768, which only adc_tsdf_upload can bring in, is read as
 * -32767).  With the colour flag there is a second uint32 per voxel: r | g << 8 | b << 16 | cw << 24.  All bytes zero = an empty volume.
 *
 * Frame (adc_tsdf_frame, 96 bytes): int32 kind, ADC_REG_FROM_DISPARITY or ADC_REG_FROM_DEPTH; an adc_calib; float R[9] row-major and
 * float t[3], which take a WORLD point into the rectified left CAMERA frame, Xc = R * Xw + t (for a camera-to-world pose (Rcw, c):
 * R = transpose(Rcw), t = -(R * c)); every field finite; uint32 flags = 0, uint32 reserved_[5] = 0.  fb = focal_px * baseline is one
 * multiply.  Validity and Z of a map value are exactly those of adc_register_depth_device (ADC_REG_FROM_*).
 *
 * Integrate.  Voxels are independent; a skipped voxel keeps its bits.  For voxel (i, j, k):
 *   1. centre: xw = origin[0] + ((float)i + 0.5f) * voxel; yw from j and origin[1], zw from k and origin[2] in the same way.
 *   2. camera frame: Xc = ((R[0]*xw + R[1]*yw) + R[2]*zw) + t[0]; Yc from R[3..5], t[1]; Zc from R[6..8], t[2].
 *   3. skip unless Zc is finite, Zc > 0 and z_min <= Zc && Zc <= z_max.
 *   4. project: rz = 1.0f / Zc; u = ((Xc * focal_px) * rz) + cx; v = ((Yc * focal_px) * rz) + cy; skip unless fabsf(u) < 32768.0f &&
 *      fabsf(v) < 32768.0f (a NaN fails).
 *   5. pixel: x = (int)floorf(u + 0.5f), y = (int)floorf(v + 0.5f); skip unless 0 <= x < W && 0 <= y < H.  No float reaches an
 *      address before that test.  The voxel now counts as in_frustum.
 *   6. depth: D = the Z of map[y][x] by the frame's kind; a pixel without depth: skip, count no_depth.
 *   7. signed distance: sdf = D - Zc; if !(sdf >= -trunc): skip, count occluded.  (D = +inf from an overflowing fb / s is free space.)
 *   8. quantise: f = fminf(sdf * inv_trunc, 1.0f); q = (int)floorf(f * 32767.0f + 0.5f)   (q >= -32767 whatever the rounding).
 *   9. update from the old t, w in non-negative integers: m = w + 1; t' = (t*w + q + 32767*m + m/2) / m - 32767;
 *      w' = min(w + 1, max_weight); count updated.  (The numerator stays below 2^32.)
 *  10. colour, only with a colour volume, an image given and fabsf(sdf) <= trunc: cm = cw + 1; each channel becomes
 *      (c*cw + c_obs + cm/2) / cm with c_obs from the left image at (x, y), stored B,G,R; cw' = min(cw + 1, min(max_weight, 255)).
 * Integrate report (adc_tsdf_report, uint32 each): in_frustum (voxels that reached step 6), no_depth, occluded, updated, four
 * reserved words; in_frustum = no_depth + occluded + updated.
 *
 * Extract (surface points).  Parameters (adc_tsdf_extract_params, 32 bytes): uint32 min_weight in [1, 65535], uint32 reserved_[7] = 0;
 * NULL: min_weight = 1.  For voxel a = (i, j, k) and an axis x, y or z whose neighbour b = a + 1 on that axis lies inside the volume,
 * the pair is a crossing iff w_a >= min_weight && w_b >= min_weight && (t_a < 0) != (t_b < 0).  s = (float)t_a / ((float)t_a -
 * (float)t_b): both conversions and the difference are exact, so there is one rounding.  The point is a's centre as in step 1 with
 * s * voxel added to the coordinate of that axis.  A record is an adc_point in the WORLD frame; r, g, b come from a when s <= 0.5f and
 * from b otherwise (0 without a colour volume); pad = min(min(w_a, w_b), 255).  Order: ascending n of a; within a voxel x, then y, then
 * z.  `points` is the number of crossings whatever the capacity: the first min(points, capacity) records are written and nothing
 * behind them; a capacity of 0 with a non-NULL pointer counts only.  d_count (optional): one uint32 device word = points, written on
 * the stream.  A voxel whose t is exactly 0 can yield two coincident points: the crossing in front of it ends on its centre (s = 1
 * from a - 1) and the crossing behind it starts there (s = 0).
 * Extract report (adc_tsdf_extract_report, uint32 each): voxels_seen (w >= min_weight), points, six reserved words.
 *
 * adc_tsdf_create            allocates and zeroes the volume (4 bytes per voxel, 8 with ADC_TSDF_COLOR); a second call replaces it.
 * adc_tsdf_reset             an empty volume again: one memset per plane of words.
 * adc_tsdf_destroy           gives the volume's memory back early (adc_destroy frees it too); 0 also when there was none.
 * adc_tsdf_integrate_device  one frame; d_map float32 [H][W] of the handle's geometry (4-byte aligned), d_bgr_left uint8 [H][W][3] or
 *                            NULL.  Asynchronous on the handle's stream, completed by adc_wait; successive calls may be enqueued
 *                            without a wait between them (the stream orders them; the report is that of the last).
 * adc_tsdf_integrate         the same with HOST pointers, synchronous; device scratch is allocated on the first call that needs it.
 * adc_tsdf_extract_device    the surface points; d_points is 16-byte aligned, d_count 4-byte aligned; asynchronous, completed by adc_wait.
 *                            The first call allocates the scratch (per-tile counts).
 * adc_tsdf_extract           the same with HOST pointers, synchronous; copies out min(points, capacity) records; points may be NULL
 *                            with capacity 0 (counts only).  Its device scratch holds min(points, capacity) records: when it has to
 *                            grow, the call counts first, so a generous capacity costs no memory.
 * adc_get_tsdf_report        the reports of the last completed integrate / extract call; either pointer may be NULL (not both); a
 *                            report that is asked for and does not exist yet is refused.
 * adc_tsdf_get_volume_device the device addresses of the voxel words and the colour words (NULL without a colour volume) and the
 *                            parameters, for a GPU consumer such as a ray caster; each out pointer may be NULL.
 * adc_tsdf_download / adc_tsdf_upload   host copies of the whole volume, synchronous (they wait for the handle's stream first): tsdf
 *                            uint32 [nz][ny][nx], color the same or NULL.  To save and restore a volume.
 * Return codes: 0; 1 with adc_last_error and nothing enqueued or changed (a NULL argument, a bad parameter, flag or reserved word, no
 * volume, a calibration adc_match_out would refuse, a non-finite R or t, a misaligned device address, an image given without a colour
 * volume -- refused, not ignored --, a colour pointer given to download / upload without a colour volume, a Match pending -- adc_wait
 * first, for the reason given at adc_evaluate_device); 2 on a HIP failure (the handle stays usable; after a failed adc_tsdf_create
 * there is no volume).  The volume is not a product of adc_products or the farm.
 * ------------------------------------------------------------------------------------------- */
#define ADC_TSDF_COLOR 1u
#define ADC_TSDF_MAX_DIM 2048
typedef struct adc_tsdf_params {
    int32_t nx, ny, nz;
    float voxel;
    float origin[3];
    float trunc;
    float z_min, z_max;
    uint32_t max_weight;
    uint32_t flags;      /* ADC_TSDF_COLOR */
    uint32_t reserved_[4];
} adc_tsdf_params; /* 64 bytes */
typedef struct adc_tsdf_frame {
    int32_t kind;        /* ADC_REG_FROM_DISPARITY / ADC_REG_FROM_DEPTH */
    adc_calib calib;
    float R[9], t[3];    /* world -> camera */
    uint32_t flags;      /* 0 */
    uint32_t reserved_[5];
} adc_tsdf_frame; /* 96 bytes */
typedef struct adc_tsdf_report {
    uint32_t in_frustum, no_depth, occluded, updated;
    uint32_t reserved_[4];
} adc_tsdf_report;
typedef struct adc_tsdf_extract_params {
    uint32_t min_weight; /* [1, 65535] */
    uint32_t reserved_[7];
} adc_tsdf_extract_params;
typedef struct adc_tsdf_extract_report {
    uint32_t voxels_seen, points;
    uint32_t reserved_[6];
} adc_tsdf_extract_report;
int adc_tsdf_create(adc_handle* h, const adc_tsdf_params* params);
int adc_tsdf_reset(adc_handle* h);
int adc_tsdf_destroy(adc_handle* h);
int adc_tsdf_integrate_device(adc_handle* h, const void* d_map, const void* d_bgr_left, const adc_tsdf_frame* frame);
int adc_tsdf_integrate(adc_handle* h, const float* map, const uint8_t* bgr_left, const adc_tsdf_frame* frame, adc_tsdf_report* report);
int adc_tsdf_extract_device(adc_handle* h, const adc_tsdf_extract_params* params, void* d_points, uint64_t capacity, void* d_count);
int adc_tsdf_extract(adc_handle* h, const adc_tsdf_extract_params* params, adc_point* points, uint64_t capacity,
                     adc_tsdf_extract_report* report);
int adc_get_tsdf_report(adc_handle* h, adc_tsdf_report* integrate_report, adc_tsdf_extract_report* extract_report);
int adc_tsdf_get_volume_device(adc_handle* h, void** d_tsdf, void** d_color, adc_tsdf_params* params);
int adc_tsdf_download(adc_handle* h, uint32_t* tsdf, uint32_t* color);
int adc_tsdf_upload(adc_handle* h, const uint32_t* tsdf, const uint32_t* color);

/* -------------------------------------------------------------------------------------------
 * Triangle mesh of the TSDF volume on the device (marching cubes; k_tsdf.hip, the cell rule is adcensus_amd/csrc/tsdf_cell.h, the case
 * table adcensus_amd/csrc/tsdf_mc_table.h is generated by tools/gen_tsdf_mc_table.py; tests/tsdf_mesh_ref.py holds the same definition
 * in numpy and the kernels match it bit for bit, in whatever order the waves run).  A triangle is three integers chosen by integer
 * comparisons; the vertices carry the only float arithmetic, that of adc_tsdf_extract.
 *
 * Parameters: adc_tsdf_extract_params (min_weight); NULL: min_weight = 1.
 * Vertices: the point list of adc_tsdf_extract for the same min_weight -- the same records in the same order, including crossings
 * that no triangle uses (next to unseen voxels, on the volume's border).  The vertex number of the crossing (owner voxel a, axis) is
 * its position in that full list, whatever the vertex capacity.
 * Cells: cell (i, j, k) exists for i < nx - 1, j < ny - 1, k < nz - 1 and has the index n = (k * ny + j) * nx + i.  Corner c in [0, 8)
 * is voxel (i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)).  A cell is seen iff all eight corners have w >= min_weight; only
 * seen cells emit.  Case index: bit c is set iff t_c < 0 (a stored -32768 reads as -32767; t = 0 counts as positive, as for a
 * crossing).  Every sign-changing edge of a seen cell is therefore a crossing of the vertex list.
 * Cell edges: e = 4 * axis + m, m in [0, 4); the owner corner has the offsets (0, m & 1, m >> 1) for axis x, (m & 1, 0, m >> 1) for y,
 * (m & 1, m >> 1, 0) for z; the edge runs from the owner to its +axis neighbour and its vertex is the crossing (owner voxel, axis).
 * Case table (256 rows, generated): 1. on each of the six faces, a face with two sign-changing edges gets one segment joining them; a
 * face with four (its negative corners on a diagonal) gets two, each joining the two edges that meet at a NEGATIVE corner -- the rule
 * reads the face's four signs only, so the two cells that share a face draw the same segments and there are no cracks.  2. every
 * sign-changing edge has one segment on each of its two faces, so the segments chain into closed loops; a loop is directed so that the
 * geometric normal (v1 - v0) x (v2 - v0) of its triangles points from the negative corners to the positive side (case 1, corner 0
 * negative, is the triangle (e0, e4, e8)), starts at its lowest edge number, and the loops are ordered by their lowest edge number.
 * 3. a loop L0 .. L(m-1) becomes a fan (Ls, L(s+i), L(s+i+1)), i = 1 .. m - 2, indices modulo m: the apex is L0 wherever that is
 * admissible, precisely s is the smallest index whose fan has no diagonal joining two edges of ONE face of the cell (such a diagonal
 * lies in a face two cells share and could be drawn by both).  So on a closed surface every directed edge (a, b) occurs exactly once
 * and (b, a) exactly once.  The largest number of triangles of a case is M = 5.
 * Triangles: cells in ascending n, within a cell in table order; a record is three uint32 vertex numbers.  A voxel with t = 0 yields
 * coincident vertices (see the extraction), so zero-area triangles occur and are kept.
 * Capacities: the first min(vertices, vertex_capacity) vertex records and the first min(triangles, triangle_capacity) triangle records
 * are written and nothing behind them; a capacity of 0 with a non-NULL pointer counts only.  Both counts are always taken (one fused
 * pass over the volume); only the records that were asked for are written.  d_counts (optional): uint32[2] = {vertices, triangles},
 * written on the stream.
 * Report (adc_tsdf_mesh_report, uint32 each): voxels_seen, vertices, triangles, cells_seen, cells_surface (seen cells with at least
 * one triangle), three reserved words.
 * Count limit: the counts are 32-bit.  A call is refused when M * (nx - 1)(ny - 1)(nz - 1) > 2^32 - 1 (a volume of 2^30 voxels is;
 * 1024 x 1024 x 800 is not).
 * Cost: a call with triangles keeps one uint32 per voxel of device scratch (the rank of the voxel's first crossing; 4 bytes per voxel,
 * 512 MB at 512^3), allocated on the first such call, growing with the largest volume, freed by adc_destroy; and two uint32 per tile
 * of 256 voxels.
 *
 * adc_tsdf_mesh_device   asynchronous on the handle's stream, completed by adc_wait.  d_vertices (16-byte aligned), d_triangles and
 *                        d_counts (4-byte aligned) are device addresses; at least one of d_vertices / d_triangles.
 * adc_tsdf_mesh          the same with HOST pointers, synchronous; copies out min(count, capacity) records of each list.  Its device
 *                        scratch holds min(count, capacity) records: when it has to grow, the call counts first.
 * adc_get_tsdf_mesh_report  the report of the last call that adc_wait (or adc_tsdf_mesh) has completed.
 * Return codes as for adc_tsdf_extract: 0; 1 with adc_last_error and nothing enqueued (also: neither list requested, a pointer that is
 * NULL with a capacity, the count limit); 2 on a HIP failure (the handle and the volume stay usable).  A Match may be enqueued behind a
 * pending call and one adc_wait completes both.  The mesh is not a product of adc_products or the farm.
 * ------------------------------------------------------------------------------------------- */
typedef struct adc_tsdf_mesh_report {
    uint32_t voxels_seen, vertices, triangles, cells_seen, cells_surface;
    uint32_t reserved_[3];
} adc_tsdf_mesh_report;
int adc_tsdf_mesh_device(adc_handle* h, const adc_tsdf_extract_params* params, void* d_vertices, uint64_t vertex_capacity,
                         void* d_triangles, uint64_t triangle_capacity, void* d_counts);
int adc_tsdf_mesh(adc_handle* h, const adc_tsdf_extract_params* params, adc_point* vertices, uint64_t vertex_capacity,
                  uint32_t* triangles, uint64_t triangle_capacity, adc_tsdf_mesh_report* report);
int adc_get_tsdf_mesh_report(adc_handle* h, adc_tsdf_mesh_report* out);

/* -------------------------------------------------------------------------------------------
 * Ray cast of the TSDF volume on the device: the fused surface as seen from a camera pose, as depth, normal, colour and status maps
 * (k_tsdf_raycast.hip; the ray rule is adcensus_amd/csrc/tsdf_ray.h, tests/tsdf_raycast_ref.py holds the same definition in numpy and
 * the kernel matches it bit for bit, in whatever order the waves run: one thread owns a ray).  The predicted maps of frame-to-model
 * tracking, a viewer's image, or a denoised depth map of the current frame.  The volume is only read.  All float arithmetic is IEEE
 * binary32, one rounding per operation, nothing fused, parenthesised as written; divisions and the square root are correctly rounded.
 *
 * View (adc_tsdf_raycast_params, 128 bytes): int32 width, height, each in [1, 8192], independent of the handle's image size; float
 * focal_px (finite, > 0), cx, cy (finite); float R[9] row-major and t[3], world -> camera as in adc_tsdf_frame, all finite; float
 * z_near, z_far, finite, 0 < z_near < z_far; float step (finite, > 0), the advance in camera depth Z between samples, and float skip
 * (finite, >= step), the advance behind a sample in saturated free space; uint32 min_weight in [1, 65535]; uint32 max_steps in
 * [1, 16384], the largest number of samples of a ray: whatever the other parameters are, no ray takes more (the loop ends on this
 * counter even where Z + step == Z); uint32 flags = 0; uint32 reserved_[8] = 0.  The usual choice is step = voxel / 2 and
 * skip = trunc / 2; neither is enforced.  The host computes inv_voxel = 1.0f / voxel once.
 *
 * Ray of pixel (x, y).  Camera-frame direction (dx, dy, 1): dx = ((float)x - cx) / focal_px, dy = ((float)y - cy) / focal_px, so the
 * ray parameter IS the camera-frame depth Z.  Per world axis a in {0, 1, 2}:
 *   dw_a = ((R[a] * dx) + (R[3+a] * dy)) + R[6+a]                                (transpose(R) * (dx, dy, 1))
 *   c_a  = -(((R[a] * t[0]) + (R[3+a] * t[1])) + (R[6+a] * t[2]))                (the camera centre)
 *   g0_a = ((c_a - origin[a]) * inv_voxel) - 0.5f;   gd_a = dw_a * inv_voxel     (grid coordinates: voxel centres are the integers)
 * The sample at depth Z lies at g_a = g0_a + (Z * gd_a).
 * Clip (the slab method on the box of centres [0, n_a - 1]; part of the definition).  Z_lo = z_near, Z_hi = z_far; for a = 0, 1, 2:
 * a non-finite g0_a or gd_a makes the ray a MISS; with gd_a == 0 the ray is a MISS unless 0 <= g0_a <= (float)(n_a - 1), and the axis
 * constrains nothing else; otherwise t1 = (0.0f - g0_a) / gd_a, t2 = ((float)(n_a - 1) - g0_a) / gd_a, a non-finite t1 or t2 makes
 * the ray a MISS, and Z_lo = max(Z_lo, min(t1, t2)), Z_hi = min(Z_hi, max(t1, t2)).  !(Z_lo <= Z_hi): MISS.
 * March.  Z = Z_lo, no previous sample.  Repeat: if !(Z <= Z_hi) the status is NO_SURFACE; else if max_steps samples were taken it is
 * EXHAUSTED; else take the sample at Z:
 *   1. per axis: g_a as above; unless fabsf(g_a) < 32768.0f the sample is not inside; cell_a = (int)floorf(g_a), frac_a = g_a -
 *      floorf(g_a) (exact).  The sample is inside iff 0 <= cell_a < n_a - 1 on every axis (integers).  No float reaches an address.
 *   2. inside: the nearest voxel is cell_a + (frac_a >= 0.5f) per axis.  If it is seen (w >= min_weight) and its t == 32767
 *      (saturated free space), the sample is FREE: f = 32767.0f, the next depth is Z + skip.
 *   3. otherwise, if all eight corners of the cell (corner c = cell + (c & 1, (c >> 1) & 1, (c >> 2) & 1), as for the mesh) are
 *      seen, f is the trilinear interpolant of their t (a stored -32768 reads as -32767) as floats: along x, then y, then z, each
 *      lo + (frac * (hi - lo)) -- four, two, one.  The next depth is Z + step.
 *   4. otherwise (not inside, or a corner unseen) the sample is UNSEEN: there is no previous sample any more; next depth Z + step.
 *   A free or interpolated sample with f <= 0 ends the ray: with a previous sample (Z_prev, f_prev > 0) the status is HIT and
 *   Zh = Z_prev + ((Z - Z_prev) * (f_prev / (f_prev - f))); without one it is BEHIND (the back of a surface, or its inside met through
 *   unseen space).  With f > 0 the sample becomes the previous one.
 * At a HIT the cell and the fractions are taken again at Zh (step 1).  If that sample is not inside, normal and colour are zeros.
 *   Colour: the colour word of the nearest voxel (step 2); cw > 0: its B, G, R bytes, otherwise 0, 0, 0.
 *   Normal: if all eight corners are seen, the gradient of the trilinear interpolant: gx is the blend of the four differences along x
 *   (t1 - t0, t3 - t2, t5 - t4, t7 - t6) in y, then z; gy of (t2 - t0, t3 - t1, t6 - t4, t7 - t5) in x, then z; gz of (t4 - t0,
 *   t5 - t1, t6 - t2, t7 - t3) in x, then y.  L = sqrtf(((gx * gx) + (gy * gy)) + (gz * gz)); unless L is finite and > 0 the record
 *   is four zeros; n = (gx / L, gy / L, gz / L), rotated into the CAMERA frame: ((R[3r] * n0) + (R[3r+1] * n1)) + (R[3r+2] * n2).
 *   The fourth float is the smallest weight of the eight corners.  No flip: the gradient points to the positive (free) side, which
 *   at a HIT is the side the ray came from, so the z component is negative for a surface that faces the camera -- the sign
 *   convention of adc_normals.  A corner unseen: four zeros; the depth stays.
 * Outputs, each optional, at least one: depth float32 [height][width], Zh or 0.0f where the status is not HIT (0.0f is "no depth"
 * for ADC_REG_FROM_DEPTH); normals float32 [height][width][4], 16-byte aligned; bgr uint8 [height][width][3], refused without a
 * colour volume; status uint8 [height][width], an ADC_TSDF_RAY_* value.  Nothing is written behind the last pixel.
 * Report (adc_tsdf_raycast_report, uint32 each): rays = width * height; miss, hit, no_surface, behind, exhausted (they sum to rays);
 * samples_lo, samples_hi: the number of samples of all rays as a 64-bit count; eight reserved words.
 *
 * adc_tsdf_raycast_device      asynchronous on the handle's stream, completed by adc_wait; device addresses (d_depth 4-byte, d_normals
 *                              16-byte aligned).  Calls may be enqueued back to back and behind adc_tsdf_integrate_device.
 * adc_tsdf_raycast             the same with HOST pointers, synchronous; device scratch is allocated on first use and grows with the
 *                              largest view.
 * adc_get_tsdf_raycast_report  the report of the last call that adc_wait (or adc_tsdf_raycast) has completed; refused while none exists.
 * Return codes as for adc_tsdf_extract: 0; 1 with adc_last_error and nothing enqueued (a NULL params, a bad field, flag or reserved
 * word, no volume, no output requested, bgr without a colour volume, a misaligned device address, a Match pending); 2 on a HIP
 * failure (the handle and the volume stay usable).  A Match may be enqueued behind a pending call and one adc_wait completes both.
 * Not a product of adc_products or the farm.
 * ------------------------------------------------------------------------------------------- */
#define ADC_TSDF_RAY_MISS 0
#define ADC_TSDF_RAY_HIT 1
#define ADC_TSDF_RAY_NO_SURFACE 2
#define ADC_TSDF_RAY_BEHIND 3
#define ADC_TSDF_RAY_EXHAUSTED 4
typedef struct adc_tsdf_raycast_params {
    int32_t width, height;
    float focal_px, cx, cy;
    float R[9], t[3];    /* world -> camera */
    float z_near, z_far;
    float step, skip;
    uint32_t min_weight; /* [1, 65535] */
    uint32_t max_steps;  /* [1, 16384] */
    uint32_t flags;      /* 0 */
    uint32_t reserved_[8];
} adc_tsdf_raycast_params; /* 128 bytes */
typedef struct adc_tsdf_raycast_report {
    uint32_t rays, miss, hit, no_surface, behind, exhausted;
    uint32_t samples_lo, samples_hi;
    uint32_t reserved_[8];
} adc_tsdf_raycast_report; /* 64 bytes */
int adc_tsdf_raycast_device(adc_handle* h, const adc_tsdf_raycast_params* params, void* d_depth, void* d_normals, void* d_bgr,
                            void* d_status);
int adc_tsdf_raycast(adc_handle* h, const adc_tsdf_raycast_params* params, float* depth, float* normals, uint8_t* bgr, uint8_t* status,
                     adc_tsdf_raycast_report* report);
int adc_get_tsdf_raycast_report(adc_handle* h, adc_tsdf_raycast_report* out);

/* -------------------------------------------------------------------------------------------
 * Frame-to-model camera tracking on the device: the pose of the current frame from its depth (or disparity) map and the model's
 * predicted depth and normal maps, by projective point-to-plane ICP (k_tsdf_track.hip; the rule is adcensus_amd/csrc/tsdf_track.h,
 * tests/tsdf_track_ref.py holds the same definition in numpy and the kernels match it bit for bit, in whatever order the waves run:
 * everything summed over pixels is an integer).  The loop: adc_tsdf_raycast_device at the last pose, adc_track_device, then
 * adc_tsdf_integrate_device at the recovered pose.  The iterations never return to the host.  Nothing here touches the volume.
 *
 * Inputs.  The current frame's map, float32 [H][W] of the handle's geometry, with an adc_tsdf_frame: kind and calib are read as
 * adc_tsdf_integrate reads them (validity and Z of a map value: ADC_REG_FROM_*), R, t are the INITIAL GUESS, world -> camera.
 * Optionally the frame's normals, float32 [H][W][4] as adc_normals_device writes them.  The model maps: depth float32 [mh][mw] and
 * normals float32 [mh][mw][4] as adc_tsdf_raycast_device writes them, with the adc_tsdf_raycast_params they were cast with, of which
 * only width, height (each in [1, 8192]), focal_px, cx, cy, R, t (Rm, tm below; all finite, focal_px > 0) are read.
 *
 * Parameters (adc_track_params, 64 bytes; NULL selects the defaults in brackets, which are API defaults and NOT measured optima):
 * uint32 iterations in [1, 32] [10]; uint32 stride in [1, 16] [1]; float max_dist, finite, > 0 [0.1]; float min_cos in [-1, 1] [0.8];
 * float z_far, finite, > 0 [8]; uint32 min_pixels >= 6 [64]; float eps_rot, eps_trans >= 0 [1e-5, 1e-5]; float max_rot, max_trans,
 * finite, > 0 [0.5, 0.5]; float damping, finite, >= 0 [0]; float pivot_ratio in [0, 1) [1e-6]; uint32 flags = 0; uint32 reserved_[3] = 0.
 * The host computes max_dist2 = max_dist * max_dist once (binary32).
 *
 * Reduce pass under the current estimate (Rk, tk), floats.  Binary32, one rounding per operation, nothing fused, parenthesised as
 * written.  Every pixel (x, y) with x % stride == 0 && y % stride == 0 participates (`pixels` of them: ceil(W / stride) *
 * ceil(H / stride), at most 2^26) and counts as exactly one of seven things:
 *   1. depth: Z of map[y][x] by the frame's kind; a pixel without depth, or with !(Z <= z_far): no_depth.
 *   2. camera point: Pc = ((((float)x - cx) / focal_px) * Z, (((float)y - cy) / focal_px) * Z, Z).
 *   3. world point: d = Pc - tk; Pw_a = ((Rk[a] * d0) + (Rk[3+a] * d1)) + (Rk[6+a] * d2)                     (transpose(Rk) * d)
 *   4. model camera: Pm_r = (((Rm[3r] * Pw0) + (Rm[3r+1] * Pw1)) + (Rm[3r+2] * Pw2)) + tm[r].
 *   5. projection, as steps 3 to 5 of the integrate definition with the model view's intrinsics: Pm_2 finite and > 0; rz = 1.0f /
 *      Pm_2; u = ((Pm_0 * fm) * rz) + cxm; v likewise; fabsf(u) < 32768.0f && fabsf(v) < 32768.0f; xm = (int)floorf(u + 0.5f), ym
 *      likewise; 0 <= xm < mw && 0 <= ym < mh.  No float reaches an address before that integer test.  Otherwise: outside.
 *   6. model sample: Dm = depth[ym][xm], nm = normals[ym][xm]; !(Dm > 0.0f) or !(nm[3] > 0.0f) (a NaN included): no_model.
 *   7. distance gate: Qm = ((((float)xm - cxm) / fm) * Dm, (((float)ym - cym) / fm) * Dm, Dm); diff = Pm - Qm;
 *      d2 = ((diff0 * diff0) + (diff1 * diff1)) + (diff2 * diff2); !(d2 <= max_dist2): far (the count too_far).
 *   8. angle gate, only with frame normals given and the frame normal's fourth float > 0: nw = transpose(Rk) * nf as in step 3,
 *      nr_r = ((Rm[3r] * nw0) + (Rm[3r+1] * nw1)) + (Rm[3r+2] * nw2); dot = ((nr0 * nm0) + (nr1 * nm1)) + (nr2 * nm2);
 *      !(dot >= min_cos): angle.
 *   9. residual r = ((nm0 * diff0) + (nm1 * diff1)) + (nm2 * diff2); Jacobian for a twist (omega, v) applied on the LEFT in the
 *      model camera frame (Pm' = Pm + omega x Pm + v): J = (c, nm) with c = Pm x nm, c0 = (Pm1 * nm2) - (Pm2 * nm1), c1 = (Pm2 * nm0) -
 *      (Pm0 * nm2), c2 = (Pm0 * nm1) - (Pm1 * nm0).
 *  10. quantise, Q = 65536: the seven values s = (c0 / z_far, c1 / z_far, c2 / z_far, nm0, nm1, nm2, r / max_dist); unless
 *      fabsf(s_i) < 4.0f for all seven (a NaN fails): out_of_range.  q_i = (int32)rintf(s_i * 65536.0f) (ties to even); the pixel is used.
 *  11. sums, all int64 and exact: the 21 products q_i * q_j, i <= j < 6, by rows; the 6 products q_i * q_6; q_6 * q_6.
 * No overflow: |q_i| <= 4 * 65536 = 2^18, a product is at most 2^36, at most 2^26 pixels participate, so every sum stays at or below
 * 2^62.  The constants 65536, 4 and 2^26 may change only together with this derivation (it is repeated in tsdf_track.h).  The seven
 * counts add up to pixels.  Because everything accumulated is an integer, no result depends on the order in which waves arrive.
 *
 * Solve, once per reduce pass, in binary64 with + - * / only, a fixed order, nothing fused (two square roots fill the norms of the
 * iteration record and are read by no decision: every threshold is compared in squares).
 *   scales: zs = (double)z_far / 65536, rs = (double)max_dist / 65536, sc = (zs, zs, zs, 1/65536, 1/65536, 1/65536);
 *   H_ij = ((double)S_ij * sc_i) * sc_j (symmetric), b_i = ((double)S_i6 * sc_i) * rs, rms = sqrt((((double)S_66 * rs) * rs) / used).
 *   used < min_pixels: LOST.
 *   diag_i = H_ii + (damping * H_ii).  H = L D L^T without pivoting, column j = 0 .. 5: d_j = diag_j - sum over c < j, ascending,
 *   of ((L_jc * L_jc) * d_c), subtracted one by one; unless d_j is finite and d_j > pivot_ratio * diag_j: DEGENERATE; for i > j:
 *   L_ij = (H_ij - sum over c < j of ((L_ic * L_jc) * d_c)) / d_j.
 *   H xi = -b: y_i = -b_i - sum over c < i of (L_ic * y_c); z_i = y_i / d_i; for i = 5 .. 0: xi_i = z_i - sum over c > i, ascending,
 *   of (L_ci * xi_c).  xi = (omega, v).  w2 = ((omega0^2 + omega1^2) + omega2^2), v2 likewise.
 *   !(w2 <= max_rot^2) or !(v2 <= max_trans^2) (squares of the doubles; a NaN included): DIVERGED.
 *   After LOST, DEGENERATE or DIVERGED the pose stays the last accepted one, bit for bit.
 *   Update.  The rotation of the step is the Cayley map of a = omega * 0.5 -- a rotation by rational arithmetic alone, no sin or cos,
 *   on which a host's libm and the device library would not agree: aa = ((a0^2 + a1^2) + a2^2);
 *   dR_ij = ((((i == j) ? 1 - aa : 0) + (2 * (a_i * a_j))) + (2 * X_ij)) / (1 + aa), X = [0 -a2 a1; a2 0 -a0; -a1 a0 0]; dT = (dR, v).
 *   Tk <- ((Tk * Tm^-1) * dT^-1) * Tm with (R1, t1) * (R2, t2) = (R1 R2, R1 t2 + t1), every entry ((x + y) + z) [+ t1_i], and
 *   (R, t)^-1 = (R^T, -(R^T t)).  Then one square-root-free step towards an orthonormal rotation: R <- R * ((3 I - R^T R) * 0.5).
 *   R and t are rounded once to float: the estimate of the next reduce pass.
 *   w2 < eps_rot^2 && v2 < eps_trans^2: CONVERGED (the step has been applied).  After `iterations` solves: MAX_ITERATIONS.
 *
 * Result (adc_track_result, 960 bytes): uint32 status (ADC_TRACK_*), uint32 solves (the number of solves run); float R[9], t[3], the
 * last accepted pose, ready to be copied into an adc_tsdf_frame; uint32 pixels, no_depth, outside, no_model, too_far, angle,
 * out_of_range, used of the last reduce pass; double H[36] (row-major 6 x 6) and b[6] of the last solve, undamped, twist order omega
 * then v, model camera frame, for pose-graph users; adc_track_iteration iteration[32]: uint32 used, float rms (of the residual, in
 * the map's unit), rot = |omega|, trans = |v| of each solve run (rot and trans are 0 where the solve ended before it had a step);
 * uint32 reserved_[6] = 0.
 *
 * adc_track_device      asynchronous on the handle's stream, completed by adc_wait: one clear, `iterations` pairs of (reduce, solve)
 *                       enqueued up front, one read-back.  Every kernel begins with a wave-uniform read of a `done` word and returns
 *                       at once when a terminal status has set it.  No host synchronisation in between, no graph, no other stream.
 *                       d_map and d_model_depth 4-byte, d_frame_normals (may be NULL) and d_model_normals 16-byte aligned; d_result
 *                       (optional, 8-byte aligned) receives the same record on the stream for a GPU consumer.  May be enqueued
 *                       directly behind adc_tsdf_raycast_device; a Match may be enqueued behind it and one adc_wait completes both.
 *                       Its state and its pinned result block are its own, allocated on first use; it needs no volume.
 * adc_tsdf_track        HOST pointers, synchronous; needs a volume: ray-casts it from the frame's own pose and intrinsics at W x H with
 *                       step = voxel / 2, skip = max(trunc / 2, step), z_near = voxel, z_far = 3e38, min_weight 1, max_steps 16384,
 *                       then tracks the map against those maps.  Device scratch is allocated on first use.
 * adc_get_track_result  the result of the last call that adc_wait (or adc_tsdf_track) has completed; refused while none exists.
 * Return codes: 0; 1 with adc_last_error and nothing enqueued (a NULL argument, a bad field, flag or reserved word, a non-finite pose,
 * a calibration adc_tsdf_integrate would refuse, more than 2^26 participating pixels, a model view larger than 8192 on a side, a
 * misaligned address, a Match pending, for adc_tsdf_track no volume) -- every refusal stands before the first HIP call; 2 on a HIP
 * failure (the handle stays usable).  Not a product of adc_products or the farm.
 * ------------------------------------------------------------------------------------------- */
#define ADC_TRACK_CONVERGED 0
#define ADC_TRACK_MAX_ITERATIONS 1
#define ADC_TRACK_LOST 2
#define ADC_TRACK_DEGENERATE 3
#define ADC_TRACK_DIVERGED 4
#define ADC_TRACK_MAX_ITERATIONS_LIMIT 32
typedef struct adc_track_params {
    uint32_t iterations;   /* [1, 32] */
    uint32_t stride;       /* [1, 16] */
    float max_dist;
    float min_cos;
    float z_far;
    uint32_t min_pixels;   /* >= 6 */
    float eps_rot, eps_trans;
    float max_rot, max_trans;
    float damping;
    float pivot_ratio;     /* [0, 1) */
    uint32_t flags;        /* 0 */
    uint32_t reserved_[3];
} adc_track_params; /* 64 bytes */
typedef struct adc_track_iteration {
    uint32_t used;
    float rms, rot, trans;
} adc_track_iteration;
typedef struct adc_track_result {
    uint32_t status;       /* ADC_TRACK_* */
    uint32_t solves;
    float R[9], t[3];      /* world -> camera */
    uint32_t pixels, no_depth, outside, no_model, too_far, angle, out_of_range, used;
    double H[36], b[6];
    adc_track_iteration iteration[ADC_TRACK_MAX_ITERATIONS_LIMIT];
    uint32_t reserved_[6];
} adc_track_result; /* 960 bytes */
int adc_track_device(adc_handle* h, const void* d_map, const void* d_frame_normals, const adc_tsdf_frame* frame,
                     const adc_tsdf_raycast_params* model_view, const void* d_model_depth, const void* d_model_normals,
                     const adc_track_params* params, void* d_result);
int adc_tsdf_track(adc_handle* h, const float* map, const adc_tsdf_frame* frame, const adc_track_params* params, adc_track_result* result);
int adc_get_track_result(adc_handle* h, adc_track_result* out);

/* -------------------------------------------------------------------------------------------
 * Stereo-aware TSDF fusion: a per-pixel observation weight, and an integrate that applies it and may read the map by a gated bilinear
 * interpolation (k_tsdf_fuse.hip; the rule is adcensus_amd/csrc/tsdf_fuse.h, tests/tsdf_fuse_ref.py holds the same definition in numpy
 * and the kernels match it bit for bit).  adc_tsdf_integrate* gives every observation the weight 1 and reads the nearest pixel, which
 * suits a time-of-flight map; a stereo map's depth error grows with Z^2, its filled pixels are guesses, and its disparity steps make
 * the nearest pixel a staircase.  Optional: nothing here changes what adc_tsdf_integrate* or any other entry point does.
 * All float arithmetic is IEEE binary32, one rounding per operation, nothing fused, parenthesised as written.
 *
 * Observation weights.  Output: uint8 [H][W] of the handle's geometry, a pure function of one pixel (a caller may as well supply a
 * weight map of their own to adc_tsdf_fuse*).  Inputs: the float32 [H][W] map with an adc_tsdf_frame, of which kind and calib are read
 * as adc_tsdf_integrate reads them (R, t must be finite and are not used); optional provenance (uint8 [H][W]) and confidence (float32
 * [H][W]) maps as adc_match_device_ex delivers them; adc_tsdf_weight_params (64 bytes): uint8 class_weight[4] indexed by ADC_FILL_*;
 * float min_confidence in [0, 1]; uint32 flags: ADC_TSDF_W_SCALE_CONFIDENCE; uint32 depth_power, 0, 2 or 4; float z_ref, finite and
 * > 0, in the unit of Z; uint32 reserved_[11] = 0.  NULL: class_weight {16, 4, 1, 0}, min_confidence 0, flags 0, depth_power 4, z_ref 1
 * (defaults of the interface, not measured optima).  For a pixel with map value v, code and conf:
 *   1. D = the Z of v by the frame's kind; a pixel without depth gets 0 (it is not `valid`).
 *   2. fill = (code >> ADC_PROV_FILL_SHIFT) & 3; without a provenance map fill = ADC_FILL_WTA.
 *   3. wc = class_weight[fill]; with a provenance map and (code & ADC_PROV_SPECKLE): wc = 0.
 *   4. with a confidence map and fill == ADC_FILL_WTA: if !(conf >= min_confidence) (a NaN fails): wc = 0, count below_confidence;
 *      otherwise, with ADC_TSDF_W_SCALE_CONFIDENCE: cq = (int)floorf(fminf(fmaxf(conf, 0.0f), 1.0f) * 256.0f + 0.5f);
 *      wc = (wc * cq + 128) >> 8.
 *   5. wc == 0 or D == +inf (an overflowing fb / s): 0.  Otherwise g = z_ref / D; s = (float)wc for depth_power 0, s = (float)wc *
 *      (g * g) for 2, s = (float)wc * ((g * g) * (g * g)) for 4; w = (int)floorf(fminf(s, 255.0f) + 0.5f).
 * Report (adc_tsdf_weight_report, uint32 each): valid (pixels with depth), nonzero (w > 0), below_confidence, saturated (w == 255),
 * four reserved words.
 *
 * Fuse.  adc_tsdf_fuse_params (32 bytes): uint32 flags: ADC_TSDF_FUSE_BILINEAR; float interp_gap, in the map's own unit (disparity or
 * depth as stored), finite and >= 0; uint32 reserved_[6] = 0.  NULL: no flag, interp_gap 0.  Steps 1 to 5 and 8 are those of
 * adc_tsdf_integrate; with x, y, u, v of its steps 4 and 5:
 *   6.  D = the Z of map[y][x] by the frame's kind; a pixel without depth: skip, count no_depth.
 *   6a. wo = weight[y][x], or 1 without a weight map; wo == 0: skip, count unweighted (nothing further is loaded).
 *   6b. only with ADC_TSDF_FUSE_BILINEAR: x0 = (int)floorf(u), y0 = (int)floorf(v).  The interpolation is used iff 0 <= x0 && x0 + 1 <
 *       W && 0 <= y0 && y0 + 1 < H (in integers, before any load); the raw values a = map[y0][x0], b = map[y0][x0+1], c = map[y0+1][x0],
 *       d = map[y0+1][x0+1] all have depth by the kind's rule; fmaxf(fmaxf(a, b), fmaxf(c, d)) - fminf(fminf(a, b), fminf(c, d)) <=
 *       interp_gap; and val has depth by the kind's rule, where fx = u - (float)x0, fy = v - (float)y0, top = a + fx * (b - a), bot = c +
 *       fx * (d - c), val = top + fy * (bot - top).  Then D = the Z of val and the voxel counts as interpolated (whatever step 7 then
 *       decides); otherwise D stays the nearest pixel's.  The raw values are interpolated: a disparity is affine in the pixel on a
 *       plane, so a plane comes back exactly up to rounding.
 *   7.  as adc_tsdf_integrate, on that D.
 *   9'. m = w + wo; t' = ((t + 32767) * w + (q + 32767) * wo + m / 2) / m - 32767 in non-negative 64-bit integers (the numerator can
 *       reach 65534 * 65535 + 65534 * 255 + 32895 > 2^32); w' = min(m, max_weight); count updated.  With wo == 1 this is step 9 bit for bit.
 *   10. colour as adc_tsdf_integrate: the nearest pixel (x, y), cm = cw + 1 whatever wo.
 * Report (adc_tsdf_fuse_report, uint32 each): in_frustum, no_depth, unweighted, occluded, updated, interpolated, two reserved words;
 * in_frustum = no_depth + unweighted + occluded + updated.  Without a weight map and without the flag the volume and the four common
 * counts equal those of adc_tsdf_integrate_device.
 *
 * adc_tsdf_weights_device   d_map 4-byte aligned; d_provenance, d_confidence (4-byte aligned) may be NULL; d_weight uint8 [H][W], any
 *                           alignment.  Needs no volume.  Asynchronous on the handle's stream, completed by adc_wait.
 * adc_tsdf_weights          the same with HOST pointers, synchronous; its device scratch is allocated on the first call.
 * adc_tsdf_fuse_device      as adc_tsdf_integrate_device with d_weight (uint8 [H][W], any alignment, or NULL: 1 everywhere) and params
 *                           (or NULL).  Asynchronous; calls may be enqueued back to back, behind adc_tsdf_weights_device and in
 *                           front of adc_tsdf_raycast_device / adc_track_device with one adc_wait.
 * adc_tsdf_fuse             the same with HOST pointers, synchronous.
 * adc_get_tsdf_fuse_report  the reports of the last completed fuse / weights call; either pointer may be NULL (not both); a report
 *                           that is asked for and does not exist yet is refused.
 * Return codes and refusals as for adc_tsdf_integrate_device (every refusal stands before the first HIP call), and: a bad field, flag
 * or reserved word of either params.
 * ------------------------------------------------------------------------------------------- */
#define ADC_TSDF_W_SCALE_CONFIDENCE 1u
#define ADC_TSDF_FUSE_BILINEAR 1u
typedef struct adc_tsdf_weight_params {
    uint8_t class_weight[4]; /* ADC_FILL_WTA, _VOTING, _INTERPOLATION, _NONE */
    float min_confidence;    /* [0, 1] */
    uint32_t flags;          /* ADC_TSDF_W_SCALE_CONFIDENCE */
    uint32_t depth_power;    /* 0, 2, 4 */
    float z_ref;             /* finite, > 0 */
    uint32_t reserved_[11];
} adc_tsdf_weight_params; /* 64 bytes */
typedef struct adc_tsdf_weight_report {
    uint32_t valid, nonzero, below_confidence, saturated;
    uint32_t reserved_[4];
} adc_tsdf_weight_report;
typedef struct adc_tsdf_fuse_params {
    uint32_t flags;          /* ADC_TSDF_FUSE_BILINEAR */
    float interp_gap;        /* finite, >= 0 */
    uint32_t reserved_[6];
} adc_tsdf_fuse_params; /* 32 bytes */
typedef struct adc_tsdf_fuse_report {
    uint32_t in_frustum, no_depth, unweighted, occluded, updated, interpolated;
    uint32_t reserved_[2];
} adc_tsdf_fuse_report;
int adc_tsdf_weights_device(adc_handle* h, const void* d_map, const void* d_provenance, const void* d_confidence, const adc_tsdf_frame* frame,
                            const adc_tsdf_weight_params* params, void* d_weight);
int adc_tsdf_weights(adc_handle* h, const float* map, const uint8_t* provenance, const float* confidence, const adc_tsdf_frame* frame,
                     const adc_tsdf_weight_params* params, uint8_t* weight, adc_tsdf_weight_report* report);
int adc_tsdf_fuse_device(adc_handle* h, const void* d_map, const void* d_bgr_left, const void* d_weight, const adc_tsdf_frame* frame,
                         const adc_tsdf_fuse_params* params);
int adc_tsdf_fuse(adc_handle* h, const float* map, const uint8_t* bgr_left, const uint8_t* weight, const adc_tsdf_frame* frame,
                  const adc_tsdf_fuse_params* params, adc_tsdf_fuse_report* report);
int adc_get_tsdf_fuse_report(adc_handle* h, adc_tsdf_fuse_report* fuse_report, adc_tsdf_weight_report* weight_report);

/* -------------------------------------------------------------------------------------------
 * Moving TSDF volume: the window shifts by whole voxels on the device, the origin moves along, and the surface points whose voxels
 * leave are handed out exactly once (k_tsdf_shift.hip; the rule is adcensus_amd/csrc/tsdf_shift.h, tests/tsdf_shift_ref.py holds the
 * same definition in numpy and the kernels match it byte for byte).  Optional: nothing of it exists before the first shift call, and
 * no other entry point changes -- every consumer reads the volume's origin, which is all a whole-voxel shift changes for them.
 *
 * Shift.  s = (sx, sy, sz) in voxels, any int32; the window moves by +s in the world.  New voxel (i, j, k) takes the voxel word (with
 * a colour volume also the colour word) of old voxel (i + sx, j + sy, k + sz) if that lies inside [0, nx) x [0, ny) x [0, nz);
 * otherwise both words become 0, the empty voxel.  An old voxel LEAVES iff (i - sx, j - sy, k - sz) lies outside the box.  Space that
 * re-enters the window is empty: what is fused there later is a new observation.
 *
 * Origin.  The handle keeps origin0, the origin given to adc_tsdf_create, and int32 offset[3], the sum of all shifts since
 * (adc_tsdf_create clears it, adc_tsdf_reset keeps it).  After a shift the volume's origin[a] = origin0[a] + (float)offset[a] * voxel:
 * binary32, one multiply and one add, nothing fused, from the TOTAL offset and never accumulated, so the rounding does not drift.
 * |offset[a]| stays <= 2^24 (the conversion is exact): a shift that would pass it is refused.  adc_tsdf_upload, adc_tsdf_download,
 * integrate, fuse, extract, mesh, ray cast and track behave as before, on the new origin.
 *
 * Leaving surface.  The crossings of adc_tsdf_extract's definition on the OLD volume (the min_weight gate, the pair a, b = a + 1 on
 * an axis, the record, computed with the OLD origin) for which a or b leaves, in the extraction's order (ascending n of a, then x, y,
 * z), cut by the capacity as extract cuts them; d_count (optional) receives the count.  Over a session each crossing is handed out at
 * most once: an edge with a leaving endpoint is emitted now, and the endpoint that stays then sits on the window's face without a
 * neighbour on that side; every other edge is still in the window, for a later shift or the final adc_tsdf_extract.
 *
 * A zero shift is valid: bits, device addresses and offset unchanged, a report of zeros, d_count = 0.  With |s_a| >= n_a on any axis
 * everything leaves: the list is the whole list of adc_tsdf_extract and the new volume is empty.
 *
 * Parameters (adc_tsdf_shift_params, 32 bytes): int32 shift[3]; uint32 min_weight in [1, 65535]; uint32 flags = 0; uint32
 * reserved_[3] = 0.  Report (adc_tsdf_shift_report, uint32 each): moved_nonempty (voxels that stayed and whose voxel word is not 0),
 * left_nonempty (leaving voxels whose voxel word is not 0), left_seen (leaving voxels with w >= min_weight), points (the leaving
 * list's length whatever the capacity), four reserved words.
 *
 * adc_tsdf_shift_device   d_points adc_point records, 16-byte aligned, or NULL with capacity 0 (counts only); d_count one uint32
 *                         device word, 4-byte aligned, or NULL.  Asynchronous on the handle's stream, completed by adc_wait; calls
 *                         may follow one another (and integrate / extract calls) without a wait.  The shift works out of place: the
 *                         first non-zero shift allocates a second plane of voxel words (and of colour words), which adc_tsdf_destroy,
 *                         adc_destroy and a replacing adc_tsdf_create free.  THE DEVICE ADDRESSES adc_tsdf_get_volume_device RETURNS
 *                         CHANGE WITH EVERY NON-ZERO SHIFT: ask again after each.
 * adc_tsdf_shift          the same with HOST pointers, synchronous; copies out min(points, capacity) records; points may be NULL
 *                         with capacity 0.  Its device scratch is that of adc_tsdf_extract and grows the same way.
 * adc_get_tsdf_shift_report  the report of the last completed shift call.
 * adc_tsdf_get_offset     the total offset and origin0; either out pointer may be NULL (not both).
 * adc_tsdf_follow_plan    PURE (no handle, no HIP): how far to shift so that a point of the camera frame stays near the volume's
 *                         centre.  params: the volume with its CURRENT origin; R, t: world -> camera as in adc_tsdf_frame;
 *                         adc_tsdf_follow_params (32 bytes): float anchor[3] in the camera frame (e.g. 0, 0, 2.5), int32 margin >= 0
 *                         and int32 quantum >= 1 in voxels, uint32 reserved_[3] = 0.  binary64, in this order: d = anchor - t;
 *                         A[a] = (R[0][a]*d[0] + R[1][a]*d[1]) + R[2][a]*d[2]; p = (A[a] - origin[a]) / voxel - n_a / 2;
 *                         shift[a] = quantum * trunc(p / quantum) if |p| > margin, else 0 (clipped to +-2^30).  With quantum <=
 *                         margin the plan that follows an applied shift is 0 on every axis (while |shift| * voxel is exact in
 *                         binary32), and the sign of a shift follows the anchor.
 * Return codes: 0; 1 before the first HIP call (a NULL argument, no volume, a bad field, flag or reserved word, a non-finite R, t or
 * anchor, an offset that would pass 2^24, a misaligned d_points or d_count, points NULL with a capacity, a Match pending); 2 on a HIP
 * failure: the volume, its origin and its offset are as before the call.  Not a product of adc_products or the farm.
 * ------------------------------------------------------------------------------------------- */
typedef struct adc_tsdf_shift_params {
    int32_t shift[3];
    uint32_t min_weight; /* [1, 65535] */
    uint32_t flags;      /* 0 */
    uint32_t reserved_[3];
} adc_tsdf_shift_params; /* 32 bytes */
typedef struct adc_tsdf_shift_report {
    uint32_t moved_nonempty, left_nonempty, left_seen, points;
    uint32_t reserved_[4];
} adc_tsdf_shift_report;
typedef struct adc_tsdf_follow_params {
    float anchor[3];     /* camera frame */
    int32_t margin;      /* >= 0, voxels */
    int32_t quantum;     /* >= 1, voxels */
    uint32_t reserved_[3];
} adc_tsdf_follow_params; /* 32 bytes */
int adc_tsdf_shift_device(adc_handle* h, const adc_tsdf_shift_params* params, void* d_points, uint64_t capacity, void* d_count);
int adc_tsdf_shift(adc_handle* h, const adc_tsdf_shift_params* params, adc_point* points, uint64_t capacity, adc_tsdf_shift_report* report);
int adc_get_tsdf_shift_report(adc_handle* h, adc_tsdf_shift_report* out);
int adc_tsdf_get_offset(adc_handle* h, int32_t offset[3], float origin0[3]);
int adc_tsdf_follow_plan(const adc_tsdf_params* params, const float R[9], const float t[3], const adc_tsdf_follow_params* follow_params,
                         int32_t shift_out[3]);

/* Stage timers (ms, HIP events on the handle's stream) of the most recent completed match.
 * Enable with adc_set_profiling(h,1).  Order: see adc_stage_name().
 * Level 2 records only the marks around the aggregation launches (adc_aggregate_info: the live duration of the roofline kernel) and
 * no stage marks -- every event record on the stream costs ~6 us of its time, ten of them 1.3 % of a 1080p Match (bench.py times its
 * region at level 2 and measures the stage times on extra Matches behind it). */
enum {
    ADC_STAGE_COST = 0,       /* gray + census + AD-census cost volume   (cost_computor.cpp)      */
    ADC_STAGE_ARMS,           /* cross arms + support counts             (cross_aggregator.cpp:76-86,271-325) */
    ADC_STAGE_AGGREGATE,      /* 4 iterations x (H,V) passes             (cross_aggregator.cpp:89-118) */
    ADC_STAGE_SCANLINE,       /* 4 chained DP passes                     (scanline_optimizer.cpp:40-61) */
    ADC_STAGE_WTA,            /* left + right WTA / sub-pixel            (ADCensusStereo.cpp:188-310) */
    ADC_STAGE_REFINE,         /* LR check, region voting, interpolation, [DDA], median (multistep_refiner.cpp:60-87) */
    ADC_STAGE_COUNT
};
const char* adc_stage_name(int stage);
void adc_set_profiling(adc_handle* h, int on);
int adc_get_stage_ms(adc_handle* h, float* ms, int n);
/* Per-kernel-launch average of the aggregation pass kernel over the last match (ms), and the
 * number of launches it averaged (8 for 4 iterations). */
int adc_get_aggregate_pass_ms(adc_handle* h, float* avg_ms, int* launches);
/* The same average with what it covers: number of REGULAR aggregation launches of the last match (the first pass is
 * left out when it computed the matching cost itself: first_fused = 1, write-only), and the number of algorithmic
 * passes (cross_aggregator.cpp:100-118, two per iteration) those launches covered -- a pass-pair launch covers two. */
int adc_get_aggregate_info(adc_handle* h, float* avg_launch_ms, int* launches, int* passes, int* first_fused);
/* Name of the kernel family the last regular aggregation launch of the handle used (static string, "" before the first Match). */
const char* adc_get_aggregate_kernel(adc_handle* h);

/* OPT-IN paper modes: features of the AD-Census paper the reference declares or stores but does not
 * implement.  Default 0 = exactly the reference.  Any other value changes the results BY DEFINITION (no parity with the
 * reference; checked against the test suite's own plain-C restatement of the same definitions).  Functional, not tuned.
 *   ADC_PAPER_CENSUS5X5   5x5 census window (adcensus_types.h:39-42, CensusSize::Census5x5, declared / unimplemented)
 *   ADC_PAPER_SO_SUM      the four scanline paths computed independently and averaged (paper eq. 10) instead of chained
 *                         (scanline_optimizer.cpp:54-60)
 *   ADC_PAPER_RIGHT_ARMS  support regions limited by the arms of BOTH images (cross_aggregator.h:91 stores img_right_, unused)
 * Call between matches (not while one is in flight).  Returns 0, 1 on bad arguments, 2 on an allocation failure. */
#define ADC_PAPER_CENSUS5X5 1u
#define ADC_PAPER_SO_SUM 2u
#define ADC_PAPER_RIGHT_ARMS 4u
int adc_set_paper_modes(adc_handle* h, uint32_t modes);

/* Print the reference's six timing lines from Match (ADCensusStereo.cpp:88-129); default off. */
void adc_set_verbose(adc_handle* h, int on);

/* Plumbing for callers that own device memory / streams elsewhere (e.g. torch). */
void* adc_get_stream(adc_handle* h);                 /* hipStream_t as void* */
int   adc_device_synchronize(void);
void* adc_device_malloc(size_t bytes);
void  adc_device_free(void* p);
int   adc_memcpy_h2d(void* dst, const void* src, size_t bytes);
int   adc_memcpy_d2h(void* dst, const void* src, size_t bytes);
/* Measured device-to-device copy time of `bytes` bytes (hipMemcpyAsync on the null stream, best of `reps`), in ms;
 * negative on error.  bench.py reports 2*bytes/time next to the 8 TB/s peak: the practical HBM ceiling of this device
 * for a pass that reads one volume and writes another. */
double adc_device_copy_ms(void* dst, const void* src, size_t bytes, int reps);
/* the same with a float4 grid-stride copy KERNEL (the hardware guide's yardstick shape), best of a few grid sizes; -1 on error */
double adc_device_copy_kernel_ms(void* dst, const void* src, size_t bytes, int reps);

/* -------------------------------------------------------------------------------------------
 * Test-only debug surface (parity tests drive single stages with oracle-provided inputs).
 * Volumes cross this boundary in the REFERENCE layout [H][W][D] float32 (D = max-min disparity);
 * the padded internal layout is private.
 * ------------------------------------------------------------------------------------------- */
enum {
    ADC_BUF_GRAY_LEFT = 0,    /* u8  [H][W]                                                    */
    ADC_BUF_GRAY_RIGHT,       /* u8  [H][W]                                                    */
    ADC_BUF_CENSUS_LEFT,      /* u64 [H][W]                                                    */
    ADC_BUF_CENSUS_RIGHT,     /* u64 [H][W]                                                    */
    ADC_BUF_ARMS,             /* u8  [H][W][4] = left,right,top,bottom (CrossArm, cross_aggregator.h:17-20) */
    ADC_BUF_SUPCOUNT_H,       /* u16 [H][W]  horizontal-first support count (vec_sup_count_[0]) */
    ADC_BUF_SUPCOUNT_V,       /* u16 [H][W]  vertical-first support count   (vec_sup_count_[1]) */
    ADC_BUF_VOLUME_A,         /* f32 [H][W][D]  the volume holding the latest stage result      */
    ADC_BUF_DISP_LEFT,        /* f32 [H][W]  current left disparity map                         */
    ADC_BUF_DISP_RIGHT,       /* f32 [H][W]                                                     */
    ADC_BUF_OUTLIER_LABEL,    /* u8  [H][W]  0 valid, 1 mismatch, 2 occlusion                   */
    ADC_BUF_COUNT
};
/* Copies a device buffer to host (de-padding volumes). dst must hold the full buffer. */
int adc_debug_read(adc_handle* h, int which, void* dst);
/* Overwrites a device buffer from host (padding volumes). */
int adc_debug_write(adc_handle* h, int which, const void* src);
/* The padded code maps the interpolation's table walk reads (one byte per pixel: 255 valid, 254 outside the image, else the steps a
 * ray may skip behind this pixel), as the last ADC_RUN_INTERPOLATION or Match left them.  Geometry: `pitch` bytes per row, `rows`
 * rows, the image's column 0 at padded column `gx`, its row 0 at row 0.  pass 0 = the mismatch list's map, 1 = the occlusion list's;
 * dst holds pitch * rows bytes.  Both return 1 on a handle that has no code maps (its search range or width rules the table walk out). */
int adc_debug_itp_code_geometry(adc_handle* h, int* pitch, int* rows, int* gx);
int adc_debug_read_itp_code(adc_handle* h, int pass, void* dst);
/* Uploads the image pair without running anything. */
int adc_debug_set_images(adc_handle* h, const uint8_t* bgr_left, const uint8_t* bgr_right);

enum {
    ADC_RUN_GRAY_CENSUS = 0,  /* images -> gray, census                                        */
    ADC_RUN_COST,             /* images, census -> VOLUME_A                                    */
    ADC_RUN_ARMS,             /* left image -> arms, support counts                            */
    ADC_RUN_AGGREGATE,        /* VOLUME_A, arms, counts -> VOLUME_A (4 iterations)             */
    ADC_RUN_SCANLINE,         /* VOLUME_A, images -> VOLUME_A (4 passes)                       */
    ADC_RUN_WTA,              /* VOLUME_A -> DISP_LEFT, DISP_RIGHT                             */
    ADC_RUN_LRCHECK,          /* DISP_LEFT, DISP_RIGHT -> DISP_LEFT, OUTLIER_LABEL             */
    ADC_RUN_REGION_VOTING,    /* DISP_LEFT, OUTLIER_LABEL, arms -> DISP_LEFT                   */
    ADC_RUN_INTERPOLATION,    /* DISP_LEFT, OUTLIER_LABEL, left image -> DISP_LEFT             */
    ADC_RUN_DISCONTINUITY,    /* DISP_LEFT, VOLUME_A -> DISP_LEFT                              */
    ADC_RUN_MEDIAN,           /* DISP_LEFT -> DISP_LEFT (in-place semantics)                   */
    ADC_RUN_COUNT
};
/* Runs ONE stage on the handle's current device buffers and synchronizes. `arg` is stage
 * specific (ADC_RUN_AGGREGATE: number of iterations, 0 -> 4, +100 fused cost, +200 host-chosen
 * ring / pass pairs; ADC_RUN_SCANLINE: number of chained passes 1..4, 0 -> 4, +100 = the
 * production form whose last pass also writes DISP_LEFT (the fused left-view winner-takes-all);
 * ADC_RUN_MEDIAN: 100 = do not run, arm the fallback path of the next adc_wait (single-workgroup kernel); 101 = the same as if
 * a seam of the speculative bands had differed (the chained form of the banded kernel is redone);
 * ADC_RUN_INTERPOLATION: 1 = this run takes the double-precision ray walk also where the handle would walk the integer ray table
 * (the walk of handles whose search range or padded width rules the table out); else ignored). */
int adc_debug_run(adc_handle* h, int stage, int arg);
/* Test-only event counters of the handle: which = 0 -> number of times adc_wait had to redo the median filter with the
 * single-workgroup kernel (hand-off time-out of the banded kernel); 1 -> continuations of the voting chain (launch budget
 * too small); 2 -> aggregation redos (assumed ring depth too small); 3 -> launch budget (kernels) of the next Match's
 * voting chain; 4 -> Matches redone because a scanline row segment failed its seam check, 5 -> segments per row of the last
 * scanline run, 6 -> seams that failed in it; 7 -> speculative median seams that differed, 8 -> the last median used speculative
 * bands; 9 -> consecutive Matches that needed different aggregation plans (short-arm / long-arm image), 10 -> Matches whose
 * aggregation was enqueued as two plans (the device chose), 11 -> redos that restarted at the aggregation, 12 -> Matches for which
 * both plans will still be enqueued, 13 -> Matches whose last aggregation pass ran inside the first scanline pass (the fused tail of
 * short-arm images, k_scanline_seg_agg), 14 -> the voting chain's band -> XCD sweep is in use (0: the device's workgroup -> XCD
 * mapping is not the assumed round-robin, plain schedule), 15 -> column segments per band link of the last banded median launch (1:
 * whole rows -- odd widths, the chained form, or a segment seam failed within the last 64 Matches).  ADC_RUN_REGION_VOTING of adc_debug_run takes the budget of that run as `arg` (0 = keep;
 * arg < 0: run nothing, set the budget of the NEXT Match's chain to -arg). */
int64_t adc_debug_counter(adc_handle* h, int which);
/* Statistics of the last region-voting run: rounds of the fixed-point iteration (all ten passes of the reference iterate at
 * once since round 5) and total vote evaluations. */
int adc_debug_voting_stats(adc_handle* h, int64_t* rounds, int64_t* evaluations);

#ifdef __cplusplus
}
#endif
#endif /* ADCENSUS_C_API_H_ */
