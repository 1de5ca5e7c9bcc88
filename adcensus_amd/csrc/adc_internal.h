// adc_internal.h -- private state of an adc_handle and the kernel-launch entry points.  Which kind of state lives where (parameters,
// resources, set-call configuration, learned, in flight, observations of the last run): DESIGN.md, "Kinds of handle state".
//
// Memory.  Every device and pinned buffer of a handle is one of the pointer fields below, allocated through dev_mem.h, the only owner:
// capi.hip calls it (no k_*.hip file allocates or frees handle state), the handle's registry `mem` knows which fields own memory, and
// adc_destroy releases exactly that registry.  adc_create allocates what every Match needs (alloc_all: images, per-pixel maps, volumes,
// tables, refinement state, pin_in / pin_out / pin_flags; upload_tables: ray_tab).  Everything optional is allocated by the first call
// that needs it and kept until adc_destroy: out_words, map_buf[], os_cloud (products); sp_* (speckle filter); rect[], pin_raw
// (rectification, raw formats); ev_*, evs_* (evaluation); reg_*, regs_* (registration); nrm_*, nrms_* (surface normals); msh_*, mshs_* (triangle mesh); tsdf_*, tsdfs_* (TSDF volume: adc_tsdf_create and the first calls of its entry points); vox_* (voxel grid); arms_r, bgrx_r, armmax_r, vol_c (paper modes).
// os_cloud, the raw buffers, ev_raw, reg_zbuf and the target-sized regs_* grow with the largest size asked for; their capacities count
// elements of the field's own type.
//
// HBM layout of the buffers of adc_create (288 GB HBM3E is plentiful):
//   img_l / img_r      u8  [H][W][3]  BGR, as handed over by the caller
//   gray_l / gray_r    u8  [H][W]
//   census_l/census_r  u64 [H][W]
//   arms               u8x4[H][W]     left,right,top,bottom
//   sup_h / sup_v      u16 [H][W]     support counts of the H-first / V-first iterations
//   cdiff_*            u8  [H][W]     max-channel colour difference to the left / upper neighbour of
//                                     the left (L) and right (R) image (scanline penalties)
//   vol_a / vol_b      f32 [H][W][Dp] cost volumes (ping-pong).  d innermost, Dp = 64*VPL, VPL in
//                                     {1,2,4}: lanes = disparities, lane l holds d = l*VPL .. l*VPL+VPL-1.
//                                     d >= D are padding (never read by a reduction).
//   disp_l / disp_r    f32 [H][W]
//   label              u8  [H][W]     outlier class (0 valid, 1 mismatch, 2 occlusion)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <type_traits>

#include "../../include/adcensus_c_api.h"
#include "learn_plan.h"
#include "agg_plan.h" // AggArms
#include "dev_mem.h"
#include "voxel_point.h" // VoxGrid

#define ADC_WAVE 64

// Streaming hint for the volume accesses (every element is read once and written once per pass; 1 GB >> every cache):
// the loads / stores of the marching kernels (K4, K5, K6) are marked non-temporal: same-box A/B at 1080p, K4 launch 0.394 -> 0.376 ms
// (0.462 -> 0.445 in the slower clock state of the same box), scanline stage -1 %, right-view WTA -4 % (profiles/r5_ab_nontemporal.txt);
// -DADC_VOL_NT=0 switches it off (tools/build_variant.sh).
#if !defined(ADC_VOL_NT) || ADC_VOL_NT
#define ADC_VOL_NT_STR " nt"
#define ADC_VOL_STORE(PTR, VAL) __builtin_nontemporal_store((VAL), (PTR))
#else
#define ADC_VOL_NT_STR ""
#define ADC_VOL_STORE(PTR, VAL) (*(PTR) = (VAL))
#endif


// Fault injection -- TEST BUILDS ONLY.  libadcensus_hip_faultinj.so (csrc/Makefile, target faultinj) is capi.hip compiled with
// -DADC_FAULT_INJECTION=1 and linked with the product's kernel objects; the product library never defines it.  There every HIP
// call of capi.hip's object-lifetime and Match path goes through ADC_HIP(call): the n-th one (ADC_TEST_FAIL_AT=<n> in the
// environment, or adc_test_fail_at(n)) is NOT executed and reports hipErrorOutOfMemory -- the reference's contract for that is
// `return false` (ADCensusStereo.cpp:31-40,71-76; SURVEY.md 8b "HIP failure -> false").  tests/test_gpu_faults.py.
#ifdef ADC_FAULT_INJECTION
extern "C" int adc_test_fault_now(void);
#define ADC_HIP(call) (adc_test_fault_now() ? hipErrorOutOfMemory : (call))
#else
#define ADC_HIP(call) (call)
#endif

struct AdcParams {
    int W, H;
    int dmin, dmax, D; // D = dmax - dmin
    int VPL;           // disparities per lane (1,2,4,8,16)
    int Dp;            // padded disparity count = 64*VPL
    adc_option opt;
};

// The outputs computed from the final map (k_outputs.hip), validated and resolved to device addresses: part of a Match's request,
// or the whole request of adc_reproject_device
struct AdcOutReq {
    int active;           // kept until adc_wait, so that its redos (which call enqueue_output again) rewrite the outputs
    int calibrated;       // calib holds the caller's calibration, fb = focal_px * baseline (one f32 multiply on the host)
    adc_calib calib;
    float fb;
    float* depth;         // device addresses; NULL = not requested
    void* cloud;
    uint32_t capacity;    // points the cloud buffer holds
    uint32_t* cloud_count;
    uint8_t* disp8;
};

// The optional map products of a Match, in the order of every per-map table (AdcMatchReq::host, adc_handle::map_buf)
enum { ADC_MAP_PROV, ADC_MAP_CONF, ADC_MAP_DEPTH, ADC_MAP_DISP8, ADC_MAP_DISP16, ADC_REQ_MAPS };
struct AdcHostMap {
    void* dst;         // the caller's host buffer; NULL = not requested
    size_t bytes;
    int direct;        // 0 = via pinned staging + host copy in adc_wait, 1 = dst lies in a registered range: the stream writes it in place,
                       // 2 = blocking copy by adc_wait from the device scratch (adc_match_ex, adc_match_out)
};
// Everything the Match in flight was asked for; all zero = idle (match_req_clear).  Every entry point is a view of this one
// request: the kernels write the device targets (the caller's device buffers, or for host callers the handle's map_buf scratch),
// enqueue_output sends every host map behind them to its pinned staging block (or straight into a destination the caller has
// registered), adc_wait copies staging -> caller (adc_match_ex, adc_match_out: device scratch -> caller, blocking) and, once the count
// is known, the first min(count, capacity) points of the cloud.
// Kept until adc_wait, so that its redos write and send everything again.
struct AdcMatchReq {
    float* map_host;      // the disparity map: a host destination ...
    int map_host_direct;  // 0 = via pin_out + host copy, 1 = DMA into the caller's page-locked map, 2 = pageable copy by adc_wait (ADC_HOST_DIRECT)
    void* map_dev;        // ... or the caller's device buffer (re-filled by the median fallback)
    uint8_t* prov;        // device targets of the provenance / confidence / 16-bit maps; NULL: not requested
    float* conf;
    uint16_t* disp16;
    float disp16_scale;
    AdcOutReq out;        // depth / cloud / 8-bit image (out.active)
    int host_delivery;    // a host caller asked for products: the table below says where adc_wait delivers them
    AdcHostMap host[ADC_REQ_MAPS];
    adc_point* cloud;     // host
    uint32_t capacity;
    uint32_t* cloud_count; // host word, written at delivery
};
// what a host caller's map product goes through, each allocated by the first call that needs it
struct AdcMapBuf {
    void* dev;         // device scratch the kernels write
    void* pin;         // pinned staging of the asynchronous delivery (none while no destination needed it)
};
// Everything IN FLIGHT on a handle: what the next adc_wait has to settle, or the next stage of the same Match consumes.  All zero =
// idle: a successful adc_wait leaves every byte zero, a failed call gets there by the ONE reset of abort_match (a memset of the struct:
// a member added here cannot be forgotten on the failure path).  Each member is written by whom its comment names first and
// consumed (put back to 0) by whom it names behind "->".
struct AdcInFlight {
    int match_pending;    // run_heavy: a Match was enqueued -> adc_wait, once it has looked at its arm maxima / speculation flags
    int irv_pending;      // adc_run_region_voting: a chain was enqueued -> adc_voting_finish (adc_wait), which looks at its final state
    int so_agg_fused;     // adc_launch_aggregate left its last pass to the scanline stage: vol_a holds the volume BEFORE that pass -> run_so
    int wta_left_done;    // run_so: the last scanline pass also wrote the left-view map -> adc_launch_wta, which then only runs the right view
    bool timings_pending; // run_pipeline: profiling marks were recorded -> collect_timings (adc_wait)
    int force_median_fallback; // test hook (adc_debug_run ADC_RUN_MEDIAN 100 / 101): the next adc_wait takes the fallback path -> adc_wait
    int ev_pending;       // adc_evaluate_device: an evaluation was enqueued -> adc_wait moves ev_pin and ev_echo into ev_report
    int reg_pending;      // adc_register_depth_device: a registration was enqueued -> adc_wait moves reg_pin into reg_report
    int nrm_pending;      // adc_normals_device: a normals kernel was enqueued -> adc_wait moves pin_flags[ADC_PIN_NORMALS..] into nrm_report
    int msh_pending;      // adc_mesh_device: a mesh was enqueued -> adc_wait moves pin_flags[ADC_PIN_MESH..] into msh_report
    int tsdf_pending;     // adc_tsdf_integrate_device: a frame was enqueued -> adc_wait moves pin_flags[ADC_PIN_TSDF..] into tsdf_report
    int tsdfx_pending;    // adc_tsdf_extract_device: an extraction was enqueued -> adc_wait moves pin_flags[ADC_PIN_TSDF_EXTRACT..] into tsdf_xreport
    int tsdfr_pending;    // adc_tsdf_raycast_device: a ray cast was enqueued -> adc_wait moves pin_flags[ADC_PIN_TSDF_RAY..] into tsdf_rreport
    int track_pending;    // adc_track_device: a track was enqueued -> adc_wait moves the pinned record track_pin into track_result
    int tsdff_pending;    // adc_tsdf_fuse_device: a frame was enqueued -> adc_wait moves pin_flags[ADC_PIN_TSDF_FUSE..] into tsdf_freport
    int tsdfw_pending;    // adc_tsdf_weights_device: a weight map was enqueued -> adc_wait moves pin_flags[ADC_PIN_TSDF_WEIGHT..] into tsdf_wreport
    int tsdfh_pending;    // adc_tsdf_shift_device: a shift was enqueued -> adc_wait moves pin_flags[ADC_PIN_TSDF_SHIFT..] into tsdf_sreport
    int tsdfm_pending;    // adc_tsdf_mesh_device: a mesh of the volume was enqueued -> adc_wait moves pin_flags[ADC_PIN_TSDF_MESH..] into tsdf_mreport
    AdcMatchReq req;      // the request resolver / the entry points: what the Match in flight was asked for -> adc_wait (match_req_clear)
};
static_assert(std::is_trivially_copyable<AdcInFlight>::value, "AdcInFlight is reset with memset");

// One side of the optional rectification (k_rectify.hip): the declared geometry of the raw images, and what the set call made of
// the maps.  The [H][W] buffers are allocated by the first set call of a handle (both sides at once), the raw buffer grows with the
// largest geometry declared; adc_destroy frees them.
struct AdcRectSide {
    int set;              // a set call has succeeded for this side: 1 with maps, 2 conversion only (adc_set_input_format);
                          // adc_clear_rectify / a failed set call: 0
    adc_raw_format fmt;   // as declared: .format may carry the significant bits (ADC_PIX_BITS)
    uint32_t* rec;        // uint2 per destination pixel: {xi | yi << 16, ax | ay << 8 | flags << 16}
    float *mx, *my;       // the float maps (the caller's, or the model's): adc_get_rectify_maps
    uint8_t* valid;       // 1 where every tap with a nonzero weight lies inside the source
    uint8_t* raw;         // device copy of the raw image of the host entry points
    size_t raw_cap;       // bytes raw holds
};

#define ADC_PIN_ARM 64 // pin_flags[ADC_PIN_ARM + i] = armmax[i] of the last Match (one copy at the end of the heavy stream)
#define ADC_PIN_MEDIAN 0   // error flag of the banded median's hand-off (k_refine.hip)
#define ADC_PIN_CLOUD 8    // point count of the last cloud (k_outputs.hip): adc_get_cloud_count
#define ADC_PIN_SPECKLE 9  // three stat words of the last speckle filter run (k_speckle.hip): adc_get_speckle_stats
#define ADC_PIN_VOXEL 12   // voxels, points_valid, points_kept of the last voxel cloud (k_voxel.hip): adc_get_voxel_report
#define ADC_PIN_MESH 1     // lattice_valid, vertices, triangles, cells_two, cells_one of the last mesh call (k_mesh.hip): adc_get_mesh_report
#define ADC_PIN_VOTING 16  // eight state words of the voting chain, read back behind every chain (k_voting.hip: adc_run_region_voting, adc_voting_finish)
#define ADC_PIN_IRV_COLD 32 // staging of the voting chain's cold block, two slots of 16 words (k_voting.hip)
// behind the mirror of the armmax words (ADC_PIN_ARM + ADC_ARMMAX_WORDS, adc_device_fn.h), where no Match writes: a Match may be enqueued
// behind a pending TSDF call and one adc_wait completes both
#define ADC_PIN_TSDF (ADC_PIN_ARM + ADC_ARMMAX_WORDS) // in_frustum, no_depth, occluded, updated of the last integrate call (k_tsdf.hip): adc_get_tsdf_report
#define ADC_PIN_TSDF_EXTRACT (ADC_PIN_TSDF + 4)       // voxels_seen, points of the last extract call
#define ADC_PIN_TSDF_MESH (ADC_PIN_TSDF + 8)          // voxels_seen, vertices, triangles, cells_seen, cells_surface of the last TSDF mesh call
#define ADC_PIN_TSDF_RAY (ADC_PIN_TSDF + 16)          // rays, the five status counts, the 64-bit sample count of the last ray cast
#define ADC_PIN_TSDF_FUSE (ADC_PIN_TSDF + 24)         // in_frustum, no_depth, unweighted, occluded, updated, interpolated of the last fuse call (k_tsdf_fuse.hip)
#define ADC_PIN_TSDF_WEIGHT (ADC_PIN_TSDF + 32)       // valid, nonzero, below_confidence, saturated of the last weights call
#define ADC_PIN_TSDF_SHIFT (ADC_PIN_TSDF + 40)        // moved_nonempty, left_nonempty, left_seen, points of the last shift call (k_tsdf_shift.hip)
#define ADC_PIN_WORDS (ADC_PIN_TSDF + 48)             // int32 words of pin_flags
#define ADC_PIN_NORMALS 24 // usable, fitted, few_points, degenerate of the last normals call (k_normals.hip): adc_get_normals_report
struct adc_handle {
    AdcParams p;
    int device;
    DevMemOwner mem;    // which of the pointer fields below own device / pinned memory (dev_mem.h)
    hipStream_t stream; // per-object stream: uploads, refinement (latency-bound kernels), downloads
    hipStream_t heavy;  // bandwidth lane: cost/arms/aggregate/scanline/WTA kernels.  Shared by all objects of a
                        // device (FIFO), so the streaming kernels of different pairs never fight for HBM while
                        // the latency-bound refinement of one pair overlaps the streaming phase of the next
    hipEvent_t ev_in, ev_heavy_done;
    bool own_stream;

    // images + per-pixel maps
    uint8_t *img_l, *img_r;         // the pair being matched: the handle's own buffers, or the caller's (adc_match_device)
    uint8_t *img_l_own, *img_r_own;
    int bgrx_valid;                 // cache tag of the pair: bgrx_l holds its packed left image (written by the arms stage); capi.hip: images_own
    uint8_t *gray_l, *gray_r;
    uint64_t *census_l, *census_r;
    uint8_t* arms;
    uint16_t *sup_h, *sup_v;
    int* armmax;             // [0] max horizontal arm, [1] max vertical arm of the current left image, [2] failed seams, [3] ring too
                             // shallow, [ADC_NZ_BASE..] sharded record densities (ADC_ARMMAX_WORDS words, adc_device_fn.h)
    uint32_t *rec_h, *rec_v; // packed {arm_lo, arm_hi, divisor} per pixel, line-major (rec_v transposed)
    uint32_t *rec2_h, *rec2_v; // uint2 {arm_lo | span<<8 | divisor<<16, RN(1/divisor)}: records of the register-ring kernels
    float* agg_sink;           // 256 KiB scratch: store target of the halo steps of a pass pair (k_aggregate_rr.h)
    uint8_t *cdiff_lh, *cdiff_lv, *cdiff_rh, *cdiff_rv;
    uint8_t* so_cls; // path-ordered left-image colour-step words (d1) of the 4 scanline pass types (k_scanline.hip)
    float* so_seam;  // seam slots of the row passes cut into verified segments: [2 passes][H][ADC_SO_MAX_SEG - 1][Dp] (k_scanline.hip)
    // What the handle has learned from its earlier Matches, and the counters of the rules that move it (learn_plan.h: the only
    // file that assigns a member of `learned`, but for adc_create and the two budget hooks of adc_debug_run)
    AdcLearned learned;
    AdcLearnStats lstats;
    AdcInFlight fly;      // what is in flight; all zero = idle.  Below: what the stage run last did (adc_wait's AdcMatchReport, with pin_flags)
    int irv_chain;        // kernels of the chain enqueued so far (continuation starts here)
    int so_nseg_last;     // segments per row of the last scanline run (1 = whole rows)
    int med_spec_last;    // the last banded median launch used speculative bands
    int med_seg_last;     // ... and this many column segments per band link
    // volumes
    float *vol_a, *vol_b;
    // host-built tables: same libm as the CPU reference
    float* lut_ad;      // [766] A[k] = (1 - expf(-(k/3.0f)/lambda_ad)) + 1
    float* lut_census;  // [64]  C[h] = expf(-(float)h/lambda_census)
    double* ray_sincos; // [16][2] (sin, cos) of the 16 interpolation angles
    float so_P1[3], so_P2[3]; // penalty classes (p, p/4, p/10)
    // disparity maps and refinement state
    float *disp_l, *disp_r, *disp_tmp;
    uint8_t* label;
    uint8_t* elig;       // scratch: invalid mask of the LR check (byte per pixel), then the voting chain's bitmap of the pixels on its work list
    uint8_t* irv_bbox;   // uchar4 per pixel: widest H arms {left, right} over ALL region rows (k_sup_counts): read box / dirty box of a vote
    int32_t* vote_list;  // work list of the voting chain: int4 entries, one segment per workgroup in evaluation order (irv_plan.h)
    int32_t* vote_evals_arr; // evaluation counter per wave of the chain's grid (statistics), then the entries per workgroup segment
    int32_t* interp_list;     // target list of the interpolation (its own buffers: the voting chain may be CONTINUED after
    int32_t* interp_counters; // the interpolation has run once, and must find its list and control block untouched)
    int32_t* ray_tab;     // [max_search][16] packed ray offsets (dy<<16 | dx&0xffff), NULL when a step is too close to a .5 tie
    int ray_tab_rows;
    int32_t* ray_lin;     // [max_search + ADC_ITP_LPAD][16] linear ray offsets dy * itp_pitch + dx into the padded code map (same allocation as ray_tab)
    int itp_pitch, itp_ms; // row pitch of the code map and the search range it is padded for (adc_device_fn.h); pitch 0: no table walk on this handle (itp_plan.h)
    uint32_t* cost_rrec;  // [H][rrec_pitch] uint4 {bgrx, census lo, census hi, 0} of the RIGHT image, padded with out-of-image
                          // markers (bgrx = ~0) on both sides; cost_lrec [H][W] the same for the LEFT image (fused cost, k_aggregate.hip)
    uint32_t* cost_lrec;
    int rrec_pitch, rrec_padl;
    // Streams that alternate between short-arm and long-arm images: instead of assuming ONE ring depth and redoing the
    // Match when it is wrong, the aggregation is enqueued as TWO plans (assumed small rings + pass pairs | full ring) and the
    // kernels decide on the device which plan works (agg_gate_skip, k_aggregate_rr.h).
    int agg_dual_last;    // the last aggregation run enqueued both plans (per-launch timings are then not separable)
    int agg_first_fused;  // the last aggregation run did so (pass timings: the regular passes are 1..)
    int agg_dual_runs;    // Matches whose aggregation was enqueued as two plans
    int agg_so_fusions;   // Matches whose last aggregation pass ran inside the first scanline pass
    // Sparse small-ring launches (k_aggregate.hip): chosen per direction from the density of pass-changing records the handle
    // last saw (k_make_records counts them behind the arm maxima; they reach the host like the maxima do)
    int32_t* pin_nz;      // the sharded density words of the last Match inside pin_flags (pin_flags + ADC_PIN_ARM + ADC_NZ_BASE; ADC_NZ_*: adc_device_fn.h)
    int agg_sparse_last;  // the last aggregation run used sparse launches (pass timings are then not priced as read V + write V)
    int agg_sparse_launches; // sparse launches of this handle
    int agg_gather_launches; // ... of which in the gather form (k_agg_gather: only the changed pixels are computed)
    int agg_flat_launches;   // first (fused-cost) launches that ran as the element-wise k_cost_agg_flat instead of the small-ring march
    float* med_hand;      // banded median: per-band hand-off rows [bands][med_hpitch], indexed by wavefront level
    int med_hpitch;
    float* med_sink;      // banded median: 16-byte store sink per lane of every wave (bands + speculative copies)
    int32_t* pin_flags;   // pinned host word: error flag of the banded median's hand-off (read back after every Match)
    uint32_t* bgrx_l;     // left image packed B | G<<8 | R<<16 per pixel (interpolation gathers)
    uint16_t* st16;      // region voting: 16-bit state map [H][st16_pitch] {bin:11 | iteration of the fill:3 | list:2} (irv_plan.h)
    int st16_pitch;      // row pitch of st16 in elements (multiple of 8: rows start 16-byte aligned)
    float* disp_vote;    // the map the voting chain works on (copy of the LR-checked map, copied back when the chain ends)
    int irv_xcd_mode;    // 1: the chain's work list uses the band -> XCD sweep layout (the device's workgroup -> XCD mapping was probed)
    int irv_grid;        // workgroups of the voting chain (adc_irv_grid, fixed per handle: the work-list layout depends on it)
    float *tail_disp_l, *tail_disp_tmp; // buffer roles at the start of the stages behind the voting (for a redo)
    void* irv_cold;                  // device block of the chain's rarely used kernel arguments (64 bytes)
    unsigned char irv_cold_host[64]; // the block as it was last sent (k_voting.hip: IrvCold; staged through pin_flags[32..63])
    int irv_cold_valid, irv_cold_flip;
    int32_t* vote_counters; // voting chain control block (state slots + accumulator ring), median progress words at [160..]
    uint32_t* irv_px;    // per-pixel change bitmap of the voting rounds, IRV_PX_PLANES planes (slack budgets, irv_plan.h)
    uint8_t* chg_a;      // change-tile map of the voting rounds: one byte stamp per 8x8 tile, row pitch chg_pitch
    int chg_pitch;
    uint8_t* edge;       // discontinuity adjustment edge mask
    uint8_t* itp_cells;  // interpolation: 3 byte maps of 2x2-pixel cells (cell has a valid pixel / row distance / Chebyshev distance
                         // in cells to the nearest cell with a valid pixel): empty-space skipping of the ray walk (k_refine.hip);
                         // behind them the padded code map of the walk (adc_device_fn.h: ADC_ITP_VALID ...)
    // pinned staging for adc_match / adc_match_async
    uint8_t* pin_in;  // 2 * 3*W*H
    float* pin_out;   // W*H
    AdcMapBuf map_buf[ADC_REQ_MAPS]; // scratch and staging of the host callers' map products
    uint32_t* out_words;  // device scratch of k_outputs.hip (min / max words, count, tile counts), allocated on first use
    void* os_cloud;       // device scratch of the host callers' cloud; grows with the largest capacity asked for
    size_t os_cloud_cap;  // points os_cloud holds
    // optional speckle filter (k_speckle.hip; off = sp_max_size <= 0: nothing of it is enqueued)
    int32_t sp_max_size;  // handle state (adc_set_speckle_filter): every later Match filters its delivered map
    float sp_max_diff;
    int32_t* sp_parent;   // device scratch, allocated on first use: parent [P], size [P], then the three stat words
    float* sp_map;        // the filtered map of a Match (out of place: a redo of adc_wait may patch disp_l only in part)
    // optional voxel-grid filter of the cloud (k_voxel.hip; off = vox_set 0: the cloud's own kernels run, nothing of this is enqueued)
    int vox_set;          // handle state (adc_set_cloud_voxel_grid): every later cloud is the voxel cloud
    VoxGrid vox_grid;     // the caller's parameters and inv = 1.0f / leaf
    void* vox_table;      // device scratch, allocated by the first set call: the hash table (adc_voxel_table_bytes, 64-byte slots) ...
    uint32_t* vox_slot;   // ... the slot of every pixel [P] ...
    uint32_t* vox_words;  // ... and the count words: voxels, points_valid, points_kept, then three counts per tile
    // optional rectification of raw images in front of the Match (k_rectify.hip; on = both sides set, off: nothing of it is enqueued)
    AdcRectSide rect[2];  // ADC_SIDE_LEFT, ADC_SIDE_RIGHT
    uint8_t* pin_raw;     // pinned staging of the two raw images (left at 0, right behind it)
    size_t pin_raw_cap;
    // optional evaluation against ground truth (k_eval.hip; nothing of it exists before the first adc_set_ground_truth)
    int ev_set;               // ground truth is set (adc_clear_ground_truth / a failed set call: 0)
    int ev_has_right, ev_has_mask; // where the occlusion byte map came from (neither: occlusion is not defined, the map is all 0)
    float ev_occ_thres;
    int ev_cus;               // CUs of the device: the measure kernel's grid is a fixed multiple of it
    float* ev_g[2];           // decoded ground truth of the left / right view, unknown = +inf
    uint8_t* ev_occ;          // 1 = known and non-occluded
    uint8_t* ev_raw;          // device copy of the caller's raw array being decoded (one at a time), then of the mask
    size_t ev_raw_cap;
    uint64_t* ev_rep;         // the report words the measure kernel adds to (adc_eval_report without its echo)
    uint64_t* ev_pin;         // pinned: read-back of the report words, enqueued behind the kernel
    adc_eval_report ev_echo;  // the echo fields of the evaluation enqueued last
    adc_eval_report ev_report; // adc_get_eval_report
    int ev_report_valid;
    float* evs_disp;          // device scratch of adc_evaluate (host callers), each allocated on the first call that needs it
    uint8_t* evs_prov;
    float* evs_conf;
    float* evs_err;
    uint8_t* evs_cls;
    // optional registration of depth into a second camera (k_register.hip; nothing of it exists before the first adc_set_register_target)
    int reg_set;              // a target is set (adc_clear_register_target / a failed set call: 0)
    adc_reg_target reg_target;
    int reg_cus;              // CUs of the device: the counting kernels' grids are a fixed multiple of it
    uint64_t* reg_zbuf;       // one 64-bit key per target pixel, all ones = empty
    size_t reg_zbuf_cap;      // target pixels reg_zbuf holds
    uint32_t* reg_rep;        // the report words the kernels add to (adc_reg_report)
    uint32_t* reg_pin;        // pinned: read-back of the report words, enqueued behind the kernels
    adc_reg_report reg_report; // adc_get_register_report
    int reg_report_valid;
    float* regs_map;          // device scratch of adc_register_depth / adc_align_color (host callers), each allocated on the first call
    uint8_t* regs_out;        // that needs it; the three target-sized ones grow with the largest target used
    uint8_t* regs_valid;
    float* regs_depth;
    size_t regs_depth_cap;    // target pixels each holds
    int32_t* regs_index;
    size_t regs_index_cap;
    uint8_t* regs_tbgr;
    size_t regs_tbgr_cap;
    // optional surface normals from a disparity map (k_normals.hip; nothing of it exists before the first adc_normals_device)
    uint32_t* nrm_rep;        // the four report words the kernel adds to (adc_normals_report); read back into pin_flags[ADC_PIN_NORMALS..]
    adc_normals_report nrm_report; // adc_get_normals_report
    int nrm_report_valid;
    float* nrms_map;          // device scratch of adc_normals (host callers), each allocated on the first call that needs it
    float* nrms_out;
    uint8_t* nrms_out8;
    // optional triangle mesh from a disparity map (k_mesh.hip; nothing of it exists before the first adc_mesh_device)
    uint32_t* msh_words;      // one block sized for step 1 (adc_mesh_scratch_bytes): report words, per-chunk bases, used words, cell codes
    adc_mesh_report msh_report; // adc_get_mesh_report
    int msh_report_valid;
    float* mshs_map;          // device scratch of adc_mesh (host callers), each allocated on the first call that needs it
    uint8_t* mshs_img;
    adc_point* mshs_vtx;          // (these three grow with the largest capacity asked for)
    size_t mshs_vtx_cap;
    int32_t* mshs_vidx;
    size_t mshs_vidx_cap;
    uint32_t* mshs_tri;
    size_t mshs_tri_cap;
    // optional TSDF volume (k_tsdf.hip; nothing of it exists before the first adc_tsdf_create)
    int tsdf_set;             // a volume exists (adc_tsdf_destroy / a failed adc_tsdf_create: 0)
    adc_tsdf_params tsdf_params;
    uint32_t* tsdf_vol;       // one word per voxel: (uint16)(int16)t | w << 16
    uint32_t* tsdf_col;       // with ADC_TSDF_COLOR: r | g << 8 | b << 16 | cw << 24 per voxel
    uint32_t* tsdf_rep;       // ADC_TSDF_REP_WORDS report words the kernels add to: integrate at 0, extract at ADC_TSDF_REP_EXTRACT
    uint32_t* tsdf_tiles;     // per-tile counts / bases of the extraction, allocated on its first use; grows with the largest volume
    size_t tsdf_tiles_cap;
    adc_tsdf_report tsdf_report;          // adc_get_tsdf_report
    int tsdf_report_valid;
    adc_tsdf_extract_report tsdf_xreport;
    int tsdf_xreport_valid;
    float* tsdfs_map;         // device scratch of adc_tsdf_integrate / adc_tsdf_extract (host callers), each allocated on the first call that needs it
    uint8_t* tsdfs_img;
    adc_point* tsdfs_pts;     // (grows with the largest capacity asked for)
    size_t tsdfs_pts_cap;
    // triangle mesh of the volume (adc_tsdf_mesh*; nothing of it exists before the first such call).  tsdf_tiles then holds two arrays
    // of tiles (crossings, triangles); the extraction uses the first
    uint32_t* tsdf_first;     // per voxel: the rank of its first crossing, written by the vertex pass of a call that writes triangles; grows with the largest volume
    size_t tsdf_first_cap;
    adc_tsdf_mesh_report tsdf_mreport;    // adc_get_tsdf_mesh_report
    int tsdf_mreport_valid;
    uint32_t* tsdfs_tri;      // device scratch of adc_tsdf_mesh (host callers): three words per triangle; grows with the largest capacity asked for
    size_t tsdfs_tri_cap;
    // ray cast of the volume (adc_tsdf_raycast*; nothing of it exists before the first adc_tsdf_raycast of a host caller)
    adc_tsdf_raycast_report tsdf_rreport; // adc_get_tsdf_raycast_report
    int tsdf_rreport_valid;
    uint8_t* tsdfs_ray;       // device scratch of adc_tsdf_raycast (host callers): 24 bytes per pixel (depth, normals, bgr, status planes); grows with the largest view
    size_t tsdfs_ray_cap;     // (pixels)
    // stereo-aware fusion (adc_tsdf_weights*, adc_tsdf_fuse*; nothing of it exists before the first such call; the fuse adds its counts
    // to tsdf_rep[ADC_TSDF_REP_FUSE..])
    uint32_t* tsdfw_rep;      // the four report words k_tsdf_obs_weight adds to (no volume needed), allocated by the first weights call
    adc_tsdf_fuse_report tsdf_freport;    // adc_get_tsdf_fuse_report
    int tsdf_freport_valid;
    adc_tsdf_weight_report tsdf_wreport;
    int tsdf_wreport_valid;
    uint8_t* tsdfs_wgt;       // device scratch of adc_tsdf_weights / adc_tsdf_fuse (host callers): the weight map, its provenance and
    uint8_t* tsdfs_prov;      // confidence inputs, each allocated on the first call that needs it (the map and the image use tsdfs_map, tsdfs_img)
    float* tsdfs_conf;
    // moving volume (adc_tsdf_shift*; k_tsdf_shift.hip).  origin0 and offset are set by adc_tsdf_create; no memory exists before the
    // first shift call (the report words) and the first non-zero shift (the second planes, which swap roles with tsdf_vol / tsdf_col)
    float tsdf_origin0[3];    // the origin given to adc_tsdf_create: tsdf_params.origin = origin0 + (float)offset * voxel
    int32_t tsdf_offset[3];   // the sum of all shifts, |.| <= 2^24
    uint32_t* tsdf_vol2;      // the planes the next shift writes
    uint32_t* tsdf_col2;
    uint32_t* tsdf_shift_rep; // 8 words in the layout of adc_tsdf_shift_report: the kernels add to [0..2], the scan writes [3]
    adc_tsdf_shift_report tsdf_sreport;   // adc_get_tsdf_shift_report
    int tsdf_sreport_valid;
    // frame-to-model tracking (adc_track_device / adc_tsdf_track; nothing of it exists before the first call)
    struct AdcTrackState* track_state; // device: the sums, the counts, the `done` word and the record the kernels work on (k_tsdf_track.hip)
    adc_track_result* track_pin;       // pinned: the record of the last enqueued track; no Match writes here
    adc_track_result track_result;     // adc_get_track_result
    int track_result_valid;
    int track_cus;            // CUs of the device: the reduce pass's grid is capped at a fixed multiple of it
    float* tracks_map;        // device scratch of adc_tsdf_track (host callers), allocated by its first call: the model's normals, the map, the model's depth (24 bytes per pixel of the handle)
    // profiling
    int profiling, verbose;
    hipEvent_t ev[ADC_STAGE_COUNT + 1];
    hipEvent_t ev_agg[9];
    float stage_ms[ADC_STAGE_COUNT];
    float agg_pass_ms;
    int agg_launches;
    int agg_passes;    // algorithmic passes those launches covered (a pair launch covers two)
    const char* agg_kernel; // kernel family of the last regular aggregation launch (static string)
    // opt-in paper modes (k_paper.hip; 0 = the reference's behaviour)
    uint32_t paper;
    uint8_t* arms_r;      // arms built on the RIGHT image (ADC_PAPER_RIGHT_ARMS), with its packed pixels and a scratch armmax
    uint32_t* bgrx_r;
    int* armmax_r;
    float* vol_c;         // third volume: accumulator of the averaged scanline paths (ADC_PAPER_SO_SUM)
    // region voting statistics of the last run
    int64_t vote_rounds, vote_evals;
};

// ------------------------------------------------------------------ kernel launchers (one per stage)
// All launch on h->stream, asynchronous, return hipError_t of the launch.
hipError_t adc_launch_gray_census(adc_handle* h);
hipError_t adc_launch_cost(adc_handle* h, float* vol_out);
hipError_t adc_launch_cost_records(adc_handle* h);
// The pipeline's front end (run_heavy without a paper mode; the debug stages, the paper modes and the redo paths keep the plain kernels):
// one pass over both images = gray + census, packed left image, colour-step maps and cost records ...
hipError_t adc_launch_front(adc_handle* h);
hipError_t adc_launch_rrec_markers(adc_handle* h); // ... whose marker columns of the right records are written once per handle (alloc_all)
// ... and behind it the arm words cleared, arms + maxima, then support counts, region boxes and aggregation records from one kernel
hipError_t adc_launch_arm_words_clear(adc_handle* h);
hipError_t adc_launch_build_arms(adc_handle* h);
hipError_t adc_launch_sup_records(adc_handle* h);
// first aggregation pass of the short-arm plan, element-wise (k_cost_agg_flat): writes the volume the small-ring fused-cost march would;
// cap = the ring depth that march would have had, (small_variant, small_L) = its gate.  hipErrorInvalidValue: the geometry does not fit.
bool adc_cost_agg_flat_fits(const adc_handle* h, int cap);
hipError_t adc_launch_cost_agg_flat(adc_handle* h, float* dst, int cap, int small_variant, int small_L);
int adc_agg_small_L(const adc_handle* h);
double adc_agg_sparse_density(void); // density of pass-changing records up to which a direction's small-ring launches run sparse
double adc_agg_gather_density(void); // ... up to which the sparse launches run in their gather form
double adc_cost_flat_density(void);  // horizontal density up to which the first launch of the short-arm plan runs as k_cost_agg_flat
hipError_t adc_launch_arms(adc_handle* h); // arms, support counts, colour-difference maps (= _left + _rest)
hipError_t adc_launch_arms_left(adc_handle* h); // what needs only the left image: packed pixels, arms, maxima, support counts
hipError_t adc_launch_sup_counts(adc_handle* h); // support counts + region boxes from the arms in HBM (debug surface)
hipError_t adc_launch_arms_rest(adc_handle* h); // what reads both images: colour-step maps (+ paper mode: right-image arms)
hipError_t adc_launch_aggregate_tail(adc_handle* h); // the dividing H pass adc_launch_aggregate left to the scanline stage, as a launch of its own
hipError_t adc_launch_records(adc_handle* h); // arms + counts -> packed aggregation records
// vol_a -> vol_a via vol_b; fuse_cost: the first pass computes the matching cost itself, fuse_agg_so: the last pass may move into the
// first scanline pass (short-arm plan); arms: what the caller knows about this image's arm maxima, redo: adc_wait is redoing the Match
// (no sparse launches).  What it launches is planned by agg_plan.h from these and the handle's learned arm / density state, which it only reads.
hipError_t adc_launch_aggregate(adc_handle* h, int iterations, AggArms arms, bool redo, bool fuse_cost, bool fuse_agg_so);
hipError_t adc_launch_so_classes(adc_handle* h, hipStream_t stream);
size_t adc_so_cls_bytes(int W, int H);
hipError_t adc_launch_scanline(adc_handle* h, int passes, bool fuse_wta); // vol_a -> vol_a via vol_b (passes=4); fuse_wta: the last pass also writes disp_l
int adc_so_segments(const adc_handle* h, int* warm_out);        // verified segments per row of the next scanline run
bool adc_so_can_fuse_agg(const adc_handle* h);                  // the next scanline run can take over the last aggregation pass
size_t adc_so_seam_bytes(int W, int H, int Dp);
hipError_t adc_launch_wta(adc_handle* h);                       // vol_a -> disp_l, disp_r
hipError_t adc_launch_wta_left(adc_handle* h);                  // vol_a -> disp_l only (debug form of the left view)
hipError_t adc_paper_aggregate(adc_handle* h, int iterations);  // k_paper.hip: aggregation limited by both images' arms
hipError_t adc_paper_accumulate(adc_handle* h, float* acc, const float* src, int first, int last);
hipError_t adc_launch_lrcheck(adc_handle* h);
hipError_t adc_launch_confidence(adc_handle* h);                // k_extras.hip: vol_a -> req.conf (heavy stream, behind the WTA)
hipError_t adc_launch_provenance(adc_handle* h);                // label, disp_l -> req.prov, req.conf = 0 where filled (object stream)
size_t adc_outputs_scratch_bytes(int W, int H);                 // k_outputs.hip: bytes of out_words
// with_cloud = false: the cloud of the request is somebody else's (the voxel-grid filter), only depth / disp8 are computed
hipError_t adc_launch_out_measure(adc_handle* h, const float* disp, const uint8_t* img, bool with_cloud); // disp -> depth, min / max words, tile counts
hipError_t adc_launch_out_scan(adc_handle* h);                  // tile counts -> tile bases, count words
hipError_t adc_launch_out_emit(adc_handle* h, const float* disp, const uint8_t* img, bool with_cloud);    // disp, img -> disp8, cloud
size_t adc_voxel_table_bytes(int W, int H);                     // k_voxel.hip: bytes of vox_table (cleared once per cloud)
size_t adc_voxel_words_bytes(int W, int H);                     // ... and of vox_words
hipError_t adc_launch_vox_insert(adc_handle* h, const float* disp, const uint8_t* img); // disp, img -> table, vox_slot, valid / kept per tile
hipError_t adc_launch_vox_count(adc_handle* h);                 // leaders per tile; vox_slot keeps the leaders' slots only
hipError_t adc_launch_vox_scan(adc_handle* h);                  // leader counts -> tile bases; the three report words, the count words
hipError_t adc_launch_vox_emit(adc_handle* h);                  // table, vox_slot -> cloud
hipError_t adc_launch_disp16(adc_handle* h, const float* disp, float scale, uint16_t* out);                  // disp -> 16-bit fixed point (k_disp16)
size_t adc_speckle_scratch_words(int W, int H);                 // k_speckle.hip: int32 words of sp_parent
hipError_t adc_launch_speckle_runs(adc_handle* h, const float* src, float max_diff);    // src -> row runs in parent, size = 0, stat words = 0
hipError_t adc_launch_speckle_merge(adc_handle* h, const float* src, float max_diff);   // unions across rows and 64-pixel pieces
hipError_t adc_launch_speckle_flatten(adc_handle* h, int32_t* labels);                  // parent = root (-> labels, may be NULL), sizes, components
hipError_t adc_launch_speckle_apply(adc_handle* h, const float* src, float* dst, uint8_t* prov, int max_size); // small components -> +inf
hipError_t adc_launch_rect_model_maps(adc_handle* h, int side, const adc_camera_model* m); // k_rectify.hip: model -> rect[side].mx / my
hipError_t adc_launch_rect_pack(adc_handle* h, int side);                                   // mx / my -> records, valid map
hipError_t adc_launch_rect_remap(adc_handle* h, int side, const uint8_t* raw, uint8_t* bgr_out); // raw image -> [H][W][3] BGR
hipError_t adc_launch_rect_convert(adc_handle* h, int side, const uint8_t* raw, uint8_t* bgr_out); // the same without maps (set == 2)
// the layout behind a format word: code without the bits, bytes per sample row element, 16-bit samples
static inline int adc_pix_code(int format) { return format & 0xff; }
static inline bool adc_pix_is16(int format) { const int c = format & 0xff; return c == ADC_PIX_GRAY16 || (c >= ADC_PIX_BAYER_RGGB16 && c <= ADC_PIX_BAYER_BGGR16); }
static inline int adc_pix_shift(int format) { const int b = (format >> 8) & 0xff; return adc_pix_is16(format) ? (b ? b : 16) - 8 : 0; }
size_t adc_eval_report_words(void);                             // k_eval.hip: uint64 words of ev_rep / ev_pin
hipError_t adc_launch_eval_gt(adc_handle* h, int side, int format, int pitch, float scale); // ev_raw -> ev_g[side]
hipError_t adc_launch_eval_occ(adc_handle* h, int mode, float occ_thres);                   // 1: ev_g[0], ev_g[1] -> ev_occ; 2: ev_g[0], mask in ev_raw -> ev_occ
hipError_t adc_launch_eval_measure(adc_handle* h, const float* disp, const uint8_t* prov, const float* conf, const float* thresholds, float* err, uint8_t* cls);
hipError_t adc_launch_reg_scatter(adc_handle* h, const float* map, int kind, const adc_calib* calib, uint32_t flags); // k_register.hip: map -> keys in reg_zbuf, src counts
hipError_t adc_launch_reg_resolve(adc_handle* h, float* depth, int32_t* index);                                       // reg_zbuf -> depth, index, dst_filled
hipError_t adc_launch_reg_align(adc_handle* h, const float* map, int kind, const adc_calib* calib, const uint8_t* tbgr, uint8_t* out, uint8_t* valid);
// k_normals.hip: map -> normals / normals8 (each may be NULL), counts added to nrm_rep; G = the gate in 1/1024 pixel
hipError_t adc_launch_normals(adc_handle* h, const float* disp, const adc_calib* calib, int radius, int32_t G, int min_points, float* normals, uint8_t* normals8);
// k_mesh.hip: the three launches of a mesh (measure: cell codes, used words, per-chunk counts, report counts; scan: bases, totals,
// the caller's count words; emit: vertices, vertex_index, triangles -- each output may be NULL) on the words of msh_words
struct AdcMeshReq {
    const float* disp;
    const uint8_t* img;        // may be NULL: colours 0
    const adc_calib* calib;    // may be NULL
    float max_diff;
    int step;
    void* vertices;
    int32_t* vertex_index;
    uint32_t* triangles;
    uint32_t vertex_capacity, triangle_capacity;
    uint32_t* counts;          // the caller's device words, may be NULL
};
size_t adc_mesh_scratch_bytes(int W, int H);
hipError_t adc_launch_mesh_measure(adc_handle* h, const AdcMeshReq& r);
hipError_t adc_launch_mesh_scan(adc_handle* h, const AdcMeshReq& r);
hipError_t adc_launch_mesh_emit(adc_handle* h, const AdcMeshReq& r);
// k_tsdf.hip: one frame into the handle's volume (counts added to tsdf_rep[0..3]); the three launches of an extraction on tsdf_tiles
// (measure: crossings per tile, voxels_seen; scan: bases, points -> tsdf_rep and the caller's word; emit: the records)
#define ADC_TSDF_REP_WORDS 32
#define ADC_TSDF_REP_EXTRACT 8
struct AdcTsdfExtReq {
    uint32_t min_weight;
    void* points;              // may be NULL: counts only
    uint32_t capacity;
    uint32_t* count;           // the caller's device word, may be NULL
};
size_t adc_tsdf_tile_count(const adc_tsdf_params* p);
hipError_t adc_launch_tsdf_integrate(adc_handle* h, const float* map, const uint8_t* img, const adc_tsdf_frame* frame);
hipError_t adc_launch_tsdf_measure(adc_handle* h, const AdcTsdfExtReq& r);
hipError_t adc_launch_tsdf_scan(adc_handle* h, const AdcTsdfExtReq& r);
hipError_t adc_launch_tsdf_emit(adc_handle* h, const AdcTsdfExtReq& r);
hipError_t adc_launch_tsdf_scan_on(adc_handle* h, uint32_t* tbase, int ntiles, uint32_t* rep, uint32_t* count); // k_tsdf_scan on any tile array: rep[1] and *count = the total
// k_tsdf_shift.hip: the leaving list of a shift on tsdf_tiles (measure and emit; the scan between them is adc_launch_tsdf_scan_on with
// rep = tsdf_shift_rep + 2), and the old planes into the second pair (counts added to tsdf_shift_rep[0..2])
#define ADC_TSDF_SHIFT_WORDS 4 // the counts of adc_tsdf_shift_report in front of its reserved words
struct AdcTsdfShiftReq {
    int32_t shift[3];
    uint32_t min_weight;
    void* points;              // may be NULL: counts only
    uint32_t capacity;
    uint32_t* count;           // the caller's device word, may be NULL
};
hipError_t adc_launch_tsdf_leave_measure(adc_handle* h, const AdcTsdfShiftReq& r);
hipError_t adc_launch_tsdf_leave_emit(adc_handle* h, const AdcTsdfShiftReq& r);
hipError_t adc_launch_tsdf_shift(adc_handle* h, const AdcTsdfShiftReq& r, bool move);
// the triangle mesh of the volume: one fused measure (crossings and triangles per tile into the two halves of tsdf_tiles; voxels_seen,
// cells_seen, cells_surface added to tsdf_rep[ADC_TSDF_REP_MESH..]), the scan once per list (which: 0 vertices, 1 triangles), the vertex
// pass (records; with_first also tsdf_first), the triangle pass
#define ADC_TSDF_REP_MESH 10
#define ADC_TSDF_MESH_WORDS 5 // the counts of adc_tsdf_mesh_report in front of its reserved words
struct AdcTsdfMeshReq {
    uint32_t min_weight;
    void* vertices;            // may be NULL
    uint32_t vertex_capacity;
    void* triangles;           // may be NULL
    uint32_t triangle_capacity;
    uint32_t* counts;          // the caller's two device words, may be NULL
};
hipError_t adc_launch_tsdf_mesh_measure(adc_handle* h, const AdcTsdfMeshReq& r);
hipError_t adc_launch_tsdf_mesh_scan(adc_handle* h, const AdcTsdfMeshReq& r, int which);
hipError_t adc_launch_tsdf_mesh_vertices(adc_handle* h, const AdcTsdfMeshReq& r, bool with_first);
hipError_t adc_launch_tsdf_mesh_triangles(adc_handle* h, const AdcTsdfMeshReq& r);
// k_tsdf_raycast.hip: one launch, a lane per ray; the report words (the layout of adc_tsdf_raycast_report: rays, five status counts,
// the 64-bit sample count at an 8-byte aligned place) are added to tsdf_rep[ADC_TSDF_REP_RAY..]
#define ADC_TSDF_REP_RAY 16
#define ADC_TSDF_RAY_WORDS 8 // the counts of adc_tsdf_raycast_report in front of its reserved words
struct AdcTsdfRayReq {
    adc_tsdf_raycast_params view;
    float* depth;              // each may be NULL
    float* normals;
    uint8_t* bgr;
    uint8_t* status;
};
hipError_t adc_launch_tsdf_raycast(adc_handle* h, const AdcTsdfRayReq& r);
// k_tsdf_fuse.hip: the observation weights of a map (counts added to tsdfw_rep[0..3]) and one weighted frame into the handle's volume
// (counts added to tsdf_rep[ADC_TSDF_REP_FUSE..])
#define ADC_TSDF_REP_FUSE 24
#define ADC_TSDF_FUSE_WORDS 6   // the counts of adc_tsdf_fuse_report in front of its reserved words
#define ADC_TSDF_WEIGHT_WORDS 4 // the counts of adc_tsdf_weight_report in front of its reserved words
struct AdcTsdfWeightReq {
    adc_tsdf_frame frame;          // kind, calib
    adc_tsdf_weight_params params;
    const float* map;
    const uint8_t* prov;           // may be NULL
    const float* conf;             // may be NULL
    uint8_t* weight;
};
struct AdcTsdfFuseReq {
    adc_tsdf_frame frame;
    adc_tsdf_fuse_params params;
    const float* map;
    const uint8_t* img;            // may be NULL
    const uint8_t* weight;         // may be NULL: 1 everywhere
};
hipError_t adc_launch_tsdf_weights(adc_handle* h, const AdcTsdfWeightReq& r);
hipError_t adc_launch_tsdf_fuse(adc_handle* h, const AdcTsdfFuseReq& r);
// k_tsdf_track.hip: the state the two kernels of a track share (all bytes zero in front of pass 0) and the two launches of pass
// `iter`: the reduce pass adds its pixels' integers to sums / counts under the state's pose (the request's guess in pass 0); the solve
// turns them into the next pose and the iteration record of res, clears them and sets `done` on a terminal status
struct AdcTrackState {
    long long sums[28];
    uint32_t counts[8];
    uint32_t done, pad_;
    adc_track_result res;
};
struct AdcTrackReq {
    adc_tsdf_frame frame;          // kind, calib; R, t: the guess
    adc_tsdf_raycast_params model; // width, height, focal_px, cx, cy, R, t
    adc_track_params params;
    const float* map;
    const float* fnormals;         // may be NULL
    const float* mdepth;
    const float* mnormals;
};
hipError_t adc_launch_track_reduce(adc_handle* h, const AdcTrackReq& r, uint32_t iter);
hipError_t adc_launch_track_solve(adc_handle* h, const AdcTrackReq& r, uint32_t iter);
#define ADC_MEDB_MAX_SEG 12                   // column segments per band link of the median, at most (k_refine.hip; sizes the hand-off / sink / seam buffers)
size_t adc_median_hand_rows(int H);             // hand-off rows / store-sink blocks of the banded median (k_refine.hip)       // byte maps of the interpolation's empty-space skipping (k_refine.hip)
int adc_irv_probe_xcd_mode(int device);         // 1 iff workgroup g of a launch runs on XCD g % 8 on this device (probed once)
int adc_irv_grid(size_t pixels);                // workgroups of the voting chain for an image of this size
size_t adc_irv_waves(int grid);                // ints of the chain's statistics block (per-wave counters + per-workgroup segment lengths)
size_t adc_irv_px_words(int W, int H);          // dwords of the per-pixel change bitmap (all planes)
size_t adc_irv_list_entries(int W, int H, int D, int grid);     // capacity of the voting work list (one segment per workgroup)
hipError_t adc_run_region_voting(adc_handle* h); // enqueue only (device-driven chain with a launch budget)
hipError_t adc_voting_finish(adc_handle* h, int* continued); // after a sync: continue the chain if the budget was too small
hipError_t adc_launch_interpolation(adc_handle* h, bool force_f64); // force_f64 (debug surface): the f64 walk also where the table walk would run
hipError_t adc_launch_discontinuity(adc_handle* h);
hipError_t adc_launch_median(adc_handle* h);
hipError_t adc_median_fallback(adc_handle* h); // after a hand-off time-out of the banded filter (adc_wait)
// layout helpers for the debug surface
hipError_t adc_launch_pad_volume(adc_handle* h, const float* src_HWD, float* dst_HWDp);
hipError_t adc_launch_unpad_volume(adc_handle* h, const float* src_HWDp, float* dst_HWD);
