// capi.hip -- the C ABI of include/adcensus_c_api.h: object lifetime, the Match pipeline
// (ADCensusStereo.cpp:69-132 stage order) and the test-only per-stage debug surface.
// Host code only; kernels live in the k_*.hip files.
#include "adc_internal.h"
#include "adc_device_fn.h"
#include "itp_plan.h"
#include "tsdf_voxel.h" // tsdf_params_refusal, tsdf_frame_refusal
#include "tsdf_cell.h"  // tsdf_mesh_refusal
#include "tsdf_ray.h"   // tsdf_raycast_refusal
#include "tsdf_track.h" // track_params_refusal, track_model_refusal, track_size_refusal
#include "tsdf_fuse.h"  // tsdf_weight_params_refusal, tsdf_fuse_params_refusal, the defaults
#include "tsdf_shift.h" // the refusals of a shift, the origin from the total offset, the follow rule

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <new>
#include <mutex>
#include <atomic>

static thread_local std::string g_last_error;

#ifdef ADC_FAULT_INJECTION // (test builds only, adc_internal.h)
static std::atomic<long> g_fi_calls{0};
static std::atomic<long> g_fi_fail_at{[] { const char* e = getenv("ADC_TEST_FAIL_AT"); return e ? atol(e) : 0L; }()};
extern "C" int adc_test_fault_now(void) { const long n = ++g_fi_calls; return n == g_fi_fail_at.load(); }
extern "C" void adc_test_fail_at(long n) { g_fi_calls = 0; g_fi_fail_at = n; } // the n-th call from now on fails (0: none)
extern "C" long adc_test_hip_calls(void) { return g_fi_calls.load(); }
static std::atomic<long> g_fi_live{0};
extern "C" long adc_test_live_buffers(void) { return g_fi_live.load(); } // allocations of HipMem not yet freed, all handles of the process
#define ADC_LIVE(d) (g_fi_live += (d))
extern "C" int adc_test_inflight(adc_handle* h) // 0 = idle; bit 0: some byte of h->fly is nonzero, bit 1: the image pointers are borrowed
{
    int r = (h->img_l != h->img_l_own || h->img_r != h->img_r_own) ? 2 : 0;
    for (size_t i = 0; i < sizeof(h->fly); i++) r |= reinterpret_cast<const unsigned char*>(&h->fly)[i] ? 1 : 0;
    return r;
}
#else
#define ADC_LIVE(d) ((void)0)
#endif

// Host ranges the CALLER has page-locked for the library (adc_host_register): images / maps inside such a range are
// transferred by DMA straight from / to the caller's memory, without the pinned staging copies.  Opt-in on purpose: a
// registration must not outlive the allocation (a freed and re-used address range would DMA into stale pages), which only
// the caller can guarantee.
struct HostRange { const char* base; size_t bytes; };
static std::mutex g_host_mu;
static std::vector<HostRange> g_host_ranges;
static bool host_registered(const void* p, size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_host_mu);
    const char* c = static_cast<const char*>(p);
    for (const HostRange& r : g_host_ranges)
        if (c >= r.base && c + bytes <= r.base + r.bytes) return true;
    return false;
}

static void set_error(const char* what, hipError_t e)
{
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
}
static hipError_t hip_checked(const char* what, hipError_t e) { if (e != hipSuccess) set_error(what, e); return e; }
// HIP_TRY: return the error of a call that has made its own hooked HIP calls and left its own message (not counted again);
// HIP_OK: one hooked HIP call, its text is the message
#define HIP_TRY(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return e__; } while (0)
#define HIP_OK(call) HIP_TRY(hip_checked(#call, ADC_HIP(call)))

// A handle's device and pinned memory: dev_mem.h owns it, these are the four HIP calls it makes.  One hooked call per allocation;
// frees are not hooked.  No other function of this file allocates or frees handle state.
struct HipMem {
    static int alloc_device(void** p, size_t bytes) { const hipError_t e = ADC_HIP(hipMalloc(p, bytes)); if (e == hipSuccess) ADC_LIVE(1); return e; }
    static int alloc_pinned(void** p, size_t bytes) { const hipError_t e = ADC_HIP(hipHostMalloc(p, bytes, hipHostMallocDefault)); if (e == hipSuccess) ADC_LIVE(1); return e; }
    static void free_device(void* p) { hipFree(p); ADC_LIVE(-1); }
    static void free_pinned(void* p) { hipHostFree(p); ADC_LIVE(-1); }
};
static hipError_t mem_result(int rc, const char* field)
{
    if (rc != DEV_MEM_FULL) return hip_checked(field, (hipError_t)rc);
    g_last_error = std::string(field) + ": the handle's buffer registry is full (DEV_MEM_SLOTS)";
    return hipErrorOutOfMemory;
}
// (`h` is the handle in scope; on failure the field is null, a grown field's capacity 0, and adc_last_error names the field)
#define MEM_ONCE(field, bytes) mem_result(dev_mem_once<HipMem>(&h->mem, &(field), (bytes)), #field)
#define MEM_ONCE_PINNED(field, bytes) mem_result(dev_mem_once_pinned<HipMem>(&h->mem, &(field), (bytes)), #field)
#define MEM_GROW(field, cap, need, elem) mem_result(dev_mem_grow<HipMem>(&h->mem, &(field), &(cap), (need), (elem)), #field)
#define MEM_GROW_PINNED(field, cap, need, elem) mem_result(dev_mem_grow_pinned<HipMem>(&h->mem, &(field), &(cap), (need), (elem)), #field)
static int scratch_failed(const char* who) { g_last_error = std::string(who) + ": scratch: " + g_last_error; (void)hipGetLastError(); return 2; } // (first use)

// The guide's yardstick (MI355X_MICROARCH.md: "float4 copy"): a grid-stride copy kernel, 16 bytes per lane, four loads in
// flight per lane; best time over a few grid sizes and plain / non-temporal accesses (tools/ubench/copy_ceiling.hip sweeps more
// shapes on the same box: profiles/r4_ubench_copy_ceiling.txt).  bench.py reports the better of this and hipMemcpyAsync.
typedef float adc_vf4 __attribute__((ext_vector_type(4)));
template <bool NT>
__global__ __launch_bounds__(256) void k_copy_yardstick(const adc_vf4* __restrict__ src, adc_vf4* __restrict__ dst, size_t n)
{
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        adc_vf4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = NT ? __builtin_nontemporal_load(&src[i + u * stride]) : src[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (NT) __builtin_nontemporal_store(v[u], &dst[i + u * stride]);
            else dst[i + u * stride] = v[u];
        }
    }
    for (; i < n; i += stride) dst[i] = src[i];
}
extern "C" {

void adc_option_default(adc_option* o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->min_disparity = 0;  o->max_disparity = 64; // adcensus_types.h:67-74
    o->lambda_ad = 10;     o->lambda_census = 30;
    o->cross_L1 = 34;      o->cross_L2 = 17;
    o->cross_t1 = 20;      o->cross_t2 = 6;
    o->so_p1 = 1.0f;       o->so_p2 = 3.0f;      o->so_tso = 15;
    o->irv_ts = 20;        o->irv_th = 0.4f;
    o->lrcheck_thres = 1.0f;
    o->do_lr_check = 1;    o->do_filling = 1;    o->do_discontinuity_adjustment = 0;
}

int adc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
// (a library whose asm-prefetch / register-ring kernels were NOT re-verified on the generated code -- build() with
// ADC_BUILD_SKIP_CODEGEN_CHECK=1 -- says so: the hand-counted s_waitcnt values are only proven for a checked build)
#ifdef ADC_CODEGEN_UNCHECKED
const char* adc_version(void) { return "adcensus-mi355x 0.2 (gfx950) [generated-code checks SKIPPED]"; }
#else
const char* adc_version(void) { return "adcensus-mi355x 0.2 (gfx950)"; }
#endif
const char* adc_last_error(void) { return g_last_error.c_str(); }

static hipError_t alloc_all(adc_handle* h)
{
    const AdcParams& p = h->p;
    const size_t P = (size_t)p.W * p.H;
    const size_t VB = P * p.Dp * sizeof(float);
    HIP_TRY(MEM_ONCE(h->img_l_own, P * 3));
    HIP_TRY(MEM_ONCE(h->img_r_own, P * 3));
    h->img_l = h->img_l_own;
    h->img_r = h->img_r_own;
    HIP_TRY(MEM_ONCE(h->gray_l, P));
    HIP_TRY(MEM_ONCE(h->bgrx_l, P * 4));
    // sized from the PADDED range: the fused-cost pass also marches over padding chunks / lanes (d >= D), whose
    // right-image column x - d lies up to dmin + Dp - 1 columns to the left of the row
    h->rrec_padl = (p.dmin + p.Dp - 1 > 0 ? p.dmin + p.Dp - 1 : 0) + 1;
    h->rrec_pitch = h->rrec_padl + p.W + (p.dmin < 0 ? -p.dmin : 0) + 1;
    HIP_TRY(MEM_ONCE(h->cost_rrec, (size_t)p.H * h->rrec_pitch * 16));
    HIP_TRY(adc_launch_rrec_markers(h)); // (the out-of-image columns never change: adc_launch_front writes the image's own columns only)
    HIP_TRY(MEM_ONCE(h->cost_lrec, P * 16));
    h->med_hpitch = ((p.W + 2 * p.H + 64 + 15) / 16) * 16;
    HIP_TRY(MEM_ONCE(h->med_hand, adc_median_hand_rows(p.H) * h->med_hpitch * sizeof(float))); // (bands + chains of <= 4 speculative copies per band, per column segment)
    HIP_TRY(MEM_ONCE(h->med_sink, adc_median_hand_rows(p.H) * 64 * 16 + (size_t)((p.H + 63) / 64) * ADC_MEDB_MAX_SEG * 64 * 8 + 64)); // store sinks, then the segments' seam columns
    HIP_TRY(MEM_ONCE(h->gray_r, P));
    HIP_TRY(MEM_ONCE(h->census_l, P * 8));
    HIP_TRY(MEM_ONCE(h->census_r, P * 8));
    HIP_TRY(MEM_ONCE(h->arms, P * 4));
    HIP_TRY(MEM_ONCE(h->sup_h, P * 2));
    HIP_TRY(MEM_ONCE(h->sup_v, P * 2));
    HIP_TRY(MEM_ONCE(h->armmax, ADC_ARMMAX_WORDS * sizeof(int)));
    HIP_TRY(MEM_ONCE(h->rec_h, P * 4));
    HIP_TRY(MEM_ONCE(h->rec_v, P * 4));
    HIP_TRY(MEM_ONCE(h->rec2_h, P * 8));
    HIP_TRY(MEM_ONCE(h->rec2_v, P * 8));
    HIP_TRY(MEM_ONCE(h->agg_sink, 1024 * 64 * sizeof(float)));
    // + slack: the scanline kernels fetch up to VPL (<= 32) bytes starting at a column <= W-1 (+1 on R->L passes)
    HIP_TRY(MEM_ONCE(h->cdiff_lh, P + 64));
    HIP_TRY(MEM_ONCE(h->cdiff_lv, P + 64));
    HIP_TRY(MEM_ONCE(h->cdiff_rh, P + 64));
    HIP_TRY(MEM_ONCE(h->cdiff_rv, P + 64));
    HIP_TRY(MEM_ONCE(h->so_cls, adc_so_cls_bytes(p.W, p.H)));
    if (p.VPL <= 2) HIP_TRY(MEM_ONCE(h->so_seam, adc_so_seam_bytes(p.W, p.H, p.Dp))); // (verified segments of the scanline row passes)
    HIP_TRY(MEM_ONCE(h->vol_a, VB));
    HIP_TRY(MEM_ONCE(h->vol_b, VB));
    HIP_TRY(MEM_ONCE(h->lut_ad, 768 * sizeof(float)));
    HIP_TRY(MEM_ONCE(h->lut_census, 64 * sizeof(float)));
    HIP_TRY(MEM_ONCE(h->ray_sincos, 32 * sizeof(double)));
    // (+ 1 KiB: the banded median prefetches a few columns past the last row's end without clamping, k_refine.hip)
    HIP_TRY(MEM_ONCE(h->disp_l, P * 4 + 1024));
    HIP_TRY(MEM_ONCE(h->disp_r, P * 4));
    HIP_TRY(MEM_ONCE(h->disp_tmp, P * 4 + 1024));
    HIP_OK(hipMemset(h->disp_l + P, 0, 1024));
    HIP_OK(hipMemset(h->disp_tmp + P, 0, 1024));
    HIP_TRY(MEM_ONCE(h->label, P));
    HIP_TRY(MEM_ONCE(h->elig, P + 64)); // (LR check: invalid mask, 1 byte per pixel; then the voting chain's bitmap of listed pixels, whole 64-bit words)
    HIP_TRY(MEM_ONCE(h->irv_bbox, P * 4));
    h->irv_grid = adc_irv_grid(P);
    h->irv_xcd_mode = adc_irv_probe_xcd_mode(h->device);
    HIP_TRY(MEM_ONCE(h->vote_list, adc_irv_list_entries(p.W, p.H, p.D, h->irv_grid) * 16)); // int4 per entry, one segment per workgroup (irv_plan.h)
    HIP_OK(hipMemset(h->vote_list, 0xFF, adc_irv_list_entries(p.W, p.H, p.D, h->irv_grid) * 16)); // every slot = IRV_LIST_END
    HIP_TRY(MEM_ONCE(h->vote_evals_arr, adc_irv_waves(h->irv_grid) * sizeof(int32_t)));
    HIP_OK(hipMemset(h->vote_evals_arr, 0, adc_irv_waves(h->irv_grid) * sizeof(int32_t)));
    HIP_TRY(MEM_ONCE(h->interp_list, 2 * P * 4)); // both target lists of the interpolation, P entries each
    HIP_TRY(MEM_ONCE(h->interp_counters, 64 * sizeof(int32_t)));
    {
        const long long ms = adc_itp_max_search(p.dmin, p.dmax); // multistep_refiner.cpp:236
        const bool tab = adc_itp_table_walk_ok(p.W, p.H, ms);    // (itp_plan.h; without the table walk: the cell maps alone, no code maps)
        h->itp_ms = ms > 0x7fffffff ? 0x7fffffff : (int)ms;
        h->itp_pitch = tab ? adc_itp_code_pitch(p.W, h->itp_ms) : 0;
        HIP_TRY(MEM_ONCE(h->itp_cells, adc_itp_alloc_bytes(p.W, p.H, ms)));
        // (everything outside the image never changes: the per-Match kernel only rewrites the image's own columns and rows)
        HIP_OK(hipMemset(h->itp_cells, ADC_ITP_OUTSIDE, adc_itp_alloc_bytes(p.W, p.H, ms)));
    }
    h->st16_pitch = (p.W + 7) & ~7;
    HIP_TRY(MEM_ONCE(h->st16, ((size_t)h->st16_pitch * p.H + 64) * sizeof(uint16_t))); // (an uncached allocation -- visible across XCDs inside a kernel -- measured equal)
    HIP_OK(hipMemset(h->st16, 0xFF, ((size_t)h->st16_pitch * p.H + 64) * sizeof(uint16_t))); // padding columns: invalid bin
    HIP_TRY(MEM_ONCE(h->disp_vote, P * 4));
    HIP_TRY(MEM_ONCE(h->vote_counters, 512 * sizeof(int32_t)));
    // voting chain budget of the FIRST Match of a handle (later ones adapt: kernels used + 40 % + 2): a natural 1080p image needs
    // ~50-75 kernels (round 5: all passes iterate at once; ~350 before); kernels past the end of the chain are no-ops of ~4 us, an
    // exhausted budget costs a synchronous continuation
    h->learned.irv_budget = LEARN_IRV_FIRST;
    // change-tile map of the voting rounds: one BYTE per 8x8 tile, rows padded to a multiple of 4 (+16: a 16-byte load
    // may start at the last dword of a row)
    h->chg_pitch = (((p.W + 7) / 8 + 3) & ~3) + 16;
    const size_t tiles = (size_t)h->chg_pitch * ((p.H + 7) / 8) + 64;
    HIP_TRY(MEM_ONCE(h->chg_a, 2 * tiles)); // two planes (round parity)
    HIP_TRY(MEM_ONCE(h->irv_cold, 64));
    HIP_TRY(MEM_ONCE(h->irv_px, adc_irv_px_words(p.W, p.H) * sizeof(uint32_t)));
    HIP_OK(hipMemset(h->irv_px, 0, adc_irv_px_words(p.W, p.H) * sizeof(uint32_t)));
    HIP_TRY(MEM_ONCE(h->edge, P));
    HIP_TRY(MEM_ONCE_PINNED(h->pin_in, P * 6));
    HIP_TRY(MEM_ONCE_PINNED(h->pin_out, P * 4));
    // (one block: the 64 flag words, then the mirror of the device's armmax words -- maxima, speculation flags, record densities)
    HIP_TRY(MEM_ONCE_PINNED(h->pin_flags, ADC_PIN_WORDS * sizeof(int32_t)));
    h->pin_nz = h->pin_flags + ADC_PIN_ARM + ADC_NZ_BASE; // record densities (k_make_records)
    memset(h->pin_flags, 0, ADC_PIN_WORDS * sizeof(int32_t)); // the ADC_PIN_* words of adc_internal.h: [0] median error, [ADC_PIN_ARM..] mirror of the armmax words (maxima, failed seams, violation flag, record densities), [8] cloud count (k_outputs.hip), [9..11] speckle stats (k_speckle.hip), [16..23] voting state, [32..63] staging of the voting chain's cold block, behind the armmax mirror the TSDF reports
    HIP_OK(hipMemset(h->label, 0, P));
    HIP_OK(hipMemset(h->chg_a, 0, 2 * tiles));
    HIP_OK(hipMemset(h->vol_a, 0, VB));
    HIP_OK(hipMemset(h->vol_b, 0, VB));
    return hipSuccess;
}

// Host-built tables: evaluated with the host's libm so the GPU result is
// bit-identical to what the CPU reference computes with the same libm.
static hipError_t upload_tables(adc_handle* h)
{
    const adc_option& o = h->p.opt;
    float A[768], C[64];
    memset(A, 0, sizeof(A));
    for (int k = 0; k <= 765; k++) {
        const float cost_ad = (float)k / 3.0f;                     // cost_computor.cpp:110
        const float ea = expf(-cost_ad / (float)o.lambda_ad);      // :117
        A[k] = (1.0f - ea) + 1.0f;
    }
    for (int hm = 0; hm < 64; hm++) C[hm] = expf(-(float)hm / (float)o.lambda_census);
    HIP_OK(hipMemcpy(h->lut_ad, A, sizeof(A), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(h->lut_census, C, sizeof(C), hipMemcpyHostToDevice));
    // 16 ray angles: ang = 0.0 (double); ang += pi/16 with float pi, float divide (multistep_refiner.cpp:234,254-268)
    double sc[32];
    const float pi = 3.1415926f;
    double ang = 0.0;
    for (int s = 0; s < 16; s++) {
        sc[2 * s] = sin(ang);
        sc[2 * s + 1] = cos(ang);
        ang += pi / 16;
    }
    HIP_OK(hipMemcpy(h->ray_sincos, sc, sizeof(sc), hipMemcpyHostToDevice));
    {   // integer ray offsets: lround(y + m*sin) == y + lround(m*sin) for every integer 0 <= y < 2^20 as long as m*sin is
        // not within 1e-9 of a .5 tie (the addition's rounding error is < 2^-32); one unsafe entry disables the table
        const long long ms_ll = adc_itp_max_search(o.min_disparity, o.max_disparity); // multistep_refiner.cpp:236
        h->ray_tab = nullptr;
        h->ray_lin = nullptr;
        h->ray_tab_rows = 0;
        if (adc_itp_table_walk_ok(h->p.W, h->p.H, ms_ll)) { // (itp_plan.h: no table where the table walk can never run)
            const int ms = (int)ms_ll;
            // packed offsets [ms][16], then the linear offsets into the padded code map [ms + ADC_ITP_LPAD][16] (adc_device_fn.h)
            std::vector<int32_t> tab((size_t)ms * 16 + (size_t)(ms + ADC_ITP_LPAD) * 16, 0);
            int32_t* lin = tab.data() + (size_t)ms * 16;
            bool safe = true;
            for (int m = 1; m < ms && safe; m++)
                for (int s = 0; s < 16; s++) {
                    const double fy = (double)m * sc[2 * s], fx = (double)m * sc[2 * s + 1];
                    const double ry = fabs(fabs(fy - floor(fy)) - 0.5), rx = fabs(fabs(fx - floor(fx)) - 0.5);
                    if (ry < 1e-9 || rx < 1e-9) { safe = false; break; }
                    const long dy = lround(fy), dx = lround(fx);
                    tab[(size_t)m * 16 + s] = (int32_t)(((uint32_t)(dy & 0xffff) << 16) | (uint32_t)(dx & 0xffff));
                    lin[(size_t)m * 16 + s] = (int32_t)(dy * h->itp_pitch + dx);
                    if (dy < 0 || dy >= ms || dx <= -ms || dx >= ms) safe = false; // (the padding of the code map assumes it; always true)
                }
            if (safe) {
                HIP_TRY(MEM_ONCE(h->ray_tab, tab.size() * sizeof(int32_t)));
                HIP_OK(hipMemcpy(h->ray_tab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
                h->ray_tab_rows = ms;
                h->ray_lin = h->ray_tab + (size_t)ms * 16;
            }
        }
    }
    // penalty classes (scanline_optimizer.cpp:129-141): f32 divides on the host
    h->so_P1[0] = o.so_p1;      h->so_P2[0] = o.so_p2;
    h->so_P1[1] = o.so_p1 / 4;  h->so_P2[1] = o.so_p2 / 4;
    h->so_P1[2] = o.so_p1 / 10; h->so_P2[2] = o.so_p2 / 10;
    return hipSuccess;
}

// One "bandwidth lane" stream per device, shared by every object on it (never destroyed).  ADC_SHARED_HEAVY=0
// makes every object use its own stream for everything.
static hipStream_t shared_heavy_stream(int dev, hipStream_t own)
{
    static const bool shared = [] { const char* e = getenv("ADC_SHARED_HEAVY"); return e ? atoi(e) != 0 : false; }();
    if (!shared) return own;
    static std::mutex mu;
    static hipStream_t lanes[64] = {nullptr};
    std::lock_guard<std::mutex> lk(mu);
    if (dev < 0 || dev >= 64) return own;
    if (!lanes[dev] && hipStreamCreateWithFlags(&lanes[dev], hipStreamNonBlocking) != hipSuccess) return nullptr;
    return lanes[dev];
}

adc_handle* adc_create(int32_t width, int32_t height, const adc_option* opt, int device)
{
    g_last_error.clear();
    if (!opt) { g_last_error = "adc_create: null option"; return nullptr; }
    if (width <= 0 || height <= 0) { g_last_error = "adc_create: width/height <= 0"; return nullptr; }            // ADCensusStereo.cpp:31-33
    const long long range = (long long)opt->max_disparity - (long long)opt->min_disparity;
    if (range <= 0) { g_last_error = "adc_create: disparity range <= 0"; return nullptr; }                         // :38-40
    if (range > ADC_MAX_DISP_RANGE) { g_last_error = "adc_create: disparity range > ADC_MAX_DISP_RANGE"; return nullptr; }
    if ((long long)width * height > (1LL << 30)) { g_last_error = "adc_create: image too large"; return nullptr; }
    if (device >= 0 && hipSetDevice(device) != hipSuccess) { g_last_error = "adc_create: hipSetDevice failed"; return nullptr; }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { g_last_error = "adc_create: no HIP device (the HIP path is mandatory, there is no CPU fallback)"; return nullptr; }

    adc_handle* h = new (std::nothrow) adc_handle();
    if (!h) return nullptr;
    memset(h, 0, sizeof(*h));
    h->device = dev;
    h->p.W = width; h->p.H = height;
    h->p.dmin = opt->min_disparity; h->p.dmax = opt->max_disparity; h->p.D = (int)range;
    h->p.VPL = range <= 64 ? 1 : (range <= 128 ? 2 : (range <= 256 ? 4 : (range <= 512 ? 8 : (range <= 1024 ? 16 : 32))));
    h->p.Dp = 64 * h->p.VPL;
    h->p.opt = *opt;
    bool ok = ADC_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) == hipSuccess;
    h->own_stream = ok;
    if (ok) ok = (h->heavy = shared_heavy_stream(dev, h->stream)) != nullptr;
    if (ok) ok = ADC_HIP(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming)) == hipSuccess;
    if (ok) ok = ADC_HIP(hipEventCreateWithFlags(&h->ev_heavy_done, hipEventDisableTiming)) == hipSuccess;
    for (int i = 0; ok && i <= ADC_STAGE_COUNT; i++) ok = ADC_HIP(hipEventCreate(&h->ev[i])) == hipSuccess;
    for (int i = 0; ok && i < 9; i++) ok = ADC_HIP(hipEventCreate(&h->ev_agg[i])) == hipSuccess;
    if (ok) ok = alloc_all(h) == hipSuccess;
    if (ok) ok = upload_tables(h) == hipSuccess;
    if (!ok) {
        if (g_last_error.empty()) g_last_error = "adc_create: HIP resource creation failed";
        std::string keep = g_last_error;
        adc_destroy(h);
        g_last_error = keep;
        return nullptr;
    }
    return h;
}

void adc_destroy(adc_handle* h)
{
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->heavy) hipStreamSynchronize(h->heavy);
    dev_mem_release_all<HipMem>(&h->mem);
    for (int i = 0; i <= ADC_STAGE_COUNT; i++) if (h->ev[i]) hipEventDestroy(h->ev[i]);
    for (int i = 0; i < 9; i++) if (h->ev_agg[i]) hipEventDestroy(h->ev_agg[i]);
    if (h->ev_in) hipEventDestroy(h->ev_in);
    if (h->ev_heavy_done) hipEventDestroy(h->ev_heavy_done);
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    delete h;
}

// ------------------------------------------------------------------------------ the pipeline
// the stages behind the region voting (redone by adc_wait when the voting chain had to be continued)
static hipError_t run_refine_tail(adc_handle* h)
{
    const adc_option& o = h->p.opt;
    if (h->fly.req.prov || h->fly.req.conf) HIP_OK(adc_launch_provenance(h)); // (reads the voted map before interpolation fills it)
    if (o.do_filling && o.do_lr_check) HIP_OK(adc_launch_interpolation(h, false));
    if (o.do_discontinuity_adjustment) HIP_OK(adc_launch_discontinuity(h));
    HIP_OK(adc_launch_median(h));
    return hipSuccess;
}
static hipError_t run_refine(adc_handle* h)
{
    // MultiStepRefiner::Refine (multistep_refiner.cpp:60-87); do_filling drives both the voting and the
    // interpolation (ADCensusStereo.cpp:182-183).  Without an LR check both lists are empty.
    const adc_option& o = h->p.opt;
    const size_t P = (size_t)h->p.W * h->p.H;
    if (o.do_lr_check) HIP_OK(adc_launch_lrcheck(h));
    else HIP_OK(hipMemsetAsync(h->label, 0, P, h->stream));
    h->fly.irv_pending = 0;
    if (o.do_filling && o.do_lr_check) HIP_OK(adc_run_region_voting(h));
    h->tail_disp_l = h->disp_l;
    h->tail_disp_tmp = h->disp_tmp;
    return run_refine_tail(h);
}

// The streaming phase (cost .. WTA, ~26 passes over the volume) of different objects on one device is
// made mutually exclusive with a host lock: bandwidth-bound kernels of two pairs only fight for HBM/L2,
// while the latency-bound refinement (one-CU median, voting rounds) of one pair overlaps the streaming
// phase of the next.  Measured on MI355X this is SLOWER than free overlap (56 vs 74 pairs/s with two objects),
// so it is opt-in: ADC_HEAVY_EXCLUSIVE=1.
static std::mutex& heavy_lock(int dev)
{
    static std::mutex locks[64];
    return locks[(dev >= 0 && dev < 64) ? dev : 0];
}
static bool heavy_exclusive()
{
    static const bool v = [] { const char* e = getenv("ADC_HEAVY_EXCLUSIVE"); return e ? atoi(e) != 0 : false; }();
    return v;
}

// redo (of adc_wait) == ADC_REDO_FROM_AGGREGATION: a redo that keeps what the stages in front of the aggregation produced (gray / census, the pixel
// records of the fused cost, arms, support counts, aggregation records: none of them is touched by the later stages) and
// restarts at the first aggregation pass -- possible whenever that pass computes the matching cost itself (no input volume).
static hipError_t run_heavy(adc_handle* h, AdcRedo redo)
{
    const bool from_aggregation = redo == ADC_REDO_FROM_AGGREGATION;
    AggArms arms = AGG_ARMS_FULL; // (a redo from the aggregation: valid for every image)
    const bool prof = h->profiling == 1; // (level 2: only the marks around the aggregation launches, k_aggregate.hip)
#define MARK(i, s) do { if (prof) HIP_OK(hipEventRecord(h->ev[i], s)); } while (0)
    if (h->heavy != h->stream) {
        HIP_OK(hipEventRecord(h->ev_in, h->stream));
        HIP_OK(hipStreamWaitEvent(h->heavy, h->ev_in, 0));
    }
    MARK(0, h->heavy);
    static const bool fuse_cost = [] { const char* e = getenv("ADC_FUSE_COST"); return e ? atoi(e) != 0 : true; }();
    const bool fuse_cost_now = fuse_cost && !(h->paper & ADC_PAPER_RIGHT_ARMS); // (paper mode: plain kernels on a stored cost volume)
    h->fly.match_pending = 1; // (adc_wait looks at this Match's arm maxima / speculation flags exactly once)
    if (from_aggregation) {
        MARK(1, h->heavy);
        MARK(2, h->heavy);
        HIP_OK(hipMemsetAsync(h->armmax + 2, 0, 2 * sizeof(int), h->heavy)); // failed seams, "assumed ring too shallow" flag
    } else {
    // Without a paper mode the images are read ONCE (k_front: gray, census, packed left image, colour steps, cost records) and the
    // support counts and the aggregation records come out of one kernel; the paper modes, a redo and ADC_FUSE_COST=0 run the plain
    // kernels.  Either form is four enqueue steps.
    const bool front = fuse_cost_now && h->paper == 0 && redo == ADC_REDO_NONE;
    if (front) {
        HIP_OK(adc_launch_front(h));             // ComputeCost, ADCensusStereo.cpp:84
        MARK(1, h->heavy);
        HIP_OK(adc_launch_arm_words_clear(h));   // CostAggregation, :92
        HIP_OK(adc_launch_build_arms(h));
        HIP_OK(adc_launch_sup_records(h));
    } else {
    HIP_OK(adc_launch_gray_census(h));           // ComputeCost, ADCensusStereo.cpp:84
    // ADC_FUSE_COST (default on): the cost volume is never written -- the first aggregation pass computes each cost
    // in registers from packed pixel records (k_agg_march<.., COSTIN>); otherwise K2 writes it and pass 1 reads it back
    if (fuse_cost_now) HIP_OK(adc_launch_cost_records(h));
    else HIP_OK(adc_launch_cost(h, h->vol_a));
    MARK(1, h->heavy);
    HIP_OK(adc_launch_arms(h));                  // CostAggregation, :92
    }
    MARK(2, h->heavy);
    {   // The maximum arm lengths decide the ring depth of the aggregation kernels and whether same-direction pass pairs
        // can share a launch (k_aggregate.hip).  The host does NOT wait for them: it assumes the maxima of the previous
        // Match of this handle (exact ring depth for that image), the small-ring kernels verify the assumption on the
        // device (armmax[3] is raised and the pass skipped when an arm is longer) and adc_wait redoes the Match with the
        // full ring -- which is valid for every image and is what the first Match of a handle uses.
        // ADC_AGG_HOST_ARMS=1: read the two maxima back instead (one early host synchronisation, the round-1 behaviour).
        static const bool host_arms = [] { const char* e = getenv("ADC_AGG_HOST_ARMS"); return e ? atoi(e) != 0 : false; }();
        if (host_arms && h->pin_flags) {
            HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_ARM, h->armmax, 2 * sizeof(int), hipMemcpyDeviceToHost, h->heavy));
            HIP_OK(hipStreamSynchronize(h->heavy));
            learn_take_arms(&h->learned, h->pin_flags + ADC_PIN_ARM);
            arms = AGG_ARMS_EXACT;
        } else {
            arms = (AggArms)learn_arm_assumption(h->learned);
        }
    }
    if (!front) HIP_OK(adc_launch_records(h));
    } // (!from_aggregation)
    {   // aggregator_.Aggregate(4), :164; the last pass may move into the scanline stage (the launcher decides: short-arm plan, arms <= 4, segmented row passes)
        const hipError_t e_ = adc_launch_aggregate(h, 4, arms, redo != ADC_REDO_NONE, fuse_cost_now, true);
        HIP_OK(e_); // (hooked behind the launcher, like the scanline stage: an injected failure finds the stage enqueued)
    }
    MARK(3, h->heavy);
    static const bool fuse_wta = [] { const char* e = getenv("ADC_FUSE_WTA"); return e ? atoi(e) != 0 : true; }();
    {   // ScanlineOptimize, :100 (+ left-view ComputeDisparity, :108)
        const hipError_t e_ = adc_launch_scanline(h, 4, fuse_wta);
        HIP_OK(e_);
    }
    MARK(4, h->heavy);
    HIP_OK(adc_launch_wta(h));                   // ComputeDisparity + ComputeDisparityRight, :108-109
    if (h->fly.req.conf) HIP_OK(adc_launch_confidence(h)); // (one more read of the optimised volume)
    MARK(5, h->heavy);
    // maxima + violation flag of this pair, looked at by adc_wait (they seed the next Match's assumption)
    // ... together with its record densities, which seed the next Match's choice between dense and sparse small-ring launches
    // (ONE copy of all armmax words; a redo that restarts at the aggregation makes no records: the words are still this pair's)
    if (h->pin_flags) HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_ARM, h->armmax, ADC_ARMMAX_WORDS * sizeof(int), hipMemcpyDeviceToHost, h->heavy));
    HIP_OK(hipEventRecord(h->ev_heavy_done, h->heavy));
    if (h->heavy != h->stream) HIP_OK(hipStreamWaitEvent(h->stream, h->ev_heavy_done, 0));
#undef MARK
    return hipSuccess;
}

static hipError_t run_pipeline(adc_handle* h, AdcRedo redo = ADC_REDO_NONE)
{
    if (heavy_exclusive()) {
        // the uploads of this pair (already queued on the object's stream) run before the lock is taken
        std::lock_guard<std::mutex> lk(heavy_lock(h->device));
        HIP_OK(run_heavy(h, redo));
        HIP_OK(hipEventSynchronize(h->ev_heavy_done)); // hold the lane until the streaming phase has drained
    } else {
        HIP_OK(run_heavy(h, redo));
    }
    HIP_OK(run_refine(h));                       // MultiStepRefine, :117 (object stream)
    if (h->profiling == 1) HIP_OK(hipEventRecord(h->ev[6], h->stream));
    h->fly.timings_pending = h->profiling != 0;
    return hipSuccess;
}

static void collect_timings(adc_handle* h)
{
    if (!h->fly.timings_pending) return;
    h->fly.timings_pending = false;
    for (int i = 0; i < ADC_STAGE_COUNT; i++) {
        float ms = 0.f;
        if (h->profiling != 1 || hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]) != hipSuccess) ms = -1.f; // (level 2: no stage marks were recorded)
        h->stage_ms[i] = ms;
    }
    float tot = 0.f;
    // average duration of a REGULAR aggregation pass (read V + write V); a fused first pass (write-only) is left out
    const int first = h->agg_first_fused ? 1 : 0;
    if (h->agg_dual_last) h->agg_pass_ms = 0.f; // (two plans were enqueued: the marks bracket launches that may have been skipped)
    else if (h->agg_sparse_last) h->agg_pass_ms = 0.f; // (sparse launches do not move read V + write V: no roofline figure for them)
    else if (h->agg_launches > first && hipEventElapsedTime(&tot, h->ev_agg[first], h->ev_agg[h->agg_launches]) == hipSuccess)
        h->agg_pass_ms = tot / (float)(h->agg_launches - first);
    if (h->verbose) { // the reference's stage lines (ADCensusStereo.cpp:88-129)
        printf("computing cost! timing :	%lf s\n", (h->stage_ms[0]) / 1000.0);
        printf("cost aggregating! timing :	%lf s\n", (h->stage_ms[1] + h->stage_ms[2]) / 1000.0);
        printf("scanline optimizing! timing :	%lf s\n", h->stage_ms[3] / 1000.0);
        printf("computing disparities! timing :	%lf s\n", h->stage_ms[4] / 1000.0);
        printf("multistep refining! timing :	%lf s\n", h->stage_ms[5] / 1000.0);
        printf("output disparities! timing :	%lf s\n", 0.0);
    }
}

// The voxel cloud of h->fly.req.out (k_voxel.hip): the table cleared, four launches with geometry-only grids, then the count word on
// its way to pin_flags[ADC_PIN_CLOUD] as for the plain cloud (adc_wait, the staging and the farm deliver min(count, capacity)
// records without knowing which cloud it is) and the three report words to pin_flags[ADC_PIN_VOXEL..] (adc_get_voxel_report)
static hipError_t enqueue_voxel_cloud(adc_handle* h, const float* disp, const uint8_t* img)
{
    HIP_OK(hipMemsetAsync(h->vox_table, 0, adc_voxel_table_bytes(h->p.W, h->p.H), h->stream));
    HIP_OK(adc_launch_vox_insert(h, disp, img));
    HIP_OK(adc_launch_vox_count(h));
    HIP_OK(adc_launch_vox_scan(h));
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_CLOUD, h->vox_words, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream)); // adc_get_cloud_count
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_VOXEL, h->vox_words, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(adc_launch_vox_emit(h));
    return hipSuccess;
}

// depth / point cloud / 8-bit image of h->fly.req.out from a device-resident map (k_outputs.hip), on the object stream; only what was
// asked for is launched
static hipError_t enqueue_outputs(adc_handle* h, const float* disp, const uint8_t* img)
{
    const AdcOutReq& r = h->fly.req.out;
    const bool voxel = r.cloud && h->vox_set; // the cloud is the voxel cloud: its part of measure / scan / emit is replaced
    if (r.disp8) HIP_OK(hipMemsetAsync(h->out_words, 0, 2 * sizeof(uint32_t), h->stream)); // (the min / max words)
    if (!voxel || r.depth || r.disp8) HIP_OK(adc_launch_out_measure(h, disp, img, !voxel));
    if (r.cloud && !voxel) {
        HIP_OK(adc_launch_out_scan(h));
        HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_CLOUD, h->out_words + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream)); // adc_get_cloud_count
    }
    if ((r.cloud && !voxel) || r.disp8) HIP_OK(adc_launch_out_emit(h, disp, img, !voxel));
    if (voxel) HIP_TRY(enqueue_voxel_cloud(h, disp, img));
    return hipSuccess;
}

// The speckle filter (k_speckle.hip) on a device-resident map: four launches with geometry-only grids, then the three stat words
// on their way to pin_flags[ADC_PIN_SPECKLE..] (adc_get_speckle_stats).  dst == src filters in place; max_size <= 0 only labels.
static hipError_t enqueue_speckle(adc_handle* h, const float* src, float* dst, int32_t max_size, float max_diff, int32_t* labels, uint8_t* prov)
{
    const size_t P = (size_t)h->p.W * h->p.H;
    HIP_OK(adc_launch_speckle_runs(h, src, max_diff));
    HIP_OK(adc_launch_speckle_merge(h, src, max_diff));
    HIP_OK(adc_launch_speckle_flatten(h, labels));
    if (max_size > 0) HIP_OK(adc_launch_speckle_apply(h, src, dst, prov, max_size));
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_SPECKLE, h->sp_parent + 2 * P, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

// the map a Match delivers: the filter's own copy when the speckle filter is on (out of place: the median's fallbacks in
// adc_wait rewrite disp_l from the unfiltered intermediate, and nothing of a redo may ever see a map with the filter's holes)
static const float* delivered_map(const adc_handle* h) { return h->sp_max_size > 0 ? h->sp_map : h->disp_l; }

// the final map -> where the caller wants it (pinned staging for host callers, the caller's device buffer otherwise), and the
// outputs computed from it when the Match asked for any (adc_wait comes through here again behind every redo)
static hipError_t enqueue_output(adc_handle* h)
{
    const size_t P = (size_t)h->p.W * h->p.H;
    hipError_t e = hipSuccess;
    const AdcMatchReq& r = h->fly.req;
    if (h->sp_max_size > 0 && (e = enqueue_speckle(h, h->disp_l, h->sp_map, h->sp_max_size, h->sp_max_diff, nullptr, r.prov)) != hipSuccess) return e;
    const float* map = delivered_map(h);
    if (r.map_host && r.map_host_direct == 1) e = ADC_HIP(hipMemcpyAsync(r.map_host, map, P * 4, hipMemcpyDeviceToHost, h->stream)); // page-locked by the caller
    else if (r.map_host && r.map_host_direct == 2) e = hipSuccess; // (pageable, ADC_HOST_DIRECT: copied by adc_wait after the stream has drained)
    else if (r.map_host) e = ADC_HIP(hipMemcpyAsync(h->pin_out, map, P * 4, hipMemcpyDeviceToHost, h->stream));
    else if (r.map_dev) e = ADC_HIP(hipMemcpyAsync(r.map_dev, map, P * 4, hipMemcpyDeviceToDevice, h->stream));
    if (e == hipSuccess && r.out.active) e = enqueue_outputs(h, map, h->img_l);
    if (e == hipSuccess && r.disp16) e = ADC_HIP(adc_launch_disp16(h, map, r.disp16_scale, r.disp16));
    // a host caller's products: every map behind the kernel that wrote it (the provenance map behind the speckle filter's mark)
    // -> its pinned staging, or straight into a destination the caller has registered (direct == 2: copied by adc_wait, like the map)
    for (int i = 0; e == hipSuccess && r.host_delivery && i < ADC_REQ_MAPS; i++) {
        const AdcHostMap& m = r.host[i];
        if (m.dst && m.direct != 2) e = ADC_HIP(hipMemcpyAsync(m.direct ? m.dst : h->map_buf[i].pin, h->map_buf[i].dev, m.bytes, hipMemcpyDeviceToHost, h->stream));
    }
    return e;
}

// Optional rectification (k_rectify.hip): 0 off (no side set: the entry points take rectified W x H BGR images), 1 on (both sides
// set: they take raw images of the declared geometries), -1 exactly one side set (a Match is refused)
static int rectify_state(const adc_handle* h)
{
    const int n = (h->rect[0].set ? 1 : 0) + (h->rect[1].set ? 1 : 0);
    return n == 2 ? 1 : (n == 0 ? 0 : -1);
}
static bool rectify_refused(const adc_handle* h, const char* who)
{
    if (rectify_state(h) >= 0) return false;
    g_last_error = std::string(who) + ": rectification is set for one side only (set the other side, or adc_clear_rectify)";
    return true;
}
// bytes of one raw image: NV12 carries its chroma plane (height / 2 rows of the same pitch) behind the luma plane
static size_t raw_bytes(const adc_raw_format& f)
{
    const size_t luma = (size_t)f.height * (size_t)f.pitch_bytes;
    return adc_pix_code(f.format) == ADC_PIX_NV12 ? luma / 2 * 3 : luma;
}
// one side's raw image -> a W x H BGR buffer: through the maps, or (adc_set_input_format) the conversion alone
static hipError_t launch_rect_side(adc_handle* h, int side, const uint8_t* raw, uint8_t* out)
{
    return h->rect[side].set == 2 ? adc_launch_rect_convert(h, side, raw, out) : adc_launch_rect_remap(h, side, raw, out);
}
// the 16-bit layouts are read as 16-bit words: an odd device address is refused at the call that receives it
static bool raw_address_refused(const adc_handle* h, int side, const void* d_raw, const char* who)
{
    if (!adc_pix_is16(h->rect[side].fmt.format) || ((uintptr_t)d_raw & 1u) == 0) return false;
    g_last_error = std::string(who) + ": the device address of a 16-bit raw image must be even";
    return true;
}
// both raw images -> the handle's own W x H BGR buffers, on the object stream in front of run_pipeline.  Out of place: a redo of
// adc_wait finds the rectified pair still there (nothing downstream writes the image buffers)
static hipError_t enqueue_rectify(adc_handle* h, const void* raw_l, const void* raw_r)
{
    HIP_OK(launch_rect_side(h, ADC_SIDE_LEFT, static_cast<const uint8_t*>(raw_l), h->img_l_own));
    HIP_OK(launch_rect_side(h, ADC_SIDE_RIGHT, static_cast<const uint8_t*>(raw_r), h->img_r_own));
    h->bgrx_valid = 0;
    return hipSuccess;
}

// A HIP call of a Match failed half-way (the reference's contract: Match returns false and the object stays usable,
// ADCensusStereo.cpp:71-76).  Whatever was already enqueued is drained and everything in flight goes back to idle in ONE reset of
// h->fly -- a later Match cannot find a half-described predecessor (a pending voting chain, a dropped aggregation pass the scanline
// stage never consumed, a request with the caller's buffers): a flag that lives in AdcInFlight cannot be forgotten here.  What the
// handle has LEARNED from earlier pairs (arm maxima, chain budget) stays: it is verified on the device for every pair anyway.
static void match_req_clear(adc_handle* h) { memset(&h->fly.req, 0, sizeof(h->fly.req)); }
static void inflight_reset(adc_handle* h) { memset(&h->fly, 0, sizeof(h->fly)); }
// the handle looks at its own image buffers again; the packed left image is stale when they had been borrowed (or the caller says so)
static void images_own(adc_handle* h, bool repack)
{
    if (repack || h->img_l != h->img_l_own || h->img_r != h->img_r_own) h->bgrx_valid = 0;
    h->img_l = h->img_l_own; h->img_r = h->img_r_own;
}

static void abort_match(adc_handle* h)
{
    if (h->heavy) hipStreamSynchronize(h->heavy);
    if (h->stream) hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
    inflight_reset(h);
    learn_forget_densities(&h->learned);
    if (h->pin_flags) { h->pin_flags[ADC_PIN_MEDIAN] = 0; h->pin_flags[ADC_PIN_ARM + 0] = h->pin_flags[ADC_PIN_ARM + 1] = h->pin_flags[ADC_PIN_ARM + 2] = h->pin_flags[ADC_PIN_ARM + 3] = 0; h->pin_flags[ADC_PIN_SPECKLE] = h->pin_flags[ADC_PIN_SPECKLE + 1] = h->pin_flags[ADC_PIN_SPECKLE + 2] = 0; h->pin_flags[ADC_PIN_VOXEL] = h->pin_flags[ADC_PIN_VOXEL + 1] = h->pin_flags[ADC_PIN_VOXEL + 2] = 0; }
    images_own(h, true);
}
// the failure epilogue of the Match path: the message, everything in flight back to idle; code 2
static int fail_match(adc_handle* h, const char* what, hipError_t e) { set_error(what, e); abort_match(h); return 2; }
// the failure epilogue of a call outside a Match: adc_last_error gains the entry point's name, the streams are drained; code 2
static int fail_call(adc_handle* h, const char* who)
{
    const std::string keep = std::string(who) + ": " + g_last_error;
    abort_match(h);
    g_last_error = keep;
    return 2;
}

int adc_match_device(adc_handle* h, const void* d_left, const void* d_right, void* d_disp)
{
    if (!h || !d_left || !d_right || !d_disp) return 1; // ADCensusStereo.cpp:71-76
    if (rectify_refused(h, "adc_match_device")) return 1;
    if (rectify_state(h) > 0 && (raw_address_refused(h, 0, d_left, "adc_match_device") || raw_address_refused(h, 1, d_right, "adc_match_device"))) return 1;
    hipSetDevice(h->device);
    if (rectify_state(h) > 0) {
        // rectification on: the caller's RAW images are read by the remap only (borrowed until adc_wait all the same), the Match
        // runs on the handle's own buffers
        images_own(h, false);
        if (enqueue_rectify(h, d_left, d_right) != hipSuccess) { abort_match(h); return 2; }
    } else {
    // the caller's device images are BORROWED until adc_wait returns (like the reference borrows the host pointers for the
    // duration of Match, ADCensusStereo.cpp:78-79): no copy
    h->img_l = const_cast<uint8_t*>(static_cast<const uint8_t*>(d_left));
    h->img_r = const_cast<uint8_t*>(static_cast<const uint8_t*>(d_right));
    }
    if (run_pipeline(h) != hipSuccess) { abort_match(h); return 2; }
    h->fly.req.map_dev = d_disp;
    h->fly.req.map_host = nullptr;
    if (enqueue_output(h) != hipSuccess) return fail_match(h, "adc_match_device: output copy", hipGetLastError());
    return 0;
}

static int match_async_impl(adc_handle* h, const uint8_t* left, const uint8_t* right, float* disp, bool sync_call)
{
    if (!h || !left || !right || !disp) return 1;
    if (rectify_refused(h, "adc_match")) return 1;
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H;
    images_own(h, false);
    // rectification on: what is uploaded are the two RAW images (height * pitch_bytes each) into the raw buffers, through the raw
    // staging; the remap then writes the own buffers.  Off: nl == nr == 3 * P into the image buffers, as ever
    const bool rect = rectify_state(h) > 0;
    const size_t nl = rect ? raw_bytes(h->rect[0].fmt) : P * 3, nr = rect ? raw_bytes(h->rect[1].fmt) : P * 3;
    uint8_t *const dst_l = rect ? h->rect[0].raw : h->img_l, *const dst_r = rect ? h->rect[1].raw : h->img_r, *const pin = rect ? h->pin_raw : h->pin_in;
    // Synchronous adc_match only (the caller cannot touch its buffers before the call returns): hand the pageable pointers to
    // the runtime (its own chunked staging / pin-in-place: measured 145 vs 140 pairs/s at 1080p; ADC_HOST_DIRECT=0 switches it
    // off).  The asynchronous entry points promise "the images may be reused as soon as the call returns", so they always
    // stage through the handle's pinned buffers (complete on return) unless the caller registered its memory.
    static const bool direct_env = [] { const char* e = getenv("ADC_HOST_DIRECT"); return e ? atoi(e) != 0 : true; }();
    const bool direct = direct_env && sync_call;
    // Registered (page-locked) INPUT images are DMA-ed in place only by the synchronous adc_match, which returns after the
    // copy: the asynchronous entry points (adc_match_async, adc_farm_submit) promise that the caller may refill its images as
    // soon as the call returns, so they always stage the inputs (a DMA still in flight would read the refilled pixels).  The
    // OUTPUT map of a registered range is written in place by every entry point (it is the caller's until adc_wait anyway).
    const bool reg_in = sync_call && host_registered(left, nl) && host_registered(right, nr);
    // (Round 6, measured and NOT adopted: left image first, the kernels that need only the left image -- arms, support counts,
    // aggregation records -- enqueued, the right image on a second stream behind an event.  Pageable buffers: no gain; buffers the
    // caller registered: 192 -> 180 pairs/s -- the cross-stream dependency costs more than the ~0.1 ms of overlap it buys,
    // profiles/r6_ab_upload_overlap.txt.)
    const uint8_t *lsrc = left, *rsrc = right;
    if (!(reg_in || direct)) { // staging: the second image is copied while the first one is on the bus
        memcpy(pin, left, nl);
        lsrc = pin;
    }
    // (reg_in / direct: DMA from the caller's memory -- page-locked by the caller: asynchronous; pageable: the runtime stages)
    if (ADC_HIP(hipMemcpyAsync(dst_l, lsrc, nl, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail_match(h, "adc_match: upload of the left image", hipGetLastError());
    if (!(reg_in || direct)) {
        memcpy(pin + nl, right, nr);
        rsrc = pin + nl;
    }
    if (ADC_HIP(hipMemcpyAsync(dst_r, rsrc, nr, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail_match(h, "adc_match: upload of the right image", hipGetLastError());
    if (rect && enqueue_rectify(h, dst_l, dst_r) != hipSuccess) { abort_match(h); return 2; }
    if (run_pipeline(h) != hipSuccess) { abort_match(h); return 2; }
    h->fly.req.map_host = disp;
    h->fly.req.map_host_direct = host_registered(disp, P * 4) ? 1 : (direct ? 2 : 0);
    h->fly.req.map_dev = nullptr;
    if (enqueue_output(h) != hipSuccess) return fail_match(h, "adc_match: output copy", hipGetLastError());
    return 0;
}

int adc_match_async(adc_handle* h, const uint8_t* left, const uint8_t* right, float* disp)
{
    return match_async_impl(h, left, right, disp, false);
}

int adc_host_register(void* ptr, size_t bytes)
{
    if (!ptr || !bytes) return 1;
    if (hipHostRegister(ptr, bytes, hipHostRegisterDefault) != hipSuccess) { set_error("adc_host_register", hipGetLastError()); return 2; }
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_ranges.push_back(HostRange{static_cast<const char*>(ptr), bytes});
    return 0;
}
int adc_host_unregister(void* ptr)
{
    if (!ptr) return 1;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        bool found = false;
        for (size_t i = 0; i < g_host_ranges.size(); i++)
            if (g_host_ranges[i].base == static_cast<const char*>(ptr)) { g_host_ranges.erase(g_host_ranges.begin() + (long)i); found = true; break; }
        if (!found) return 1;
    }
    return hipHostUnregister(ptr) == hipSuccess ? 0 : 2;
}

// pixels with a pass-changing horizontal / vertical record: the shard sums of the density words in pin_nz
static void rec_nz_sums(const adc_handle* h, long long nz[2])
{
    for (int c = 0; c < 2; c++) {
        nz[c] = 0;
        for (int s = 0; s < ADC_NZ_SHARDS; s++) nz[c] += h->pin_nz[(c * ADC_NZ_SHARDS + s) * ADC_NZ_STRIDE];
    }
}
// what the device said about the Match just drained (pin_flags: one copy at the end of the heavy stream) and which forms it ran
static AdcMatchReport match_report(const adc_handle* h)
{
    const int32_t* a = h->pin_flags + ADC_PIN_ARM;
    AdcMatchReport r = {};
    r.armmax[0] = a[0]; r.armmax[1] = a[1]; r.seam_fails = a[2]; r.ring_shallow = a[3];
    r.rec_nz_valid = h->pin_nz != nullptr;
    if (r.rec_nz_valid) rec_nz_sums(h, r.rec_nz);
    r.so_nseg_last = h->so_nseg_last; r.med_spec_last = h->med_spec_last; r.med_seg_last = h->med_seg_last;
    r.agg_first_fused = h->agg_first_fused != 0;
    r.paper_right_arms = (h->paper & ADC_PAPER_RIGHT_ARMS) != 0;
    return r;
}

// deliver again: everything enqueue_output sends, then the wait for it
static hipError_t redeliver(adc_handle* h) { const hipError_t e = enqueue_output(h); return e != hipSuccess ? e : ADC_HIP(hipStreamSynchronize(h->stream)); }

// The steps of adc_wait, in its order:
// (1) an assumed aggregation ring was too shallow, or a scanline row segment failed its seam: learn_redo says whether the Match
//     runs again and from where (the aggregation on, or as a whole: the inputs are still there); the flags are read again behind it
static int wait_settle_speculation(adc_handle* h)
{
    if (!h->pin_flags) return 0;
    AdcMatchReport rep = match_report(h);
    for (int attempt = 0; attempt < LEARN_MAX_REDOS; attempt++) {
        const AdcRedo redo = learn_redo(&h->learned, &h->lstats, rep);
        if (redo == ADC_REDO_NONE) break;
        hipError_t e = run_pipeline(h, redo);
        if (e == hipSuccess) e = redeliver(h);
        if (e != hipSuccess) return fail_match(h, "adc_wait: redo (full aggregation ring / whole scanline rows)", e);
        rep = match_report(h);
    }
    if (learn_redo_wanted(rep)) { g_last_error = "adc_wait: redo did not clear the speculation flags"; abort_match(h); return 2; }
    learn_commit(&h->learned, &h->lstats, rep, h->fly.match_pending != 0, h->fly.match_pending ? adc_agg_small_L(h) : 0);
    h->fly.match_pending = 0;
    return 0;
}
// (2) the voting chain ran out of its launch budget before it converged: continue it, redo the stages behind it
static hipError_t wait_continue_voting(adc_handle* h)
{
    if (!h->fly.irv_pending) return hipSuccess;
    // the continuation delivers into the buffer that was disp_l when the chain was enqueued (the stages behind the voting have swapped the roles since)
    float *now_l = h->disp_l, *now_tmp = h->disp_tmp;
    h->disp_l = h->tail_disp_l;
    h->disp_tmp = h->tail_disp_tmp;
    int continued = 0;
    hipError_t e = adc_voting_finish(h, &continued);
    if (!continued) { h->disp_l = now_l; h->disp_tmp = now_tmp; }
    if (e == hipSuccess && continued) e = run_refine_tail(h);
    if (e == hipSuccess && continued) e = redeliver(h);
    return e;
}
// (3) a median band gave up waiting for its upstream band: the map is incomplete -- redo the filter with the
//     single-workgroup kernel (no inter-workgroup dependency) and deliver that result
static hipError_t wait_median_fallback(adc_handle* h)
{
    if (h->pin_flags && (h->pin_flags[ADC_PIN_MEDIAN] != 0 || h->fly.force_median_fallback)) {
        hipError_t e = adc_median_fallback(h); // (looks at pin_flags[ADC_PIN_MEDIAN]: 2 = a speculative seam differed -> chained form first)
        h->pin_flags[ADC_PIN_MEDIAN] = 0;
        if (e == hipSuccess) e = redeliver(h);
        if (e != hipSuccess) return e;
    }
    h->fly.force_median_fallback = 0;
    learn_median_commit(&h->learned, h->med_spec_last, h->med_seg_last);
    return hipSuccess;
}
// (4) a host caller's map and products: staging (or, direct == 2, the device scratch) -> the caller's buffers, then the points that exist
static int wait_deliver(adc_handle* h)
{
    const AdcMatchReq r = h->fly.req;
    const size_t map_bytes = (size_t)h->p.W * h->p.H * 4;
    if (r.map_host && r.map_host_direct == 2 && ADC_HIP(hipMemcpy(r.map_host, delivered_map(h), map_bytes, hipMemcpyDeviceToHost)) != hipSuccess) return fail_match(h, "adc_wait: copy-out", hipGetLastError());
    if (r.map_host && r.map_host_direct == 0) memcpy(r.map_host, h->pin_out, map_bytes);
    if (r.host_delivery) {
        for (int i = 0; i < ADC_REQ_MAPS; i++) {
            const AdcHostMap& m = r.host[i];
            if (m.dst && m.direct == 0) memcpy(m.dst, h->map_buf[i].pin, m.bytes);
            if (m.dst && m.direct == 2 && ADC_HIP(hipMemcpy(m.dst, h->map_buf[i].dev, m.bytes, hipMemcpyDeviceToHost)) != hipSuccess) return fail_match(h, "adc_wait: product copy-out", hipGetLastError());
        }
        if (r.cloud) {
            const uint32_t count = (uint32_t)h->pin_flags[ADC_PIN_CLOUD];
            const size_t n = count < r.capacity ? count : r.capacity;
            if (n && ADC_HIP(hipMemcpy(r.cloud, h->os_cloud, n * sizeof(adc_point), hipMemcpyDeviceToHost)) != hipSuccess) return fail_match(h, "adc_wait: cloud copy-out", hipGetLastError());
            if (r.cloud_count) *r.cloud_count = count;
        }
    }
    match_req_clear(h);
    return 0;
}
#define MSH_PIN_WORDS 5 // the counts of adc_mesh_report in front of its reserved words: pin_flags[ADC_PIN_MESH .. ADC_PIN_MESH + 4]
// (5) an evaluation / a registration / a normals / a mesh call has completed: its report words have arrived in the pinned block (adc_get_eval_report,
//     adc_get_register_report, adc_get_normals_report, adc_get_mesh_report)
static void wait_take_reports(adc_handle* h)
{
    if (h->fly.ev_pending) {
        h->ev_report = h->ev_echo;
        memcpy(&h->ev_report, h->ev_pin, adc_eval_report_words() * sizeof(uint64_t));
        h->ev_report_valid = 1;
        h->fly.ev_pending = 0;
    }
    if (h->fly.reg_pending) {
        memcpy(&h->reg_report, h->reg_pin, sizeof(h->reg_report));
        h->reg_report_valid = 1;
        h->fly.reg_pending = 0;
    }
    if (h->fly.nrm_pending) {
        memcpy(&h->nrm_report, h->pin_flags + ADC_PIN_NORMALS, sizeof(h->nrm_report));
        h->nrm_report_valid = 1;
        h->fly.nrm_pending = 0;
    }
    if (h->fly.msh_pending) {
        memset(&h->msh_report, 0, sizeof(h->msh_report));
        memcpy(&h->msh_report, h->pin_flags + ADC_PIN_MESH, MSH_PIN_WORDS * sizeof(uint32_t));
        h->msh_report_valid = 1;
        h->fly.msh_pending = 0;
    }
    if (h->fly.tsdf_pending) {
        memset(&h->tsdf_report, 0, sizeof(h->tsdf_report));
        memcpy(&h->tsdf_report, h->pin_flags + ADC_PIN_TSDF, 4 * sizeof(uint32_t));
        h->tsdf_report_valid = 1;
        h->fly.tsdf_pending = 0;
    }
    if (h->fly.tsdfx_pending) {
        memset(&h->tsdf_xreport, 0, sizeof(h->tsdf_xreport));
        memcpy(&h->tsdf_xreport, h->pin_flags + ADC_PIN_TSDF_EXTRACT, 2 * sizeof(uint32_t));
        h->tsdf_xreport_valid = 1;
        h->fly.tsdfx_pending = 0;
    }
    if (h->fly.tsdfh_pending) {
        memset(&h->tsdf_sreport, 0, sizeof(h->tsdf_sreport));
        memcpy(&h->tsdf_sreport, h->pin_flags + ADC_PIN_TSDF_SHIFT, ADC_TSDF_SHIFT_WORDS * sizeof(uint32_t));
        h->tsdf_sreport_valid = 1;
        h->fly.tsdfh_pending = 0;
    }
    if (h->fly.tsdfm_pending) {
        memset(&h->tsdf_mreport, 0, sizeof(h->tsdf_mreport));
        memcpy(&h->tsdf_mreport, h->pin_flags + ADC_PIN_TSDF_MESH, ADC_TSDF_MESH_WORDS * sizeof(uint32_t));
        h->tsdf_mreport_valid = 1;
        h->fly.tsdfm_pending = 0;
    }
    if (h->fly.tsdfr_pending) {
        memset(&h->tsdf_rreport, 0, sizeof(h->tsdf_rreport));
        memcpy(&h->tsdf_rreport, h->pin_flags + ADC_PIN_TSDF_RAY, ADC_TSDF_RAY_WORDS * sizeof(uint32_t));
        h->tsdf_rreport_valid = 1;
        h->fly.tsdfr_pending = 0;
    }
    if (h->fly.tsdff_pending) {
        memset(&h->tsdf_freport, 0, sizeof(h->tsdf_freport));
        memcpy(&h->tsdf_freport, h->pin_flags + ADC_PIN_TSDF_FUSE, ADC_TSDF_FUSE_WORDS * sizeof(uint32_t));
        h->tsdf_freport_valid = 1;
        h->fly.tsdff_pending = 0;
    }
    if (h->fly.tsdfw_pending) {
        memset(&h->tsdf_wreport, 0, sizeof(h->tsdf_wreport));
        memcpy(&h->tsdf_wreport, h->pin_flags + ADC_PIN_TSDF_WEIGHT, ADC_TSDF_WEIGHT_WORDS * sizeof(uint32_t));
        h->tsdf_wreport_valid = 1;
        h->fly.tsdfw_pending = 0;
    }
    if (h->fly.track_pending) {
        h->track_result = *h->track_pin;
        h->track_result_valid = 1;
        h->fly.track_pending = 0;
    }
}

int adc_wait(adc_handle* h)
{
    if (!h) return 1;
    hipSetDevice(h->device);
    if (ADC_HIP(hipStreamSynchronize(h->stream)) != hipSuccess) return fail_match(h, "adc_wait", hipGetLastError());
    if (wait_settle_speculation(h) != 0) return 2;
    hipError_t e = wait_continue_voting(h);
    if (e != hipSuccess) return fail_match(h, "adc_wait: region voting continuation", e);
    if ((e = wait_median_fallback(h)) != hipSuccess) return fail_match(h, "adc_wait: median fallback", e);
    if (wait_deliver(h) != 0) return 2;
    wait_take_reports(h);
    images_own(h, false); // adc_match_device BORROWED the caller's images until here (a later debug stage would read memory the caller has reused or freed)
    collect_timings(h);
    return 0;
}

int adc_match(adc_handle* h, const uint8_t* left, const uint8_t* right, float* disp)
{
    const int rc = match_async_impl(h, left, right, disp, true);
    if (rc != 0) return rc;
    return adc_wait(h);
}

// ------------------------------------------------------------------------------ one request for every optional product
// Every Match entry point is a view of one request (adc_products; the _ex and _out forms ask for a part of it): it is validated and
// resolved into h->fly.req, the existing stages and enqueue_output do the rest -- the confidence kernel runs behind the WTA in run_heavy,
// the provenance kernel at the top of run_refine_tail, depth / cloud / 8-bit image / 16-bit map are computed from the delivered map in
// enqueue_output.  Every redo of adc_wait goes through these, so every product always describes the delivered disparity map.
static bool outputs_requested(const adc_outputs* o) { return o && (o->depth || o->cloud || o->disp8); }
static bool products_requested(const adc_products* p) { return p && (p->provenance || p->confidence || outputs_requested(&p->out) || p->disp16); }
static bool match_in_flight(const adc_handle* h)
{
    const AdcMatchReq& r = h->fly.req;
    return h->fly.match_pending || r.map_host || r.map_dev || r.out.active || r.host_delivery || r.disp16;
}

static bool extras_allowed(adc_handle* h, const char* who)
{
    if (!h->paper) return true;
    g_last_error = std::string(who) + ": provenance / confidence maps are not defined with paper modes set";
    return false;
}

// validates the outputs of a request and resolves them into *out (not yet active); 0, or 1 (refused, adc_last_error) / 2 (scratch allocation)
static int outputs_prepare(adc_handle* h, const adc_outputs* o, const char* who, bool device_pointers, AdcOutReq* out)
{
    AdcOutReq r;
    memset(&r, 0, sizeof(r));
    if (o->calib) {
        const adc_calib& c = *o->calib;
        if (!(__builtin_isfinite(c.focal_px) && __builtin_isfinite(c.baseline) && __builtin_isfinite(c.cx) && __builtin_isfinite(c.cy) && __builtin_isfinite(c.doffs))) {
            g_last_error = std::string(who) + ": the calibration has a non-finite field";
            return 1;
        }
        if (!(c.focal_px > 0.0f)) { g_last_error = std::string(who) + ": the calibration's focal_px must be positive"; return 1; }
        r.calibrated = 1;
        r.calib = c;
        r.fb = c.focal_px * c.baseline;
    } else if (o->depth) {
        g_last_error = std::string(who) + ": depth needs a calibration";
        return 1;
    } else if (o->cloud && h->vox_set) {
        g_last_error = std::string(who) + ": a cloud with a voxel grid set needs a calibration";
        return 1;
    }
    if (device_pointers && o->cloud && ((uintptr_t)o->cloud & 15u)) { g_last_error = std::string(who) + ": the cloud address must be 16-byte aligned"; return 1; }
    const size_t P = (size_t)h->p.W * h->p.H;
    r.depth = o->depth;
    r.cloud = o->cloud;
    r.capacity = (uint32_t)(o->cloud_capacity < P ? o->cloud_capacity : P); // (there are at most W * H points)
    r.cloud_count = o->cloud ? o->cloud_count : nullptr;
    r.disp8 = o->disp8;
    if (MEM_ONCE(h->out_words, adc_outputs_scratch_bytes(h->p.W, h->p.H)) != hipSuccess) return scratch_failed(who);
    *out = r;
    return 0;
}

// a host caller's products: the device scratch of every requested map and (where the map is delivered through it) its pinned staging
// block, allocated on first use, and a cloud scratch of the capacity asked for
static hipError_t host_scratch(adc_handle* h, const AdcHostMap* host, bool cloud, uint32_t capacity)
{
    for (int i = 0; i < ADC_REQ_MAPS; i++) {
        AdcMapBuf& b = h->map_buf[i];
        if (!host[i].dst) continue;
        HIP_TRY(MEM_ONCE(b.dev, host[i].bytes));
        if (host[i].direct == 0) HIP_TRY(MEM_ONCE_PINNED(b.pin, host[i].bytes));
    }
    if (cloud) HIP_TRY(MEM_GROW(h->os_cloud, h->os_cloud_cap, capacity > 0 ? capacity : 1, sizeof(adc_point))); // (at least one point)
    return hipSuccess;
}

// Validates a request and resolves it into h->fly.req, whole, for the Match that the caller enqueues next.  device_pointers: the request's
// addresses are the device targets themselves; otherwise they are host destinations, the targets are the handle's scratch and
// enqueue_output / adc_wait deliver.  older: the call comes from adc_match_ex / _out or their device forms, which do not refuse while
// a Match is pending and whose host forms (all synchronous) keep their blocking copies behind adc_wait's synchronisation (direct = 2:
// through the staging they were slower than before, profiles/match_request_timing.md).  0, or 1 (refused, adc_last_error) /
// 2 (allocation); h->fly.req is written on 0 only.
static int match_req_resolve(adc_handle* h, const adc_products* p, const char* who, bool device_pointers, bool older)
{
    if (!older && match_in_flight(h)) { g_last_error = std::string(who) + ": a Match is pending (adc_wait first)"; return 1; }
    if ((p->provenance || p->confidence) && !extras_allowed(h, who)) return 1;
    if (p->disp16 && !(__builtin_isfinite(p->disp16_scale) && p->disp16_scale > 0.0f)) { g_last_error = std::string(who) + ": disp16_scale must be finite and > 0"; return 1; }
    if (p->disp16 && device_pointers && ((uintptr_t)p->disp16 & 1u)) { g_last_error = std::string(who) + ": the device address of disp16 must be even"; return 1; }
    AdcMatchReq r;
    memset(&r, 0, sizeof(r));
    if (outputs_requested(&p->out)) {
        const int rc = outputs_prepare(h, &p->out, who, device_pointers, &r.out);
        if (rc != 0) return rc;
        r.out.active = 1;
    }
    void* target[ADC_REQ_MAPS] = {p->provenance, p->confidence, p->out.depth, p->out.disp8, p->disp16};
    if (!device_pointers) {
        const size_t P = (size_t)h->p.W * h->p.H;
        const size_t bytes[ADC_REQ_MAPS] = {P, P * 4, P * 4, P, P * 2};
        for (int i = 0; i < ADC_REQ_MAPS; i++)
            if (target[i]) r.host[i] = AdcHostMap{target[i], bytes[i], host_registered(target[i], bytes[i]) ? 1 : (older ? 2 : 0)};
        if (host_scratch(h, r.host, p->out.cloud != nullptr, r.out.capacity) != hipSuccess) return scratch_failed(who);
        for (int i = 0; i < ADC_REQ_MAPS; i++)
            if (target[i]) target[i] = h->map_buf[i].dev;
        r.cloud = p->out.cloud;
        r.capacity = r.out.capacity;
        r.cloud_count = p->out.cloud ? p->out.cloud_count : nullptr;
        r.out.cloud = p->out.cloud ? h->os_cloud : nullptr;
        r.out.cloud_count = nullptr; // (the count reaches the host through pin_flags[ADC_PIN_CLOUD])
        r.host_delivery = 1;
    }
    r.prov = static_cast<uint8_t*>(target[ADC_MAP_PROV]);
    r.conf = static_cast<float*>(target[ADC_MAP_CONF]);
    r.out.depth = static_cast<float*>(target[ADC_MAP_DEPTH]);
    r.out.disp8 = static_cast<uint8_t*>(target[ADC_MAP_DISP8]);
    r.disp16 = static_cast<uint16_t*>(target[ADC_MAP_DISP16]);
    r.disp16_scale = p->disp16_scale;
    h->fly.req = r;
    return 0;
}

// The host entry points: nothing requested = exactly adc_match / adc_match_async.  A call that is refused behind the resolver (1)
// leaves the request as it found it -- a Match pending on the handle keeps its own; a HIP failure (2) has been through abort_match.
static int match_host_req(adc_handle* h, const uint8_t* left, const uint8_t* right, float* disp, const adc_products* p, bool sync_call, const char* who, bool older)
{
    if (!products_requested(p)) {
        const int rc = match_async_impl(h, left, right, disp, sync_call);
        return rc == 0 && sync_call ? adc_wait(h) : rc;
    }
    if (!h || !left || !right || !disp) return 1;
    hipSetDevice(h->device);
    const AdcMatchReq before = h->fly.req;
    int rc = match_req_resolve(h, p, who, false, older);
    if (rc != 0) return rc;
    rc = match_async_impl(h, left, right, disp, sync_call);
    if (rc == 1) h->fly.req = before;
    if (rc == 0 && sync_call) rc = adc_wait(h);
    return rc;
}
// the device entry points: nothing requested = exactly adc_match_device
static int match_device_req(adc_handle* h, const void* d_left, const void* d_right, void* d_disp, const adc_products* p, const char* who, bool older)
{
    if (!products_requested(p)) return adc_match_device(h, d_left, d_right, d_disp);
    if (!h || !d_left || !d_right || !d_disp) return 1;
    hipSetDevice(h->device);
    const AdcMatchReq before = h->fly.req;
    int rc = match_req_resolve(h, p, who, true, older);
    if (rc != 0) return rc;
    rc = adc_match_device(h, d_left, d_right, d_disp);
    if (rc == 1) h->fly.req = before;
    return rc;
}

int adc_match_products(adc_handle* h, const uint8_t* left, const uint8_t* right, float* disp, const adc_products* p)
{
    return match_host_req(h, left, right, disp, p, true, "adc_match_products", false);
}
int adc_match_async_products(adc_handle* h, const uint8_t* left, const uint8_t* right, float* disp, const adc_products* p)
{
    return match_host_req(h, left, right, disp, p, false, "adc_match_async_products", false);
}
int adc_match_device_products(adc_handle* h, const void* d_left, const void* d_right, void* d_disp, const adc_products* p)
{
    return match_device_req(h, d_left, d_right, d_disp, p, "adc_match_device_products", false);
}

// the two older generations ask for a part of the request (older = true)
static adc_products products_of(void* prov, void* conf, const adc_outputs* out)
{
    adc_products p;
    memset(&p, 0, sizeof(p));
    p.provenance = static_cast<uint8_t*>(prov);
    p.confidence = static_cast<float*>(conf);
    if (out) p.out = *out;
    return p;
}
int adc_match_ex(adc_handle* h, const uint8_t* left, const uint8_t* right, float* disp, uint8_t* prov, float* conf)
{
    const adc_products p = products_of(prov, conf, nullptr);
    return match_host_req(h, left, right, disp, &p, true, "adc_match_ex", true);
}
int adc_match_device_ex(adc_handle* h, const void* d_left, const void* d_right, void* d_disp, void* d_prov, void* d_conf)
{
    const adc_products p = products_of(d_prov, d_conf, nullptr);
    return match_device_req(h, d_left, d_right, d_disp, &p, "adc_match_device_ex", true);
}
int adc_match_out(adc_handle* h, const uint8_t* left, const uint8_t* right, float* disp, const adc_outputs* out)
{
    const adc_products p = products_of(nullptr, nullptr, out);
    return match_host_req(h, left, right, disp, &p, true, "adc_match_out", true);
}
int adc_match_device_out(adc_handle* h, const void* d_left, const void* d_right, void* d_disp, const adc_outputs* out)
{
    const adc_products p = products_of(nullptr, nullptr, out);
    return match_device_req(h, d_left, d_right, d_disp, &p, "adc_match_device_out", true);
}

int adc_reproject_device(adc_handle* h, const void* d_disp, const void* d_bgr_left, const adc_outputs* out)
{
    if (!h || !d_disp || (out && out->cloud && !d_bgr_left)) return 1;
    if (!outputs_requested(out)) return 0;
    if (h->fly.req.out.active) { g_last_error = "adc_reproject_device: a Match with outputs is pending (adc_wait first)"; return 1; }
    hipSetDevice(h->device);
    const int rc = outputs_prepare(h, out, "adc_reproject_device", true, &h->fly.req.out);
    if (rc != 0) return rc;
    // (out.active stays 0: nothing of a later adc_wait may run these again on the handle's own map)
    if (enqueue_outputs(h, static_cast<const float*>(d_disp), static_cast<const uint8_t*>(d_bgr_left)) != hipSuccess) { abort_match(h); return 2; }
    return 0;
}

int adc_get_cloud_count(adc_handle* h, uint64_t* count)
{
    if (!h || !count || !h->pin_flags) return 1;
    *count = (uint32_t)h->pin_flags[ADC_PIN_CLOUD];
    return 0;
}

int adc_disp16_device(adc_handle* h, const void* d_disp, float scale, void* d_disp16)
{
    if (!h) return 1;
    if (!d_disp || !d_disp16) { g_last_error = "adc_disp16_device: null map"; return 1; }
    if (!(__builtin_isfinite(scale) && scale > 0.0f)) { g_last_error = "adc_disp16_device: scale must be finite and > 0"; return 1; }
    if ((uintptr_t)d_disp16 & 1u) { g_last_error = "adc_disp16_device: the device address of disp16 must be even"; return 1; }
    hipSetDevice(h->device);
    const hipError_t e = ADC_HIP(adc_launch_disp16(h, static_cast<const float*>(d_disp), scale, static_cast<uint16_t*>(d_disp16)));
    if (e != hipSuccess) return fail_match(h, "adc_disp16_device", e);
    return 0;
}

// ------------------------------------------------------------------------------ speckle filter (k_speckle.hip)
// Handle state; enqueue_output runs the filter on disp_l into sp_map in front of the copy-out and the outputs, so every redo
// of adc_wait (each ends in enqueue_output) refilters the recomputed map.
static bool speckle_args_ok(float max_diff, const char* who)
{
    if (__builtin_isfinite(max_diff) && max_diff >= 0.0f) return true;
    g_last_error = std::string(who) + ": max_diff must be finite and >= 0";
    return false;
}

// first use: parent / size / stat words, and (for the Matches) the filtered map
static int speckle_scratch(adc_handle* h, bool with_map, const char* who)
{
    if (MEM_ONCE(h->sp_parent, adc_speckle_scratch_words(h->p.W, h->p.H) * sizeof(int32_t)) != hipSuccess) return scratch_failed(who);
    if (with_map && MEM_ONCE(h->sp_map, (size_t)h->p.W * h->p.H * 4) != hipSuccess) return scratch_failed(who);
    return 0;
}

int adc_set_speckle_filter(adc_handle* h, int32_t max_size, float max_diff)
{
    if (!h) return 1;
    if (!speckle_args_ok(max_diff, "adc_set_speckle_filter")) return 1;
    if (match_in_flight(h)) { g_last_error = "adc_set_speckle_filter: a Match is pending (adc_wait first)"; return 1; }
    if (max_size <= 0) { h->sp_max_size = 0; h->sp_max_diff = 0.0f; return 0; }
    hipSetDevice(h->device);
    const int rc = speckle_scratch(h, true, "adc_set_speckle_filter");
    if (rc != 0) return rc;
    h->sp_max_size = max_size;
    h->sp_max_diff = max_diff;
    return 0;
}

int adc_filter_speckles_device(adc_handle* h, void* d_disp_inout, int32_t max_size, float max_diff, void* d_labels)
{
    if (!h) return 1;
    if (!d_disp_inout) { g_last_error = "adc_filter_speckles_device: null map"; return 1; }
    if (!speckle_args_ok(max_diff, "adc_filter_speckles_device")) return 1;
    if (max_size <= 0 && !d_labels) return 0;
    hipSetDevice(h->device);
    const int rc = speckle_scratch(h, false, "adc_filter_speckles_device");
    if (rc != 0) return rc;
    float* map = static_cast<float*>(d_disp_inout);
    if (enqueue_speckle(h, map, map, max_size, max_diff, static_cast<int32_t*>(d_labels), nullptr) != hipSuccess) { abort_match(h); return 2; }
    return 0;
}

int adc_get_speckle_stats(adc_handle* h, uint32_t* components, uint32_t* removed_components, uint32_t* removed_pixels)
{
    if (!h || !h->pin_flags) return 1;
    if (components) *components = (uint32_t)h->pin_flags[ADC_PIN_SPECKLE];
    if (removed_components) *removed_components = (uint32_t)h->pin_flags[ADC_PIN_SPECKLE + 1];
    if (removed_pixels) *removed_pixels = (uint32_t)h->pin_flags[ADC_PIN_SPECKLE + 2];
    return 0;
}

// ------------------------------------------------------------------------------ voxel-grid filter of the cloud (k_voxel.hip)
// Handle state; enqueue_outputs runs the voxel launches in place of the cloud's part of its own, so every entry point and every redo
// of adc_wait (each ends in enqueue_output) delivers the voxel cloud of the map it delivers.
static bool voxel_grid_ok(const adc_voxel_grid* g, const char* who)
{
    const char* bad = nullptr;
    if (!(__builtin_isfinite(g->leaf) && g->leaf > 0.0f)) bad = "leaf must be finite and > 0";
    else if (!(g->z_min <= g->z_max)) bad = "z_min <= z_max is required (neither may be NaN)";
    else if (g->flags & ~ADC_VOXEL_POSE) bad = "unknown flags";
    else if (g->reserved[0] | g->reserved[1] | g->reserved[2] | g->reserved[3]) bad = "the reserved words must be 0";
    for (int i = 0; !bad && (g->flags & ADC_VOXEL_POSE) && i < 12; i++)
        if (!__builtin_isfinite(i < 9 ? g->R[i] : g->t[i - 9])) bad = "the pose has a non-finite field";
    if (!bad) return true;
    g_last_error = std::string(who) + ": " + bad;
    return false;
}

int adc_set_cloud_voxel_grid(adc_handle* h, const adc_voxel_grid* grid)
{
    if (!h) { g_last_error = "adc_set_cloud_voxel_grid: null handle"; return 1; }
    if (!grid) { g_last_error = "adc_set_cloud_voxel_grid: null grid"; return 1; }
    if (!voxel_grid_ok(grid, "adc_set_cloud_voxel_grid")) return 1;
    if (match_in_flight(h)) { g_last_error = "adc_set_cloud_voxel_grid: a Match is pending (adc_wait first)"; return 1; }
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H;
    if (MEM_ONCE(h->vox_table, adc_voxel_table_bytes(h->p.W, h->p.H)) != hipSuccess || MEM_ONCE(h->vox_slot, P * sizeof(uint32_t)) != hipSuccess ||
        MEM_ONCE(h->vox_words, adc_voxel_words_bytes(h->p.W, h->p.H)) != hipSuccess) {
        h->vox_set = 0;
        return scratch_failed("adc_set_cloud_voxel_grid");
    }
    VoxGrid v;
    memset(&v, 0, sizeof(v));
    v.leaf = grid->leaf;
    v.inv = 1.0f / grid->leaf;
    v.z_min = grid->z_min; v.z_max = grid->z_max;
    v.flags = grid->flags;
    if (grid->flags & ADC_VOXEL_POSE) { memcpy(v.R, grid->R, sizeof(v.R)); memcpy(v.t, grid->t, sizeof(v.t)); }
    h->vox_grid = v;
    h->vox_set = 1;
    return 0;
}

int adc_clear_cloud_voxel_grid(adc_handle* h)
{
    if (!h) { g_last_error = "adc_clear_cloud_voxel_grid: null handle"; return 1; }
    if (match_in_flight(h)) { g_last_error = "adc_clear_cloud_voxel_grid: a Match is pending (adc_wait first)"; return 1; }
    h->vox_set = 0;
    return 0;
}

int adc_get_voxel_report(adc_handle* h, adc_voxel_report* out)
{
    if (!h || !out || !h->pin_flags) { g_last_error = "adc_get_voxel_report: null argument"; return 1; }
    out->voxels = (uint32_t)h->pin_flags[ADC_PIN_VOXEL];
    out->points_valid = (uint32_t)h->pin_flags[ADC_PIN_VOXEL + 1];
    out->points_kept = (uint32_t)h->pin_flags[ADC_PIN_VOXEL + 2];
    return 0;
}

// ------------------------------------------------------------------------------ rectification (k_rectify.hip)
// Handle state per side.  A set call brings the float maps to the device (the caller's, or the model's computed there), packs them
// into the records of the hot kernel and the valid map, and waits: the entry points above find everything ready.
// bytes per pixel of a row (NV12: of a luma row); 0: not a layout (codes 4..15 and everything between the groups stay invalid)
static int rect_bpp(int format)
{
    const int c = adc_pix_code(format);
    if (c == ADC_PIX_BGR8 || c == ADC_PIX_RGB8) return 3;
    if (c == ADC_PIX_BGRA8) return 4;
    if (c == ADC_PIX_GRAY8 || c == ADC_PIX_NV12 || (c >= ADC_PIX_BAYER_RGGB8 && c <= ADC_PIX_BAYER_BGGR8)) return 1;
    if (c == ADC_PIX_GRAY16 || c == ADC_PIX_YUYV || c == ADC_PIX_UYVY || (c >= ADC_PIX_BAYER_RGGB16 && c <= ADC_PIX_BAYER_BGGR16)) return 2;
    return 0;
}
// the format word and the parity rules of its layout; nullptr: fine
static const char* rect_format_why(const adc_raw_format* f)
{
    const int c = adc_pix_code(f->format), bits = (f->format >> 8) & 0xff;
    if (f->format < 0 || f->format > 0xffff || rect_bpp(f->format) == 0) return "unknown pixel format";
    if (bits != 0 && !(adc_pix_is16(f->format) && bits >= 9 && bits <= 16)) return "unknown pixel format (significant bits: 9..16, 16-bit layouts only)";
    if (adc_pix_is16(f->format) && (f->pitch_bytes & 1)) return "pitch_bytes of a 16-bit layout must be even";
    if (c >= ADC_PIX_BAYER_RGGB8 && c <= ADC_PIX_BAYER_BGGR16 && (f->width < 2 || f->height < 2)) return "a Bayer image needs width and height >= 2";
    if ((c == ADC_PIX_YUYV || c == ADC_PIX_UYVY || c == ADC_PIX_NV12) && (f->width & 1)) return "the width of a YUV layout must be even";
    if (c == ADC_PIX_NV12 && (f->height & 1)) return "the height of an NV12 image must be even";
    return nullptr;
}

static int rect_args_ok(adc_handle* h, int side, const adc_raw_format* f, const void* a, const void* b, const char* who)
{
    if (!h || !f || !a || !b) return 0;
    const char* why = nullptr;
    if (side != ADC_SIDE_LEFT && side != ADC_SIDE_RIGHT) why = "side must be ADC_SIDE_LEFT or ADC_SIDE_RIGHT";
    else if (f->format < 0 || f->format > 0xffff || rect_bpp(f->format) == 0) why = "unknown pixel format";
    else if (f->width < 1 || f->width > 32767 || f->height < 1 || f->height > 32767) why = "raw width / height must be 1..32767";
    else if ((long long)f->pitch_bytes < (long long)f->width * rect_bpp(f->format)) why = "pitch_bytes is smaller than a row";
    else if ((why = rect_format_why(f)) != nullptr) {}
    else if ((long long)raw_bytes(*f) > 2147483647LL) why = "a raw image must be smaller than 2 GiB";
    else if (match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    if (why) g_last_error = std::string(who) + ": " + why;
    return why ? 0 : 1;
}

// first set call of a handle: the [H][W] buffers of both sides; every set call: raw buffer and raw staging large enough
static hipError_t rect_buffers(adc_handle* h, int side, const adc_raw_format* f, bool maps)
{
    const size_t P = (size_t)h->p.W * h->p.H;
    for (int s = 0; maps && s < 2; s++) { // (conversion only: no records, no maps, no valid map)
        AdcRectSide& r = h->rect[s];
        HIP_TRY(MEM_ONCE(r.rec, P * 8));
        HIP_TRY(MEM_ONCE(r.mx, P * 4));
        HIP_TRY(MEM_ONCE(r.my, P * 4));
        HIP_TRY(MEM_ONCE(r.valid, P));
    }
    AdcRectSide& r = h->rect[side];
    const size_t n = raw_bytes(*f);
    HIP_TRY(MEM_GROW(r.raw, r.raw_cap, n, 1));
    const size_t other = h->rect[side ^ 1].set ? raw_bytes(h->rect[side ^ 1].fmt) : n; // (sized for two raw images)
    return MEM_GROW_PINNED(h->pin_raw, h->pin_raw_cap, n + other, 1);
}

static hipError_t rect_install(adc_handle* h, int side, const adc_raw_format* f, const float* map_x, const float* map_y, const adc_camera_model* model)
{
    const size_t P = (size_t)h->p.W * h->p.H;
    const hipError_t eb = rect_buffers(h, side, f, true); // (every HIP call in there is hooked itself)
    if (eb != hipSuccess) return eb;
    AdcRectSide& r = h->rect[side];
    r.fmt = *f;
    if (model) HIP_OK(adc_launch_rect_model_maps(h, side, model));
    else {
        HIP_OK(hipMemcpyAsync(r.mx, map_x, P * 4, hipMemcpyHostToDevice, h->stream));
        HIP_OK(hipMemcpyAsync(r.my, map_y, P * 4, hipMemcpyHostToDevice, h->stream));
    }
    HIP_OK(adc_launch_rect_pack(h, side));
    HIP_OK(hipStreamSynchronize(h->stream));
    return hipSuccess;
}

static int rect_set(adc_handle* h, int side, const adc_raw_format* f, const float* map_x, const float* map_y, const adc_camera_model* model, const char* who)
{
    hipSetDevice(h->device);
    h->rect[side].set = 0; // (a failure below leaves this side unset: its records may be half written)
    if (rect_install(h, side, f, map_x, map_y, model) != hipSuccess) return fail_call(h, who);
    h->rect[side].set = 1;
    return 0;
}

int adc_set_rectify_maps(adc_handle* h, int side, const adc_raw_format* raw, const float* map_x, const float* map_y)
{
    if (!rect_args_ok(h, side, raw, map_x, map_y, "adc_set_rectify_maps")) return 1;
    return rect_set(h, side, raw, map_x, map_y, nullptr, "adc_set_rectify_maps");
}

int adc_set_rectify_model(adc_handle* h, int side, const adc_raw_format* raw, const adc_camera_model* model)
{
    if (!rect_args_ok(h, side, raw, model, model, "adc_set_rectify_model")) return 1;
    const float* v = &model->fx;
    bool finite = true;
    for (size_t i = 0; i < sizeof(adc_camera_model) / sizeof(float); i++) finite = finite && __builtin_isfinite(v[i]);
    if (!finite || model->fx == 0.0f || model->fy == 0.0f || model->new_fx == 0.0f || model->new_fy == 0.0f) {
        g_last_error = "adc_set_rectify_model: every value must be finite, and fx, fy, new_fx, new_fy nonzero";
        return 1;
    }
    return rect_set(h, side, raw, nullptr, nullptr, model, "adc_set_rectify_model");
}

int adc_set_input_format(adc_handle* h, int side, const adc_raw_format* raw)
{
    if (!rect_args_ok(h, side, raw, raw, raw, "adc_set_input_format")) return 1;
    if (raw->width != h->p.W || raw->height != h->p.H) {
        g_last_error = "adc_set_input_format: width / height must be the handle's (frames of another geometry need adc_set_rectify_*)";
        return 1;
    }
    hipSetDevice(h->device);
    h->rect[side].set = 0;
    if (rect_buffers(h, side, raw, false) != hipSuccess) return fail_call(h, "adc_set_input_format"); // raw buffer and raw staging of the host entry points
    h->rect[side].fmt = *raw;
    h->rect[side].set = 2;
    return 0;
}

int adc_clear_rectify(adc_handle* h)
{
    if (!h) return 1;
    if (match_in_flight(h)) { g_last_error = "adc_clear_rectify: a Match is pending (adc_wait first)"; return 1; }
    h->rect[0].set = 0;
    h->rect[1].set = 0;
    return 0;
}

int adc_get_rectify_maps(adc_handle* h, int side, float* map_x, float* map_y, uint8_t* valid)
{
    if (!h || (side != ADC_SIDE_LEFT && side != ADC_SIDE_RIGHT)) return 1;
    const AdcRectSide& r = h->rect[side];
    if (!r.set) { g_last_error = "adc_get_rectify_maps: this side is not set"; return 1; }
    if (r.set == 2) { g_last_error = "adc_get_rectify_maps: this side converts only (adc_set_input_format): there are no maps"; return 1; }
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H;
    hipError_t e = ADC_HIP(hipStreamSynchronize(h->stream));
    if (e == hipSuccess && map_x) e = ADC_HIP(hipMemcpy(map_x, r.mx, P * 4, hipMemcpyDeviceToHost));
    if (e == hipSuccess && map_y) e = ADC_HIP(hipMemcpy(map_y, r.my, P * 4, hipMemcpyDeviceToHost));
    if (e == hipSuccess && valid) e = ADC_HIP(hipMemcpy(valid, r.valid, P, hipMemcpyDeviceToHost));
    if (e != hipSuccess) { set_error("adc_get_rectify_maps", e); return 2; }
    return 0;
}

int adc_rectify_device(adc_handle* h, int side, const void* d_raw, void* d_bgr_out)
{
    if (!h || !d_raw || !d_bgr_out || (side != ADC_SIDE_LEFT && side != ADC_SIDE_RIGHT)) return 1;
    if (!h->rect[side].set) { g_last_error = "adc_rectify_device: this side is not set"; return 1; }
    if (raw_address_refused(h, side, d_raw, "adc_rectify_device")) return 1;
    hipSetDevice(h->device);
    const hipError_t e = ADC_HIP(launch_rect_side(h, side, static_cast<const uint8_t*>(d_raw), static_cast<uint8_t*>(d_bgr_out)));
    if (e != hipSuccess) return fail_match(h, "adc_rectify_device", e);
    return 0;
}

// ------------------------------------------------------------------------------ evaluation against ground truth (k_eval.hip)
// Handle state like the rectification: a set call uploads the caller's arrays one after the other into one raw buffer, decodes each
// into its float map, builds the occlusion byte map and waits.  An evaluation is a memset of the report words, one kernel and the
// read-back of the words into a pinned block, all on the object stream; adc_wait moves the block into the handle's report.
static int gt_bpp(int format) { return format == ADC_GT_U8 ? 1 : (format == ADC_GT_U16 ? 2 : 4); }

// 0 = usable; otherwise the reason.  pitch_out: the row pitch in bytes (0 in the struct: tightly packed)
static const char* gt_check(const adc_handle* h, const adc_gt* g, bool geometry, int* pitch_out)
{
    if (!g->data) return "null ground-truth array";
    if (g->format != ADC_GT_U8 && g->format != ADC_GT_U16 && g->format != ADC_GT_F32) return "unknown ground-truth format";
    if (!(__builtin_isfinite(g->scale) && g->scale > 0.0f)) return "scale must be finite and > 0";
    if (g->pitch_bytes < 0) return "pitch_bytes is negative";
    if (!geometry) return nullptr;
    const long long row = (long long)h->p.W * gt_bpp(g->format);
    const long long pitch = g->pitch_bytes ? (long long)g->pitch_bytes : row;
    if (pitch < row) return "pitch_bytes is smaller than a row";
    if (pitch * (long long)h->p.H > 2147483647LL) return "a ground-truth array must be smaller than 2 GiB";
    *pitch_out = (int)pitch;
    return nullptr;
}

static hipError_t gt_buffers(adc_handle* h, size_t raw_bytes)
{
    const size_t P = (size_t)h->p.W * h->p.H;
    if (!h->ev_cus) {
        int cus = 0;
        HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        h->ev_cus = cus > 0 ? cus : 1;
    }
    for (int s = 0; s < 2; s++) HIP_TRY(MEM_ONCE(h->ev_g[s], P * 4));
    HIP_TRY(MEM_ONCE(h->ev_occ, P));
    HIP_TRY(MEM_ONCE(h->ev_rep, adc_eval_report_words() * sizeof(uint64_t)));
    HIP_TRY(MEM_ONCE_PINNED(h->ev_pin, adc_eval_report_words() * sizeof(uint64_t)));
    return MEM_GROW(h->ev_raw, h->ev_raw_cap, raw_bytes, 1);
}

static hipError_t gt_install(adc_handle* h, const adc_gt* left, int pitch_l, const adc_gt* right, int pitch_r, const uint8_t* nonocc, float occ_thres)
{
    const size_t P = (size_t)h->p.W * h->p.H, H = (size_t)h->p.H;
    // (the caller's last row need not be padded to the pitch: H - 1 pitches and one row are read)
    const size_t bytes_l = (size_t)pitch_l * (H - 1) + (size_t)h->p.W * gt_bpp(left->format);
    const size_t bytes_r = right ? (size_t)pitch_r * (H - 1) + (size_t)h->p.W * gt_bpp(right->format) : 0;
    size_t need = bytes_l > bytes_r ? bytes_l : bytes_r;
    if (!right && nonocc && P > need) need = P;
    const hipError_t eb = gt_buffers(h, need); // (every HIP call in there is hooked itself)
    if (eb != hipSuccess) return eb;
    // (the stream is drained between the uploads: the raw buffer is reused, and a pageable source must not be read after the call)
    HIP_OK(hipMemcpyAsync(h->ev_raw, left->data, bytes_l, hipMemcpyHostToDevice, h->stream));
    HIP_OK(adc_launch_eval_gt(h, 0, left->format, pitch_l, left->scale));
    if (right) {
        HIP_OK(hipStreamSynchronize(h->stream));
        HIP_OK(hipMemcpyAsync(h->ev_raw, right->data, bytes_r, hipMemcpyHostToDevice, h->stream));
        HIP_OK(adc_launch_eval_gt(h, 1, right->format, pitch_r, right->scale));
        HIP_OK(adc_launch_eval_occ(h, 1, occ_thres));
    } else if (nonocc) {
        HIP_OK(hipStreamSynchronize(h->stream));
        HIP_OK(hipMemcpyAsync(h->ev_raw, nonocc, P, hipMemcpyHostToDevice, h->stream));
        HIP_OK(adc_launch_eval_occ(h, 2, occ_thres));
    } else {
        HIP_OK(hipMemsetAsync(h->ev_occ, 0, P, h->stream));
    }
    HIP_OK(hipStreamSynchronize(h->stream));
    return hipSuccess;
}

int adc_set_ground_truth(adc_handle* h, const adc_gt* left, const adc_gt* right, const uint8_t* nonocc, float occ_thres)
{
    if (!h) { g_last_error = "adc_set_ground_truth: null handle"; return 1; }
    if (!left) { g_last_error = "adc_set_ground_truth: null left ground truth"; return 1; }
    int pitch_l = 0, pitch_r = 0;
    const char* why = gt_check(h, left, false, &pitch_l);
    if (!why && right) why = gt_check(h, right, false, &pitch_r);
    if (!why && !(__builtin_isfinite(occ_thres) && occ_thres >= 0.0f)) why = "occ_thres must be finite and >= 0";
    if (!why && match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    if (!why) why = gt_check(h, left, true, &pitch_l);
    if (!why && right) why = gt_check(h, right, true, &pitch_r);
    if (why) { g_last_error = std::string("adc_set_ground_truth: ") + why; return 1; }
    hipSetDevice(h->device);
    h->ev_set = 0; // (a failure below leaves ground truth unset: the maps may be half written)
    if (gt_install(h, left, pitch_l, right, pitch_r, nonocc, occ_thres) != hipSuccess) return fail_call(h, "adc_set_ground_truth");
    h->ev_has_right = right ? 1 : 0;
    h->ev_has_mask = (!right && nonocc) ? 1 : 0;
    h->ev_occ_thres = occ_thres;
    h->ev_set = 1;
    return 0;
}

int adc_clear_ground_truth(adc_handle* h)
{
    if (!h) { g_last_error = "adc_clear_ground_truth: null handle"; return 1; }
    if (match_in_flight(h)) { g_last_error = "adc_clear_ground_truth: a Match is pending (adc_wait first)"; return 1; }
    h->ev_set = 0;
    return 0;
}

// validates an evaluation request; fills the four thresholds the kernel takes (unused: +inf).  0, or 1 with adc_last_error
static int eval_check(adc_handle* h, const void* disp, const void* prov, const void* conf, const adc_eval_params* params, float* t, int* n_out, const char* who)
{
    const char* why = nullptr;
    int n = 1;
    t[0] = 1.0f;
    if (!h) why = "null handle";
    else if (!disp) why = "null map";
    else if (params && (params->n_thresholds < 0 || params->n_thresholds > ADC_EVAL_MAX_THRESHOLDS)) why = "at most 4 thresholds";
    else if (conf && !prov) why = "a confidence map needs a provenance map";
    if (!why && params) {
        n = params->n_thresholds;
        for (int k = 0; k < n; k++) {
            t[k] = params->thresholds[k];
            if (!(__builtin_isfinite(t[k]) && t[k] >= 0.0f)) why = "a threshold must be finite and >= 0";
        }
    }
    if (!why && !h->ev_set) why = "no ground truth set (adc_set_ground_truth)";
    if (!why && match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    for (int k = n; k < ADC_EVAL_MAX_THRESHOLDS; k++) t[k] = ADC_INVALID_FLOAT;
    *n_out = n;
    return 0;
}

static hipError_t enqueue_evaluation(adc_handle* h, const float* disp, const uint8_t* prov, const float* conf, const float* t, float* err, uint8_t* cls)
{
    const size_t bytes = adc_eval_report_words() * sizeof(uint64_t);
    HIP_OK(hipMemsetAsync(h->ev_rep, 0, bytes, h->stream));
    HIP_OK(adc_launch_eval_measure(h, disp, prov, conf, t, err, cls));
    HIP_OK(hipMemcpyAsync(h->ev_pin, h->ev_rep, bytes, hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

static int evaluate_device_impl(adc_handle* h, const void* d_disp, const void* d_prov, const void* d_conf, const float* t, int n, void* d_err, void* d_class,
                                const char* who)
{
    hipSetDevice(h->device);
    if (enqueue_evaluation(h, static_cast<const float*>(d_disp), static_cast<const uint8_t*>(d_prov), static_cast<const float*>(d_conf), t,
                           static_cast<float*>(d_err), static_cast<uint8_t*>(d_class)) != hipSuccess)
        return fail_call(h, who);
    memset(&h->ev_echo, 0, sizeof(h->ev_echo));
    for (int k = 0; k < n; k++) h->ev_echo.thresholds[k] = t[k];
    h->ev_echo.n_thresholds = n;
    h->ev_echo.occ_thres = h->ev_occ_thres;
    h->ev_echo.has_right_gt = (uint8_t)h->ev_has_right;
    h->ev_echo.has_nonocc_mask = (uint8_t)h->ev_has_mask;
    h->ev_echo.has_provenance = d_prov ? 1 : 0;
    h->ev_echo.has_confidence = d_conf ? 1 : 0;
    h->fly.ev_pending = 1;
    return 0;
}

int adc_evaluate_device(adc_handle* h, const void* d_disp, const void* d_provenance, const void* d_confidence, const adc_eval_params* params,
                        void* d_err, void* d_class)
{
    float t[ADC_EVAL_MAX_THRESHOLDS];
    int n = 0;
    if (eval_check(h, d_disp, d_provenance, d_confidence, params, t, &n, "adc_evaluate_device") != 0) return 1;
    return evaluate_device_impl(h, d_disp, d_provenance, d_confidence, t, n, d_err, d_class, "adc_evaluate_device");
}

int adc_evaluate(adc_handle* h, const float* disp, const uint8_t* provenance, const float* confidence, const adc_eval_params* params, float* err,
                 uint8_t* eval_class, adc_eval_report* out)
{
    float t[ADC_EVAL_MAX_THRESHOLDS];
    int n = 0;
    if (eval_check(h, disp, provenance, confidence, params, t, &n, "adc_evaluate") != 0) return 1;
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H;
    hipError_t e = MEM_ONCE(h->evs_disp, P * 4);
    if (e == hipSuccess && provenance) e = MEM_ONCE(h->evs_prov, P);
    if (e == hipSuccess && confidence) e = MEM_ONCE(h->evs_conf, P * 4);
    if (e == hipSuccess && err) e = MEM_ONCE(h->evs_err, P * 4);
    if (e == hipSuccess && eval_class) e = MEM_ONCE(h->evs_cls, P);
    if (e != hipSuccess) return scratch_failed("adc_evaluate");
    e = ADC_HIP(hipMemcpy(h->evs_disp, disp, P * 4, hipMemcpyHostToDevice));
    if (e == hipSuccess && provenance) e = ADC_HIP(hipMemcpy(h->evs_prov, provenance, P, hipMemcpyHostToDevice));
    if (e == hipSuccess && confidence) e = ADC_HIP(hipMemcpy(h->evs_conf, confidence, P * 4, hipMemcpyHostToDevice));
    if (e != hipSuccess) { set_error("adc_evaluate: upload", e); (void)hipGetLastError(); return 2; }
    int rc = evaluate_device_impl(h, h->evs_disp, provenance ? h->evs_prov : nullptr, confidence ? h->evs_conf : nullptr, t, n, err ? h->evs_err : nullptr,
                                  eval_class ? h->evs_cls : nullptr, "adc_evaluate");
    if (rc == 0) rc = adc_wait(h);
    if (rc != 0) return rc;
    if (err && (e = ADC_HIP(hipMemcpy(err, h->evs_err, P * 4, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_evaluate: error map copy-out", e); return 2; }
    if (eval_class && (e = ADC_HIP(hipMemcpy(eval_class, h->evs_cls, P, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_evaluate: class map copy-out", e); return 2; }
    if (out) *out = h->ev_report;
    return 0;
}

int adc_get_eval_report(adc_handle* h, adc_eval_report* out)
{
    if (!h || !out) { g_last_error = "adc_get_eval_report: null argument"; return 1; }
    if (!h->ev_report_valid) { g_last_error = "adc_get_eval_report: no evaluation has completed on this handle"; return 1; }
    *out = h->ev_report;
    return 0;
}

// ------------------------------------------------------------------------------ registration into a second camera (k_register.hip)
// Handle state (the target) plus entry points in the style of the evaluation: the device forms enqueue on the object stream and are
// completed by adc_wait, which moves the pinned report words into reg_report.
static const char* reg_target_why(const adc_reg_target* t)
{
    if (t->width < 1 || t->width > 32767 || t->height < 1 || t->height > 32767) return "the target's width and height must lie in [1, 32767]";
    const float f[] = {t->fx, t->fy, t->cx, t->cy, t->k1, t->k2, t->p1, t->p2, t->k3, t->R[0], t->R[1], t->R[2], t->R[3], t->R[4],
                       t->R[5], t->R[6], t->R[7], t->R[8], t->t[0], t->t[1], t->t[2]};
    for (float v : f) if (!__builtin_isfinite(v)) return "the target has a non-finite field";
    if (t->fx == 0.0f || t->fy == 0.0f) return "the target's fx and fy must not be 0";
    return nullptr;
}

static hipError_t reg_buffers(adc_handle* h, size_t Pt)
{
    if (!h->reg_cus) {
        int cus = 0;
        HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        h->reg_cus = cus > 0 ? cus : 1;
    }
    HIP_TRY(MEM_ONCE(h->reg_rep, sizeof(adc_reg_report)));
    HIP_TRY(MEM_ONCE_PINNED(h->reg_pin, sizeof(adc_reg_report)));
    return MEM_GROW(h->reg_zbuf, h->reg_zbuf_cap, Pt, sizeof(uint64_t));
}

int adc_set_register_target(adc_handle* h, const adc_reg_target* target)
{
    if (!h) { g_last_error = "adc_set_register_target: null handle"; return 1; }
    if (!target) { g_last_error = "adc_set_register_target: null target"; return 1; }
    const char* why = reg_target_why(target);
    if (!why && match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    if (why) { g_last_error = std::string("adc_set_register_target: ") + why; return 1; }
    hipSetDevice(h->device);
    // (an earlier registration may still read the z-buffer that is about to be regrown)
    hipError_t e = ADC_HIP(hipStreamSynchronize(h->stream));
    if (e != hipSuccess) set_error("hipStreamSynchronize(h->stream)", e);
    h->reg_set = 0; // (a failure below leaves the target unset)
    if (e == hipSuccess) e = reg_buffers(h, (size_t)target->width * (size_t)target->height);
    if (e != hipSuccess) return fail_call(h, "adc_set_register_target");
    h->reg_target = *target;
    h->reg_set = 1;
    return 0;
}

int adc_clear_register_target(adc_handle* h)
{
    if (!h) { g_last_error = "adc_clear_register_target: null handle"; return 1; }
    if (match_in_flight(h)) { g_last_error = "adc_clear_register_target: a Match is pending (adc_wait first)"; return 1; }
    h->reg_set = 0;
    return 0;
}

// validates the part every registration request shares; 0, or 1 with adc_last_error
// (extra: what the entry point itself found wrong with its other arguments, reported behind the shared ones and in front of the handle's state)
static int reg_check(adc_handle* h, const void* map, int input_kind, const adc_calib* calib, const char* extra, const char* who)
{
    const char* why = nullptr;
    if (!h) why = "null handle";
    else if (!map) why = "null map";
    else if (!calib) why = "null calibration";
    else if (input_kind != ADC_REG_FROM_DISPARITY && input_kind != ADC_REG_FROM_DEPTH) why = "unknown input kind";
    else if (!(__builtin_isfinite(calib->focal_px) && __builtin_isfinite(calib->baseline) && __builtin_isfinite(calib->cx) && __builtin_isfinite(calib->cy) &&
               __builtin_isfinite(calib->doffs)))
        why = "the calibration has a non-finite field";
    else if (!(calib->focal_px > 0.0f)) why = "the calibration's focal_px must be positive";
    else if (extra) why = extra;
    else if (!h->reg_set) why = "no target set (adc_set_register_target)";
    else if (match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    return 0;
}

static const char* reg_request_why(uint32_t flags, bool any_output)
{
    if (flags & ~(ADC_REG_NO_SPLAT | ADC_REG_PRETEST)) return "unknown flag";
    return any_output ? nullptr : "no output requested";
}

static hipError_t enqueue_registration(adc_handle* h, const float* map, int kind, const adc_calib* calib, uint32_t flags, float* depth, int32_t* index)
{
    const size_t Pt = (size_t)h->reg_target.width * (size_t)h->reg_target.height;
    HIP_OK(hipMemsetAsync(h->reg_zbuf, 0xff, Pt * sizeof(uint64_t), h->stream));
    HIP_OK(hipMemsetAsync(h->reg_rep, 0, sizeof(adc_reg_report), h->stream));
    HIP_OK(adc_launch_reg_scatter(h, map, kind, calib, flags));
    HIP_OK(adc_launch_reg_resolve(h, depth, index));
    HIP_OK(hipMemcpyAsync(h->reg_pin, h->reg_rep, sizeof(adc_reg_report), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

int adc_register_depth_device(adc_handle* h, const void* d_map, int input_kind, const adc_calib* calib, uint32_t flags, void* d_depth, void* d_index)
{
    const char* who = "adc_register_depth_device";
    if (reg_check(h, d_map, input_kind, calib, reg_request_why(flags, d_depth || d_index), who) != 0) return 1;
    hipSetDevice(h->device);
    if (enqueue_registration(h, static_cast<const float*>(d_map), input_kind, calib, flags, static_cast<float*>(d_depth), static_cast<int32_t*>(d_index)) != hipSuccess)
        return fail_call(h, who);
    h->fly.reg_pending = 1;
    return 0;
}

int adc_align_color_device(adc_handle* h, const void* d_map, int input_kind, const adc_calib* calib, const void* d_target_bgr, void* d_bgr_out, void* d_valid)
{
    const char* who = "adc_align_color_device";
    if (reg_check(h, d_map, input_kind, calib, !d_target_bgr ? "null target image" : (!d_bgr_out ? "no output requested" : nullptr), who) != 0) return 1;
    hipSetDevice(h->device);
    const hipError_t e = ADC_HIP(adc_launch_reg_align(h, static_cast<const float*>(d_map), input_kind, calib, static_cast<const uint8_t*>(d_target_bgr),
                                                      static_cast<uint8_t*>(d_bgr_out), static_cast<uint8_t*>(d_valid)));
    if (e != hipSuccess) { set_error("adc_launch_reg_align", e); return fail_call(h, who); }
    return 0;
}

int adc_register_depth(adc_handle* h, const float* map, int input_kind, const adc_calib* calib, uint32_t flags, float* depth, int32_t* index, adc_reg_report* report)
{
    const char* who = "adc_register_depth";
    if (reg_check(h, map, input_kind, calib, reg_request_why(flags, depth || index), who) != 0) return 1;
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H, Pt = (size_t)h->reg_target.width * (size_t)h->reg_target.height;
    hipError_t e = MEM_ONCE(h->regs_map, P * 4);
    if (e == hipSuccess && depth) e = MEM_GROW(h->regs_depth, h->regs_depth_cap, Pt, 4);
    if (e == hipSuccess && index) e = MEM_GROW(h->regs_index, h->regs_index_cap, Pt, 4);
    if (e != hipSuccess) return scratch_failed(who);
    if ((e = ADC_HIP(hipMemcpy(h->regs_map, map, P * 4, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_register_depth: upload", e); (void)hipGetLastError(); return 2; }
    int rc = adc_register_depth_device(h, h->regs_map, input_kind, calib, flags, depth ? h->regs_depth : nullptr, index ? h->regs_index : nullptr);
    if (rc == 0) rc = adc_wait(h);
    if (rc != 0) return rc;
    if (depth && (e = ADC_HIP(hipMemcpy(depth, h->regs_depth, Pt * 4, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_register_depth: depth copy-out", e); return 2; }
    if (index && (e = ADC_HIP(hipMemcpy(index, h->regs_index, Pt * 4, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_register_depth: index copy-out", e); return 2; }
    if (report) *report = h->reg_report;
    return 0;
}

int adc_align_color(adc_handle* h, const float* map, int input_kind, const adc_calib* calib, const uint8_t* target_bgr, uint8_t* bgr_out, uint8_t* valid)
{
    const char* who = "adc_align_color";
    if (reg_check(h, map, input_kind, calib, !target_bgr ? "null target image" : (!bgr_out ? "no output requested" : nullptr), who) != 0) return 1;
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H, Pt = (size_t)h->reg_target.width * (size_t)h->reg_target.height;
    hipError_t e = MEM_ONCE(h->regs_map, P * 4);
    if (e == hipSuccess) e = MEM_ONCE(h->regs_out, P * 3);
    if (e == hipSuccess && valid) e = MEM_ONCE(h->regs_valid, P);
    if (e == hipSuccess) e = MEM_GROW(h->regs_tbgr, h->regs_tbgr_cap, Pt, 3);
    if (e != hipSuccess) return scratch_failed(who);
    e = ADC_HIP(hipMemcpy(h->regs_map, map, P * 4, hipMemcpyHostToDevice));
    if (e == hipSuccess) e = ADC_HIP(hipMemcpy(h->regs_tbgr, target_bgr, Pt * 3, hipMemcpyHostToDevice));
    if (e != hipSuccess) { set_error("adc_align_color: upload", e); (void)hipGetLastError(); return 2; }
    int rc = adc_align_color_device(h, h->regs_map, input_kind, calib, h->regs_tbgr, h->regs_out, valid ? h->regs_valid : nullptr);
    if (rc == 0) rc = adc_wait(h);
    if (rc != 0) return rc;
    if ((e = ADC_HIP(hipMemcpy(bgr_out, h->regs_out, P * 3, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_align_color: image copy-out", e); return 2; }
    if (valid && (e = ADC_HIP(hipMemcpy(valid, h->regs_valid, P, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_align_color: valid map copy-out", e); return 2; }
    return 0;
}

int adc_get_register_report(adc_handle* h, adc_reg_report* out)
{
    if (!h || !out) { g_last_error = "adc_get_register_report: null argument"; return 1; }
    if (!h->reg_report_valid) { g_last_error = "adc_get_register_report: no registration has completed on this handle"; return 1; }
    *out = h->reg_report;
    return 0;
}

// ------------------------------------------------------------------------------ surface normals from a disparity map (k_normals.hip)
// Stand-alone entry points in the style of the registration: the device form enqueues on the object stream and is completed by
// adc_wait, which moves the four report words from pin_flags[ADC_PIN_NORMALS..] into nrm_report.
static const adc_normals_params NRM_DEFAULT = {2, 1.0f, 5, 0u, {0u, 0u, 0u, 0u}};

// validates a request; 0 with *p and *G filled, or 1 with adc_last_error (device: the outputs are device addresses -> alignment)
static int nrm_check(adc_handle* h, const void* map, const adc_calib* calib, const adc_normals_params* params, const void* normals, const void* normals8, bool device,
                     adc_normals_params* p, int32_t* G, const char* who)
{
    const char* why = nullptr;
    *p = params ? *params : NRM_DEFAULT;
    if (!h) why = "null handle";
    else if (!map) why = "null map";
    else if (!calib) why = "null calibration";
    else if (!(__builtin_isfinite(calib->focal_px) && __builtin_isfinite(calib->baseline) && __builtin_isfinite(calib->cx) && __builtin_isfinite(calib->cy) &&
               __builtin_isfinite(calib->doffs)))
        why = "the calibration has a non-finite field";
    else if (!(calib->focal_px > 0.0f)) why = "the calibration's focal_px must be positive";
    else if (p->radius < 1 || p->radius > ADC_NORMALS_MAX_RADIUS) why = "radius must lie in [1, 7]";
    else if (!(__builtin_isfinite(p->max_diff) && p->max_diff > 0.0f && p->max_diff <= 64.0f)) why = "max_diff must be finite and lie in (0, 64]";
    else if (p->min_points < 3 || p->min_points > (2 * p->radius + 1) * (2 * p->radius + 1)) why = "min_points must lie in [3, (2 * radius + 1)^2]";
    else if (p->flags != 0u) why = "unknown flag";
    else if (p->reserved_[0] | p->reserved_[1] | p->reserved_[2] | p->reserved_[3]) why = "a reserved word is not 0";
    else if (!normals && !normals8) why = "no output requested";
    else if (device && ((uintptr_t)normals & 15u)) why = "d_normals must be 16-byte aligned";
    else if (device && ((uintptr_t)normals8 & 3u)) why = "d_normals8 must be 4-byte aligned";
    else if (device && ((uintptr_t)map & 3u)) why = "d_disp must be 4-byte aligned";
    else if (match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    *G = (int32_t)__builtin_rintf(p->max_diff * 1024.0f);
    return 0;
}

static hipError_t enqueue_normals(adc_handle* h, const float* map, const adc_calib* calib, const adc_normals_params& p, int32_t G, float* normals, uint8_t* normals8)
{
    HIP_TRY(MEM_ONCE(h->nrm_rep, sizeof(adc_normals_report)));
    HIP_OK(hipMemsetAsync(h->nrm_rep, 0, sizeof(adc_normals_report), h->stream));
    HIP_OK(adc_launch_normals(h, map, calib, p.radius, G, p.min_points, normals, normals8));
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_NORMALS, h->nrm_rep, sizeof(adc_normals_report), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

int adc_normals_device(adc_handle* h, const void* d_disp, const adc_calib* calib, const adc_normals_params* params, void* d_normals, void* d_normals8)
{
    const char* who = "adc_normals_device";
    adc_normals_params p;
    int32_t G = 0;
    if (nrm_check(h, d_disp, calib, params, d_normals, d_normals8, true, &p, &G, who) != 0) return 1;
    hipSetDevice(h->device);
    if (enqueue_normals(h, static_cast<const float*>(d_disp), calib, p, G, static_cast<float*>(d_normals), static_cast<uint8_t*>(d_normals8)) != hipSuccess)
        return fail_call(h, who);
    h->fly.nrm_pending = 1;
    return 0;
}

int adc_normals(adc_handle* h, const float* disp, const adc_calib* calib, const adc_normals_params* params, float* normals, uint8_t* normals8, adc_normals_report* report)
{
    const char* who = "adc_normals";
    adc_normals_params p;
    int32_t G = 0;
    if (nrm_check(h, disp, calib, params, normals, normals8, false, &p, &G, who) != 0) return 1;
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H;
    hipError_t e = MEM_ONCE(h->nrms_map, P * 4);
    if (e == hipSuccess && normals) e = MEM_ONCE(h->nrms_out, P * 16);
    if (e == hipSuccess && normals8) e = MEM_ONCE(h->nrms_out8, P * 4);
    if (e != hipSuccess) return scratch_failed(who);
    if ((e = ADC_HIP(hipMemcpy(h->nrms_map, disp, P * 4, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_normals: upload", e); (void)hipGetLastError(); return 2; }
    int rc = adc_normals_device(h, h->nrms_map, calib, &p, normals ? h->nrms_out : nullptr, normals8 ? h->nrms_out8 : nullptr);
    if (rc == 0) rc = adc_wait(h);
    if (rc != 0) return rc;
    if (normals && (e = ADC_HIP(hipMemcpy(normals, h->nrms_out, P * 16, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_normals: normals copy-out", e); return 2; }
    if (normals8 && (e = ADC_HIP(hipMemcpy(normals8, h->nrms_out8, P * 4, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_normals: normals8 copy-out", e); return 2; }
    if (report) *report = h->nrm_report;
    return 0;
}

int adc_get_normals_report(adc_handle* h, adc_normals_report* out)
{
    if (!h || !out) { g_last_error = "adc_get_normals_report: null argument"; return 1; }
    if (!h->nrm_report_valid) { g_last_error = "adc_get_normals_report: no normals call has completed on this handle"; return 1; }
    *out = h->nrm_report;
    return 0;
}

// ------------------------------------------------------------------------------ triangle mesh from a disparity map (k_mesh.hip)
// Stand-alone entry points in the style of the normals: the device form enqueues on the object stream and is completed by adc_wait,
// which moves the five report counts from pin_flags[ADC_PIN_MESH..] into msh_report.
static const adc_mesh_params MSH_DEFAULT = {1.0f, 1, 0u, {0u, 0u, 0u, 0u, 0u}};

// validates a request; 0 with *p filled, or 1 with adc_last_error (device: the outputs are device addresses -> alignment)
static int msh_check(adc_handle* h, const void* map, const void* img, const adc_calib* calib, const adc_mesh_params* params, const void* vertices, const void* vindex,
                     const void* triangles, const void* counts, bool device, adc_mesh_params* p, const char* who)
{
    const char* why = nullptr;
    *p = params ? *params : MSH_DEFAULT;
    if (!h) why = "null handle";
    else if (!map) why = "null map";
    else if (calib && !(__builtin_isfinite(calib->focal_px) && __builtin_isfinite(calib->baseline) && __builtin_isfinite(calib->cx) && __builtin_isfinite(calib->cy) &&
                        __builtin_isfinite(calib->doffs)))
        why = "the calibration has a non-finite field";
    else if (calib && !(calib->focal_px > 0.0f)) why = "the calibration's focal_px must be positive";
    else if (!(p->max_diff >= 0.0f)) why = "max_diff must not be NaN and must be >= 0";
    else if (p->step < 1 || p->step > ADC_MESH_MAX_STEP) why = "step must lie in [1, 16]";
    else if (p->flags != 0u) why = "unknown flag";
    else if (p->reserved_[0] | p->reserved_[1] | p->reserved_[2] | p->reserved_[3] | p->reserved_[4]) why = "a reserved word is not 0";
    else if (!vertices && !triangles) why = "no output requested (neither vertices nor triangles)";
    else if (vindex && !vertices) why = "a vertex_index needs vertices";
    else if (device && ((uintptr_t)vertices & 15u)) why = "d_vertices must be 16-byte aligned";
    else if (device && (((uintptr_t)vindex | (uintptr_t)triangles | (uintptr_t)counts | (uintptr_t)map) & 3u)) why = "d_disp, d_vertex_index, d_triangles and d_counts must be 4-byte aligned";
    else if (match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    (void)img; // (bytes: any address)
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    return 0;
}

static uint32_t msh_cap32(uint64_t c) { return c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c; } // (a mesh has fewer than 2^32 records)

static hipError_t enqueue_mesh(adc_handle* h, const AdcMeshReq& r)
{
    HIP_TRY(MEM_ONCE(h->msh_words, adc_mesh_scratch_bytes(h->p.W, h->p.H)));
    HIP_OK(hipMemsetAsync(h->msh_words, 0, sizeof(adc_mesh_report), h->stream));
    HIP_OK(adc_launch_mesh_measure(h, r));
    HIP_OK(adc_launch_mesh_scan(h, r));
    HIP_OK(adc_launch_mesh_emit(h, r));
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_MESH, h->msh_words, MSH_PIN_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

int adc_mesh_device(adc_handle* h, const void* d_disp, const void* d_bgr_left, const adc_calib* calib, const adc_mesh_params* params, void* d_vertices,
                    uint64_t vertex_capacity, void* d_vertex_index, void* d_triangles, uint64_t triangle_capacity, void* d_counts)
{
    const char* who = "adc_mesh_device";
    adc_mesh_params p;
    if (msh_check(h, d_disp, d_bgr_left, calib, params, d_vertices, d_vertex_index, d_triangles, d_counts, true, &p, who) != 0) return 1;
    hipSetDevice(h->device);
    AdcMeshReq r;
    r.disp = static_cast<const float*>(d_disp);
    r.img = static_cast<const uint8_t*>(d_bgr_left);
    r.calib = calib;
    r.max_diff = p.max_diff;
    r.step = p.step;
    r.vertices = d_vertices;
    r.vertex_index = static_cast<int32_t*>(d_vertex_index);
    r.triangles = static_cast<uint32_t*>(d_triangles);
    r.vertex_capacity = msh_cap32(vertex_capacity);
    r.triangle_capacity = msh_cap32(triangle_capacity);
    r.counts = static_cast<uint32_t*>(d_counts);
    if (enqueue_mesh(h, r) != hipSuccess) return fail_call(h, who);
    h->fly.msh_pending = 1;
    return 0;
}

int adc_mesh(adc_handle* h, const float* disp, const uint8_t* bgr_left, const adc_calib* calib, const adc_mesh_params* params, adc_point* vertices,
             uint64_t vertex_capacity, int32_t* vertex_index, uint32_t* triangles, uint64_t triangle_capacity, adc_mesh_report* report)
{
    const char* who = "adc_mesh";
    adc_mesh_params p;
    if (msh_check(h, disp, bgr_left, calib, params, vertices, vertex_index, triangles, nullptr, false, &p, who) != 0) return 1;
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H;
    // no more records than the lattice can give (a device buffer of at least one record stands for a capacity of 0: it counts only)
    const size_t Wl = (size_t)((h->p.W - 1) / p.step + 1), Hl = (size_t)((h->p.H - 1) / p.step + 1);
    const size_t vmax = Wl * Hl, tmax = 2 * (Wl - 1) * (Hl - 1);
    const size_t vcap = vertex_capacity < vmax ? (size_t)vertex_capacity : vmax, tcap = triangle_capacity < tmax ? (size_t)triangle_capacity : tmax;
    hipError_t e = MEM_ONCE(h->mshs_map, P * 4);
    if (e == hipSuccess && bgr_left) e = MEM_ONCE(h->mshs_img, P * 3);
    if (e == hipSuccess && vertices) e = MEM_GROW(h->mshs_vtx, h->mshs_vtx_cap, vcap ? vcap : 1, sizeof(adc_point));
    if (e == hipSuccess && vertex_index) e = MEM_GROW(h->mshs_vidx, h->mshs_vidx_cap, vcap ? vcap : 1, sizeof(int32_t));
    if (e == hipSuccess && triangles) e = MEM_GROW(h->mshs_tri, h->mshs_tri_cap, 3 * (tcap ? tcap : 1), sizeof(uint32_t));
    if (e != hipSuccess) return scratch_failed(who);
    if ((e = ADC_HIP(hipMemcpy(h->mshs_map, disp, P * 4, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_mesh: upload", e); (void)hipGetLastError(); return 2; }
    if (bgr_left && (e = ADC_HIP(hipMemcpy(h->mshs_img, bgr_left, P * 3, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_mesh: image upload", e); (void)hipGetLastError(); return 2; }
    int rc = adc_mesh_device(h, h->mshs_map, bgr_left ? h->mshs_img : nullptr, calib, &p, vertices ? h->mshs_vtx : nullptr, vcap, vertex_index ? h->mshs_vidx : nullptr,
                             triangles ? h->mshs_tri : nullptr, tcap, nullptr);
    if (rc == 0) rc = adc_wait(h);
    if (rc != 0) return rc;
    const size_t nv = h->msh_report.vertices < vcap ? h->msh_report.vertices : vcap, nt = h->msh_report.triangles < tcap ? h->msh_report.triangles : tcap;
    if (vertices && nv && (e = ADC_HIP(hipMemcpy(vertices, h->mshs_vtx, nv * sizeof(adc_point), hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_mesh: vertex copy-out", e); return 2; }
    if (vertex_index && nv && (e = ADC_HIP(hipMemcpy(vertex_index, h->mshs_vidx, nv * sizeof(int32_t), hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_mesh: vertex_index copy-out", e); return 2; }
    if (triangles && nt && (e = ADC_HIP(hipMemcpy(triangles, h->mshs_tri, nt * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_mesh: triangle copy-out", e); return 2; }
    if (report) *report = h->msh_report;
    return 0;
}

int adc_get_mesh_report(adc_handle* h, adc_mesh_report* out)
{
    if (!h || !out) { g_last_error = "adc_get_mesh_report: null argument"; return 1; }
    if (!h->msh_report_valid) { g_last_error = "adc_get_mesh_report: no mesh call has completed on this handle"; return 1; }
    *out = h->msh_report;
    return 0;
}

// ------------------------------------------------------------------------------ TSDF volume (k_tsdf.hip)
// The volume is handle state (tsdf_set, tsdf_params, tsdf_vol, tsdf_col).  The device forms of integrate and extract enqueue on the
// object stream in the style of the mesh and are completed by adc_wait, which moves their report counts from
// pin_flags[ADC_PIN_TSDF..] / pin_flags[ADC_PIN_TSDF_EXTRACT..] into tsdf_report / tsdf_xreport.  Like adc_mesh_device, neither looks at
// its own pending flag: calls may follow one another on the stream without a wait, and the report is that of the last.
static const adc_tsdf_extract_params TSDF_EXTRACT_DEFAULT = {1u, {0u, 0u, 0u, 0u, 0u, 0u, 0u}};

static size_t tsdf_voxels(const adc_tsdf_params& p) { return (size_t)p.nx * (size_t)p.ny * (size_t)p.nz; }

static void tsdf_release(adc_handle* h)
{
    dev_mem_release<HipMem>(&h->mem, &h->tsdf_vol);
    dev_mem_release<HipMem>(&h->mem, &h->tsdf_col);
    dev_mem_release<HipMem>(&h->mem, &h->tsdf_vol2); // (the second planes of a volume that was shifted: no call for one that was not)
    dev_mem_release<HipMem>(&h->mem, &h->tsdf_col2);
    h->tsdf_set = 0;
}

static hipError_t tsdf_clear(adc_handle* h, const adc_tsdf_params& p)
{
    HIP_OK(hipMemsetAsync(h->tsdf_vol, 0, tsdf_voxels(p) * sizeof(uint32_t), h->stream));
    if (h->tsdf_col) HIP_OK(hipMemsetAsync(h->tsdf_col, 0, tsdf_voxels(p) * sizeof(uint32_t), h->stream));
    return hipSuccess;
}

static hipError_t tsdf_allocate(adc_handle* h, const adc_tsdf_params& p)
{
    HIP_TRY(MEM_ONCE(h->tsdf_vol, tsdf_voxels(p) * sizeof(uint32_t)));
    if (p.flags & ADC_TSDF_COLOR) HIP_TRY(MEM_ONCE(h->tsdf_col, tsdf_voxels(p) * sizeof(uint32_t)));
    HIP_TRY(MEM_ONCE(h->tsdf_rep, ADC_TSDF_REP_WORDS * sizeof(uint32_t)));
    return tsdf_clear(h, p);
}

// the checks every call on an existing volume shares; null = go on
static const char* tsdf_state_refusal(adc_handle* h)
{
    if (!h->tsdf_set) return "no volume (adc_tsdf_create first)";
    if (match_in_flight(h)) return "a Match is pending (adc_wait first)";
    return nullptr;
}

int adc_tsdf_create(adc_handle* h, const adc_tsdf_params* params)
{
    const char* who = "adc_tsdf_create";
    const char* why = nullptr;
    if (!h) why = "null handle";
    else if (!params) why = "null params";
    else if ((why = tsdf_params_refusal(*params)) != nullptr) {}
    else if (match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    hipSetDevice(h->device);
    tsdf_release(h); // (hipFree waits for whatever still reads the old volume)
    if (tsdf_allocate(h, *params) != hipSuccess) {
        const int rc = fail_call(h, who);
        tsdf_release(h);
        return rc;
    }
    h->tsdf_params = *params;
    for (int a = 0; a < 3; a++) { h->tsdf_origin0[a] = params->origin[a]; h->tsdf_offset[a] = 0; }
    h->tsdf_set = 1;
    return 0;
}

int adc_tsdf_reset(adc_handle* h)
{
    const char* who = "adc_tsdf_reset";
    const char* why = !h ? "null handle" : tsdf_state_refusal(h);
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    hipSetDevice(h->device);
    if (tsdf_clear(h, h->tsdf_params) != hipSuccess) return fail_call(h, who);
    return 0;
}

int adc_tsdf_destroy(adc_handle* h)
{
    const char* why = !h ? "null handle" : match_in_flight(h) ? "a Match is pending (adc_wait first)" : nullptr;
    if (why) { g_last_error = std::string("adc_tsdf_destroy: ") + why; return 1; }
    if (!h->tsdf_set) return 0;
    hipSetDevice(h->device);
    tsdf_release(h);
    return 0;
}

static int tsdf_integrate_check(adc_handle* h, const void* map, const void* img, const adc_tsdf_frame* frame, bool device, const char* who)
{
    const char* why = nullptr;
    if (!h) why = "null handle";
    else if (!map) why = "null map";
    else if (!frame) why = "null frame";
    else if ((why = tsdf_frame_refusal(*frame)) != nullptr) {}
    else if (device && ((uintptr_t)map & 3u)) why = "d_map must be 4-byte aligned";
    else if ((why = tsdf_state_refusal(h)) != nullptr) {}
    else if (img && !(h->tsdf_params.flags & ADC_TSDF_COLOR)) why = "an image needs a colour volume (ADC_TSDF_COLOR)";
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    return 0;
}

static hipError_t enqueue_tsdf_integrate(adc_handle* h, const float* map, const uint8_t* img, const adc_tsdf_frame* frame)
{
    HIP_OK(hipMemsetAsync(h->tsdf_rep, 0, sizeof(adc_tsdf_report), h->stream));
    HIP_OK(adc_launch_tsdf_integrate(h, map, img, frame));
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_TSDF, h->tsdf_rep, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

int adc_tsdf_integrate_device(adc_handle* h, const void* d_map, const void* d_bgr_left, const adc_tsdf_frame* frame)
{
    const char* who = "adc_tsdf_integrate_device";
    if (tsdf_integrate_check(h, d_map, d_bgr_left, frame, true, who) != 0) return 1;
    hipSetDevice(h->device);
    if (enqueue_tsdf_integrate(h, static_cast<const float*>(d_map), static_cast<const uint8_t*>(d_bgr_left), frame) != hipSuccess) return fail_call(h, who);
    h->fly.tsdf_pending = 1;
    return 0;
}

int adc_tsdf_integrate(adc_handle* h, const float* map, const uint8_t* bgr_left, const adc_tsdf_frame* frame, adc_tsdf_report* report)
{
    const char* who = "adc_tsdf_integrate";
    if (tsdf_integrate_check(h, map, bgr_left, frame, false, who) != 0) return 1;
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H;
    hipError_t e = MEM_ONCE(h->tsdfs_map, P * 4);
    if (e == hipSuccess && bgr_left) e = MEM_ONCE(h->tsdfs_img, P * 3);
    if (e != hipSuccess) return scratch_failed(who);
    if ((e = ADC_HIP(hipMemcpy(h->tsdfs_map, map, P * 4, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_tsdf_integrate: upload", e); (void)hipGetLastError(); return 2; }
    if (bgr_left && (e = ADC_HIP(hipMemcpy(h->tsdfs_img, bgr_left, P * 3, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_tsdf_integrate: image upload", e); (void)hipGetLastError(); return 2; }
    int rc = adc_tsdf_integrate_device(h, h->tsdfs_map, bgr_left ? h->tsdfs_img : nullptr, frame);
    if (rc == 0) rc = adc_wait(h);
    if (rc != 0) return rc;
    if (report) *report = h->tsdf_report;
    return 0;
}

static int tsdf_extract_check(adc_handle* h, const adc_tsdf_extract_params* params, const void* points, uint64_t capacity, const void* count, bool device,
                              adc_tsdf_extract_params* p, const char* who)
{
    const char* why = nullptr;
    *p = params ? *params : TSDF_EXTRACT_DEFAULT;
    if (!h) why = "null handle";
    else if (p->min_weight < 1u || p->min_weight > 65535u) why = "min_weight must lie in [1, 65535]";
    else if (p->reserved_[0] | p->reserved_[1] | p->reserved_[2] | p->reserved_[3] | p->reserved_[4] | p->reserved_[5] | p->reserved_[6]) why = "a reserved word is not 0";
    else if (!points && capacity != 0) why = "null points with a capacity";
    else if (device && ((uintptr_t)points & 15u)) why = "d_points must be 16-byte aligned";
    else if (device && ((uintptr_t)count & 3u)) why = "d_count must be 4-byte aligned";
    else if ((why = tsdf_state_refusal(h)) != nullptr) {}
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    return 0;
}

static hipError_t enqueue_tsdf_extract(adc_handle* h, const AdcTsdfExtReq& r)
{
    HIP_TRY(MEM_GROW(h->tsdf_tiles, h->tsdf_tiles_cap, adc_tsdf_tile_count(&h->tsdf_params), sizeof(uint32_t)));
    HIP_OK(hipMemsetAsync(h->tsdf_rep + ADC_TSDF_REP_EXTRACT, 0, sizeof(adc_tsdf_extract_report), h->stream));
    HIP_OK(adc_launch_tsdf_measure(h, r));
    HIP_OK(adc_launch_tsdf_scan(h, r));
    if (r.points && r.capacity) HIP_OK(adc_launch_tsdf_emit(h, r));
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_TSDF_EXTRACT, h->tsdf_rep + ADC_TSDF_REP_EXTRACT, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

int adc_tsdf_extract_device(adc_handle* h, const adc_tsdf_extract_params* params, void* d_points, uint64_t capacity, void* d_count)
{
    const char* who = "adc_tsdf_extract_device";
    adc_tsdf_extract_params p;
    if (tsdf_extract_check(h, params, d_points, capacity, d_count, true, &p, who) != 0) return 1;
    hipSetDevice(h->device);
    AdcTsdfExtReq r;
    r.min_weight = p.min_weight;
    r.points = d_points;
    r.capacity = msh_cap32(capacity);
    r.count = static_cast<uint32_t*>(d_count);
    if (enqueue_tsdf_extract(h, r) != hipSuccess) return fail_call(h, who);
    h->fly.tsdfx_pending = 1;
    return 0;
}

int adc_tsdf_extract(adc_handle* h, const adc_tsdf_extract_params* params, adc_point* points, uint64_t capacity, adc_tsdf_extract_report* report)
{
    const char* who = "adc_tsdf_extract";
    adc_tsdf_extract_params p;
    if (tsdf_extract_check(h, params, points, capacity, nullptr, false, &p, who) != 0) return 1;
    hipSetDevice(h->device);
    // no more records than the volume can give: three crossings per voxel
    const size_t most = 3 * tsdf_voxels(h->tsdf_params);
    size_t cap = capacity < most ? (size_t)capacity : most;
    hipError_t e = hipSuccess;
    int rc = 0;
    if (points && cap > h->tsdfs_pts_cap) {
        // the point scratch would have to grow: count first, so that it never holds more records than the volume has crossings (a
        // generous capacity on a 512^3 volume would otherwise pin up to 6 GB until adc_destroy)
        rc = adc_tsdf_extract_device(h, &p, nullptr, 0, nullptr);
        if (rc == 0) rc = adc_wait(h);
        if (rc != 0) return rc;
        if (h->tsdf_xreport.points < cap) cap = h->tsdf_xreport.points;
        if (cap == 0) { // (no crossing: the counting pass was the call)
            if (report) *report = h->tsdf_xreport;
            return 0;
        }
    }
    if (points && cap && (e = MEM_GROW(h->tsdfs_pts, h->tsdfs_pts_cap, cap, sizeof(adc_point))) != hipSuccess) return scratch_failed(who);
    rc = adc_tsdf_extract_device(h, &p, points && cap ? h->tsdfs_pts : nullptr, points ? cap : 0, nullptr);
    if (rc == 0) rc = adc_wait(h);
    if (rc != 0) return rc;
    const size_t n = h->tsdf_xreport.points < cap ? h->tsdf_xreport.points : cap;
    if (points && n && (e = ADC_HIP(hipMemcpy(points, h->tsdfs_pts, n * sizeof(adc_point), hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_tsdf_extract: copy-out", e); return 2; }
    if (report) *report = h->tsdf_xreport;
    return 0;
}

int adc_get_tsdf_report(adc_handle* h, adc_tsdf_report* integrate_report, adc_tsdf_extract_report* extract_report)
{
    if (!h || (!integrate_report && !extract_report)) { g_last_error = "adc_get_tsdf_report: null argument"; return 1; }
    if (integrate_report && !h->tsdf_report_valid) { g_last_error = "adc_get_tsdf_report: no integrate call has completed on this handle"; return 1; }
    if (extract_report && !h->tsdf_xreport_valid) { g_last_error = "adc_get_tsdf_report: no extract call has completed on this handle"; return 1; }
    if (integrate_report) *integrate_report = h->tsdf_report;
    if (extract_report) *extract_report = h->tsdf_xreport;
    return 0;
}

int adc_tsdf_get_volume_device(adc_handle* h, void** d_tsdf, void** d_color, adc_tsdf_params* params)
{
    const char* why = !h ? "null handle" : !h->tsdf_set ? "no volume (adc_tsdf_create first)" : nullptr;
    if (why) { g_last_error = std::string("adc_tsdf_get_volume_device: ") + why; return 1; }
    if (d_tsdf) *d_tsdf = h->tsdf_vol;
    if (d_color) *d_color = h->tsdf_col;
    if (params) *params = h->tsdf_params;
    return 0;
}

// the whole volume to (to_host) or from the host: waits for the stream, then one blocking copy per plane of words
static int tsdf_transfer(adc_handle* h, void* tsdf, void* color, bool to_host, const char* who)
{
    const char* why = nullptr;
    if (!h) why = "null handle";
    else if (!tsdf) why = "null tsdf";
    else if ((why = tsdf_state_refusal(h)) != nullptr) {}
    else if (color && !h->tsdf_col) why = "a colour pointer needs a colour volume (ADC_TSDF_COLOR)";
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    hipSetDevice(h->device);
    const size_t bytes = tsdf_voxels(h->tsdf_params) * sizeof(uint32_t);
    hipError_t e = ADC_HIP(hipStreamSynchronize(h->stream));
    if (e == hipSuccess) e = to_host ? ADC_HIP(hipMemcpy(tsdf, h->tsdf_vol, bytes, hipMemcpyDeviceToHost)) : ADC_HIP(hipMemcpy(h->tsdf_vol, tsdf, bytes, hipMemcpyHostToDevice));
    if (e == hipSuccess && color) e = to_host ? ADC_HIP(hipMemcpy(color, h->tsdf_col, bytes, hipMemcpyDeviceToHost)) : ADC_HIP(hipMemcpy(h->tsdf_col, color, bytes, hipMemcpyHostToDevice));
    if (e != hipSuccess) { set_error(who, e); (void)hipGetLastError(); return 2; }
    return 0;
}

int adc_tsdf_download(adc_handle* h, uint32_t* tsdf, uint32_t* color) { return tsdf_transfer(h, tsdf, color, true, "adc_tsdf_download"); }
int adc_tsdf_upload(adc_handle* h, const uint32_t* tsdf, const uint32_t* color)
{
    return tsdf_transfer(h, const_cast<uint32_t*>(tsdf), const_cast<uint32_t*>(color), false, "adc_tsdf_upload");
}

// ------------------------------------------------------------------------------ stereo-aware fusion (k_tsdf_fuse.hip)
// In the style of the integrate: the device forms enqueue on the object stream and are completed by adc_wait, which moves the report
// counts from pin_flags[ADC_PIN_TSDF_FUSE..] / pin_flags[ADC_PIN_TSDF_WEIGHT..] into tsdf_freport / tsdf_wreport.  The weights need no
// volume: their four report words are an allocation of their own (tsdfw_rep, first call).  Every refusal stands in front of the first
// HIP call.
static int tsdf_weights_check(adc_handle* h, const void* map, const void* conf, const adc_tsdf_frame* frame, const adc_tsdf_weight_params* params, const void* weight,
                              bool device, adc_tsdf_weight_params* p, const char* who)
{
    const char* why = nullptr;
    *p = params ? *params : TSDF_WEIGHT_DEFAULT;
    if (!h) why = "null handle";
    else if (!map) why = "null map";
    else if (!weight) why = "null weight";
    else if (!frame) why = "null frame";
    else if ((why = tsdf_frame_refusal(*frame)) != nullptr) {}
    else if ((why = tsdf_weight_params_refusal(*p)) != nullptr) {}
    else if (device && ((uintptr_t)map & 3u)) why = "d_map must be 4-byte aligned";
    else if (device && ((uintptr_t)conf & 3u)) why = "d_confidence must be 4-byte aligned";
    else if (match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    return 0;
}

static hipError_t enqueue_tsdf_weights(adc_handle* h, const AdcTsdfWeightReq& r)
{
    HIP_TRY(MEM_ONCE(h->tsdfw_rep, 8 * sizeof(uint32_t)));
    HIP_OK(hipMemsetAsync(h->tsdfw_rep, 0, ADC_TSDF_WEIGHT_WORDS * sizeof(uint32_t), h->stream));
    HIP_OK(adc_launch_tsdf_weights(h, r));
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_TSDF_WEIGHT, h->tsdfw_rep, ADC_TSDF_WEIGHT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

int adc_tsdf_weights_device(adc_handle* h, const void* d_map, const void* d_provenance, const void* d_confidence, const adc_tsdf_frame* frame,
                            const adc_tsdf_weight_params* params, void* d_weight)
{
    const char* who = "adc_tsdf_weights_device";
    AdcTsdfWeightReq r;
    if (tsdf_weights_check(h, d_map, d_confidence, frame, params, d_weight, true, &r.params, who) != 0) return 1;
    hipSetDevice(h->device);
    r.frame = *frame;
    r.map = static_cast<const float*>(d_map);
    r.prov = static_cast<const uint8_t*>(d_provenance);
    r.conf = static_cast<const float*>(d_confidence);
    r.weight = static_cast<uint8_t*>(d_weight);
    if (enqueue_tsdf_weights(h, r) != hipSuccess) return fail_call(h, who);
    h->fly.tsdfw_pending = 1;
    return 0;
}

int adc_tsdf_weights(adc_handle* h, const float* map, const uint8_t* provenance, const float* confidence, const adc_tsdf_frame* frame,
                     const adc_tsdf_weight_params* params, uint8_t* weight, adc_tsdf_weight_report* report)
{
    const char* who = "adc_tsdf_weights";
    adc_tsdf_weight_params p;
    if (tsdf_weights_check(h, map, confidence, frame, params, weight, false, &p, who) != 0) return 1;
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H;
    hipError_t e = MEM_ONCE(h->tsdfs_map, P * 4);
    if (e == hipSuccess) e = MEM_ONCE(h->tsdfs_wgt, P);
    if (e == hipSuccess && provenance) e = MEM_ONCE(h->tsdfs_prov, P);
    if (e == hipSuccess && confidence) e = MEM_ONCE(h->tsdfs_conf, P * 4);
    if (e != hipSuccess) return scratch_failed(who);
    if ((e = ADC_HIP(hipMemcpy(h->tsdfs_map, map, P * 4, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_tsdf_weights: upload", e); (void)hipGetLastError(); return 2; }
    if (provenance && (e = ADC_HIP(hipMemcpy(h->tsdfs_prov, provenance, P, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_tsdf_weights: provenance upload", e); (void)hipGetLastError(); return 2; }
    if (confidence && (e = ADC_HIP(hipMemcpy(h->tsdfs_conf, confidence, P * 4, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_tsdf_weights: confidence upload", e); (void)hipGetLastError(); return 2; }
    int rc = adc_tsdf_weights_device(h, h->tsdfs_map, provenance ? h->tsdfs_prov : nullptr, confidence ? h->tsdfs_conf : nullptr, frame, &p, h->tsdfs_wgt);
    if (rc == 0) rc = adc_wait(h);
    if (rc != 0) return rc;
    if ((e = ADC_HIP(hipMemcpy(weight, h->tsdfs_wgt, P, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_tsdf_weights: copy-out", e); (void)hipGetLastError(); return 2; }
    if (report) *report = h->tsdf_wreport;
    return 0;
}

static int tsdf_fuse_check(adc_handle* h, const void* map, const void* img, const adc_tsdf_frame* frame, const adc_tsdf_fuse_params* params, bool device,
                           adc_tsdf_fuse_params* p, const char* who)
{
    *p = params ? *params : TSDF_FUSE_DEFAULT;
    const char* why = tsdf_fuse_params_refusal(*p);
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    return tsdf_integrate_check(h, map, img, frame, device, who);
}

static hipError_t enqueue_tsdf_fuse(adc_handle* h, const AdcTsdfFuseReq& r)
{
    HIP_OK(hipMemsetAsync(h->tsdf_rep + ADC_TSDF_REP_FUSE, 0, ADC_TSDF_FUSE_WORDS * sizeof(uint32_t), h->stream));
    HIP_OK(adc_launch_tsdf_fuse(h, r));
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_TSDF_FUSE, h->tsdf_rep + ADC_TSDF_REP_FUSE, ADC_TSDF_FUSE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

int adc_tsdf_fuse_device(adc_handle* h, const void* d_map, const void* d_bgr_left, const void* d_weight, const adc_tsdf_frame* frame,
                         const adc_tsdf_fuse_params* params)
{
    const char* who = "adc_tsdf_fuse_device";
    AdcTsdfFuseReq r;
    if (tsdf_fuse_check(h, d_map, d_bgr_left, frame, params, true, &r.params, who) != 0) return 1;
    hipSetDevice(h->device);
    r.frame = *frame;
    r.map = static_cast<const float*>(d_map);
    r.img = static_cast<const uint8_t*>(d_bgr_left);
    r.weight = static_cast<const uint8_t*>(d_weight);
    if (enqueue_tsdf_fuse(h, r) != hipSuccess) return fail_call(h, who);
    h->fly.tsdff_pending = 1;
    return 0;
}

int adc_tsdf_fuse(adc_handle* h, const float* map, const uint8_t* bgr_left, const uint8_t* weight, const adc_tsdf_frame* frame,
                  const adc_tsdf_fuse_params* params, adc_tsdf_fuse_report* report)
{
    const char* who = "adc_tsdf_fuse";
    adc_tsdf_fuse_params p;
    if (tsdf_fuse_check(h, map, bgr_left, frame, params, false, &p, who) != 0) return 1;
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H;
    hipError_t e = MEM_ONCE(h->tsdfs_map, P * 4);
    if (e == hipSuccess && bgr_left) e = MEM_ONCE(h->tsdfs_img, P * 3);
    if (e == hipSuccess && weight) e = MEM_ONCE(h->tsdfs_wgt, P);
    if (e != hipSuccess) return scratch_failed(who);
    if ((e = ADC_HIP(hipMemcpy(h->tsdfs_map, map, P * 4, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_tsdf_fuse: upload", e); (void)hipGetLastError(); return 2; }
    if (bgr_left && (e = ADC_HIP(hipMemcpy(h->tsdfs_img, bgr_left, P * 3, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_tsdf_fuse: image upload", e); (void)hipGetLastError(); return 2; }
    if (weight && (e = ADC_HIP(hipMemcpy(h->tsdfs_wgt, weight, P, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_tsdf_fuse: weight upload", e); (void)hipGetLastError(); return 2; }
    int rc = adc_tsdf_fuse_device(h, h->tsdfs_map, bgr_left ? h->tsdfs_img : nullptr, weight ? h->tsdfs_wgt : nullptr, frame, &p);
    if (rc == 0) rc = adc_wait(h);
    if (rc != 0) return rc;
    if (report) *report = h->tsdf_freport;
    return 0;
}

int adc_get_tsdf_fuse_report(adc_handle* h, adc_tsdf_fuse_report* fuse_report, adc_tsdf_weight_report* weight_report)
{
    if (!h || (!fuse_report && !weight_report)) { g_last_error = "adc_get_tsdf_fuse_report: null argument"; return 1; }
    if (fuse_report && !h->tsdf_freport_valid) { g_last_error = "adc_get_tsdf_fuse_report: no fuse call has completed on this handle"; return 1; }
    if (weight_report && !h->tsdf_wreport_valid) { g_last_error = "adc_get_tsdf_fuse_report: no weights call has completed on this handle"; return 1; }
    if (fuse_report) *fuse_report = h->tsdf_freport;
    if (weight_report) *weight_report = h->tsdf_wreport;
    return 0;
}

// ------------------------------------------------------------------------------ moving volume (k_tsdf_shift.hip)
// In the style of the extraction: the device form enqueues on the object stream and is completed by adc_wait, which moves the four
// report words from pin_flags[ADC_PIN_TSDF_SHIFT..] into tsdf_sreport.  The shift works out of place into tsdf_vol2 / tsdf_col2; the
// HOST swaps the plane pointers, the offset and the origin only after every call of the sequence has been enqueued, so a HIP failure
// (fail_call drains the stream) leaves the volume, its origin and its offset as they were.  Every refusal stands in front of the
// first HIP call.
static int tsdf_shift_check(adc_handle* h, const adc_tsdf_shift_params* params, const void* points, uint64_t capacity, const void* count, bool device,
                            int32_t offset[3], const char* who)
{
    const char* why = nullptr;
    if (!h) why = "null handle";
    else if (!params) why = "null params";
    else if ((why = tsdf_shift_params_refusal(*params)) != nullptr) {}
    else if (!points && capacity != 0) why = "null points with a capacity";
    else if (device && ((uintptr_t)points & 15u)) why = "d_points must be 16-byte aligned";
    else if (device && ((uintptr_t)count & 3u)) why = "d_count must be 4-byte aligned";
    else if (!h->tsdf_set) why = "no volume (adc_tsdf_create first)";
    else if ((why = tsdf_shift_offset_refusal(h->tsdf_offset, params->shift, offset)) != nullptr) {}
    else if (match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    return 0;
}

// apply == false: the leaving list and its count only (the counting pass of the host form); the volume stays
static hipError_t enqueue_tsdf_shift(adc_handle* h, const AdcTsdfShiftReq& r, bool apply)
{
    const adc_tsdf_params& p = h->tsdf_params;
    const bool zero = tsdf_shift_is_zero(r.shift), all = tsdf_shift_all_leave(tsdf_shift_rule(p, r.shift));
    HIP_TRY(MEM_ONCE(h->tsdf_shift_rep, 8 * sizeof(uint32_t)));
    HIP_OK(hipMemsetAsync(h->tsdf_shift_rep, 0, 8 * sizeof(uint32_t), h->stream));
    if (zero) {
        if (r.count) HIP_OK(hipMemsetAsync(r.count, 0, sizeof(uint32_t), h->stream));
    } else {
        if (apply) {
            HIP_TRY(MEM_ONCE(h->tsdf_vol2, tsdf_voxels(p) * sizeof(uint32_t)));
            if (h->tsdf_col) HIP_TRY(MEM_ONCE(h->tsdf_col2, tsdf_voxels(p) * sizeof(uint32_t)));
        }
        HIP_TRY(MEM_GROW(h->tsdf_tiles, h->tsdf_tiles_cap, adc_tsdf_tile_count(&p), sizeof(uint32_t)));
        HIP_OK(adc_launch_tsdf_leave_measure(h, r));
        HIP_OK(adc_launch_tsdf_scan_on(h, h->tsdf_tiles, (int)adc_tsdf_tile_count(&p), h->tsdf_shift_rep + 2, r.count));
        if (r.points && r.capacity) HIP_OK(adc_launch_tsdf_leave_emit(h, r));
        if (apply && all) { // everything leaves: the new planes are empty, the kernel only counts
            HIP_OK(hipMemsetAsync(h->tsdf_vol2, 0, tsdf_voxels(p) * sizeof(uint32_t), h->stream));
            if (h->tsdf_col) HIP_OK(hipMemsetAsync(h->tsdf_col2, 0, tsdf_voxels(p) * sizeof(uint32_t), h->stream));
        }
        if (apply) HIP_OK(adc_launch_tsdf_shift(h, r, !all));
    }
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_TSDF_SHIFT, h->tsdf_shift_rep, ADC_TSDF_SHIFT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

static int tsdf_shift_call(adc_handle* h, const adc_tsdf_shift_params* params, void* d_points, uint64_t capacity, void* d_count, const int32_t offset[3], bool apply,
                           const char* who)
{
    AdcTsdfShiftReq r;
    for (int a = 0; a < 3; a++) r.shift[a] = params->shift[a];
    r.min_weight = params->min_weight;
    r.points = d_points;
    r.capacity = msh_cap32(capacity);
    r.count = static_cast<uint32_t*>(d_count);
    if (enqueue_tsdf_shift(h, r, apply) != hipSuccess) return fail_call(h, who);
    if (apply && !tsdf_shift_is_zero(r.shift)) {
        // everything is enqueued: the planes swap roles, the origin follows the total offset
        std::swap(h->tsdf_vol, h->tsdf_vol2);
        if (h->tsdf_col) std::swap(h->tsdf_col, h->tsdf_col2);
        for (int a = 0; a < 3; a++) {
            h->tsdf_offset[a] = offset[a];
            h->tsdf_params.origin[a] = tsdf_shift_origin(h->tsdf_origin0[a], offset[a], h->tsdf_params.voxel);
        }
    }
    h->fly.tsdfh_pending = 1;
    return 0;
}

int adc_tsdf_shift_device(adc_handle* h, const adc_tsdf_shift_params* params, void* d_points, uint64_t capacity, void* d_count)
{
    const char* who = "adc_tsdf_shift_device";
    int32_t offset[3];
    if (tsdf_shift_check(h, params, d_points, capacity, d_count, true, offset, who) != 0) return 1;
    hipSetDevice(h->device);
    return tsdf_shift_call(h, params, d_points, capacity, d_count, offset, true, who);
}

int adc_tsdf_shift(adc_handle* h, const adc_tsdf_shift_params* params, adc_point* points, uint64_t capacity, adc_tsdf_shift_report* report)
{
    const char* who = "adc_tsdf_shift";
    int32_t offset[3];
    if (tsdf_shift_check(h, params, points, capacity, nullptr, false, offset, who) != 0) return 1;
    hipSetDevice(h->device);
    // as adc_tsdf_extract: no more records than the volume can give, and a scratch that would have to grow is sized by a counting pass.
    // The list is made and copied out BEFORE the volume moves (a list-only pass): whatever fails, the caller either has the shifted
    // volume and its leaving points, or the volume as it was.
    const size_t most = 3 * tsdf_voxels(h->tsdf_params);
    size_t cap = capacity < most ? (size_t)capacity : most;
    hipError_t e = hipSuccess;
    int rc = 0;
    if (points && cap > h->tsdfs_pts_cap) {
        rc = tsdf_shift_call(h, params, nullptr, 0, nullptr, offset, false, who);
        if (rc == 0) rc = adc_wait(h);
        if (rc != 0) return rc;
        if (h->tsdf_sreport.points < cap) cap = h->tsdf_sreport.points;
    }
    if (points && cap) {
        if ((e = MEM_GROW(h->tsdfs_pts, h->tsdfs_pts_cap, cap, sizeof(adc_point))) != hipSuccess) return scratch_failed(who);
        rc = tsdf_shift_call(h, params, h->tsdfs_pts, cap, nullptr, offset, false, who);
        if (rc == 0) rc = adc_wait(h);
        if (rc != 0) return rc;
        const size_t n = h->tsdf_sreport.points < cap ? h->tsdf_sreport.points : cap;
        if (n && (e = ADC_HIP(hipMemcpy(points, h->tsdfs_pts, n * sizeof(adc_point), hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_tsdf_shift: copy-out", e); (void)hipGetLastError(); return 2; }
    }
    const adc_tsdf_params before = h->tsdf_params;
    const int32_t offset_before[3] = {h->tsdf_offset[0], h->tsdf_offset[1], h->tsdf_offset[2]};
    rc = tsdf_shift_call(h, params, nullptr, 0, nullptr, offset, true, who);
    if (rc != 0) return rc;
    if ((rc = adc_wait(h)) != 0) {
        // the wait failed behind a shift that was enqueued (the failure epilogue has drained the stream): the old planes were only
        // read, so the planes swap back and the volume, its origin and its offset are what they were
        if (!tsdf_shift_is_zero(params->shift)) {
            std::swap(h->tsdf_vol, h->tsdf_vol2);
            if (h->tsdf_col) std::swap(h->tsdf_col, h->tsdf_col2);
            h->tsdf_params = before;
            for (int a = 0; a < 3; a++) h->tsdf_offset[a] = offset_before[a];
        }
        return rc;
    }
    if (report) *report = h->tsdf_sreport;
    return 0;
}

int adc_get_tsdf_shift_report(adc_handle* h, adc_tsdf_shift_report* out)
{
    if (!h || !out) { g_last_error = "adc_get_tsdf_shift_report: null argument"; return 1; }
    if (!h->tsdf_sreport_valid) { g_last_error = "adc_get_tsdf_shift_report: no shift call has completed on this handle"; return 1; }
    *out = h->tsdf_sreport;
    return 0;
}

int adc_tsdf_get_offset(adc_handle* h, int32_t offset[3], float origin0[3])
{
    const char* why = !h || (!offset && !origin0) ? "null argument" : !h->tsdf_set ? "no volume (adc_tsdf_create first)" : nullptr;
    if (why) { g_last_error = std::string("adc_tsdf_get_offset: ") + why; return 1; }
    for (int a = 0; a < 3; a++) {
        if (offset) offset[a] = h->tsdf_offset[a];
        if (origin0) origin0[a] = h->tsdf_origin0[a];
    }
    return 0;
}

int adc_tsdf_follow_plan(const adc_tsdf_params* params, const float R[9], const float t[3], const adc_tsdf_follow_params* follow_params, int32_t shift_out[3])
{
    const char* who = "adc_tsdf_follow_plan";
    const char* why = nullptr;
    if (!params || !R || !t || !follow_params || !shift_out) why = "null argument";
    else if ((why = tsdf_params_refusal(*params)) != nullptr) {}
    else if ((why = tsdf_follow_params_refusal(*follow_params)) != nullptr) {}
    else {
        for (int i = 0; i < 9 && !why; i++)
            if (!__builtin_isfinite(R[i])) why = "R has a non-finite entry";
        for (int i = 0; i < 3 && !why; i++)
            if (!__builtin_isfinite(t[i])) why = "t has a non-finite entry";
    }
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    tsdf_follow_plan(*params, R, t, *follow_params, shift_out);
    return 0;
}

// ------------------------------------------------------------------------------ triangle mesh of the TSDF volume (k_tsdf.hip)
// In the style of the extraction: the device form enqueues on the object stream and is completed by adc_wait, which moves the five
// report counts from pin_flags[ADC_PIN_TSDF_MESH..] into tsdf_mreport.  Both counts are always taken; the vertex pass runs when vertex
// records or triangles are written (the triangles need every voxel's first rank), the triangle pass when triangles are written.
static int tsdf_mesh_check(adc_handle* h, const adc_tsdf_extract_params* params, const void* vertices, uint64_t vertex_capacity, const void* triangles,
                           uint64_t triangle_capacity, const void* counts, bool device, adc_tsdf_extract_params* p, const char* who)
{
    const char* why = nullptr;
    *p = params ? *params : TSDF_EXTRACT_DEFAULT;
    if (!h) why = "null handle";
    else if (p->min_weight < 1u || p->min_weight > 65535u) why = "min_weight must lie in [1, 65535]";
    else if (p->reserved_[0] | p->reserved_[1] | p->reserved_[2] | p->reserved_[3] | p->reserved_[4] | p->reserved_[5] | p->reserved_[6]) why = "a reserved word is not 0";
    else if (!vertices && !triangles) why = "neither vertices nor triangles requested";
    else if (!vertices && vertex_capacity != 0) why = "null vertices with a capacity";
    else if (!triangles && triangle_capacity != 0) why = "null triangles with a capacity";
    else if (device && ((uintptr_t)vertices & 15u)) why = "d_vertices must be 16-byte aligned";
    else if (device && ((uintptr_t)triangles & 3u)) why = "d_triangles must be 4-byte aligned";
    else if (device && ((uintptr_t)counts & 3u)) why = "d_counts must be 4-byte aligned";
    else if ((why = tsdf_state_refusal(h)) != nullptr) {}
    else if ((why = tsdf_mesh_refusal(h->tsdf_params)) != nullptr) {}
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    return 0;
}

// what adc_tsdf_mesh passes for a list that is requested with a capacity of 0 (counted, never written: no kernel receives it)
alignas(16) static unsigned char tsdf_count_only[16];

static hipError_t enqueue_tsdf_mesh(adc_handle* h, const AdcTsdfMeshReq& r)
{
    const bool tris = r.triangles && r.triangle_capacity, verts = r.vertices && r.vertex_capacity;
    HIP_TRY(MEM_GROW(h->tsdf_tiles, h->tsdf_tiles_cap, 2 * adc_tsdf_tile_count(&h->tsdf_params), sizeof(uint32_t)));
    if (tris) HIP_TRY(MEM_GROW(h->tsdf_first, h->tsdf_first_cap, tsdf_voxels(h->tsdf_params), sizeof(uint32_t)));
    HIP_OK(hipMemsetAsync(h->tsdf_rep + ADC_TSDF_REP_MESH, 0, ADC_TSDF_MESH_WORDS * sizeof(uint32_t), h->stream));
    HIP_OK(adc_launch_tsdf_mesh_measure(h, r));
    HIP_OK(adc_launch_tsdf_mesh_scan(h, r, 0));
    HIP_OK(adc_launch_tsdf_mesh_scan(h, r, 1));
    if (tris || verts) HIP_OK(adc_launch_tsdf_mesh_vertices(h, r, tris));
    if (tris) HIP_OK(adc_launch_tsdf_mesh_triangles(h, r));
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_TSDF_MESH, h->tsdf_rep + ADC_TSDF_REP_MESH, ADC_TSDF_MESH_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

int adc_tsdf_mesh_device(adc_handle* h, const adc_tsdf_extract_params* params, void* d_vertices, uint64_t vertex_capacity, void* d_triangles,
                         uint64_t triangle_capacity, void* d_counts)
{
    const char* who = "adc_tsdf_mesh_device";
    adc_tsdf_extract_params p;
    if (tsdf_mesh_check(h, params, d_vertices, vertex_capacity, d_triangles, triangle_capacity, d_counts, true, &p, who) != 0) return 1;
    hipSetDevice(h->device);
    AdcTsdfMeshReq r;
    r.min_weight = p.min_weight;
    r.vertices = d_vertices;
    r.vertex_capacity = msh_cap32(vertex_capacity);
    r.triangles = d_triangles;
    r.triangle_capacity = msh_cap32(triangle_capacity);
    r.counts = static_cast<uint32_t*>(d_counts);
    if (enqueue_tsdf_mesh(h, r) != hipSuccess) return fail_call(h, who);
    h->fly.tsdfm_pending = 1;
    return 0;
}

int adc_tsdf_mesh(adc_handle* h, const adc_tsdf_extract_params* params, adc_point* vertices, uint64_t vertex_capacity, uint32_t* triangles,
                  uint64_t triangle_capacity, adc_tsdf_mesh_report* report)
{
    const char* who = "adc_tsdf_mesh";
    adc_tsdf_extract_params p;
    if (tsdf_mesh_check(h, params, vertices, vertex_capacity, triangles, triangle_capacity, nullptr, false, &p, who) != 0) return 1;
    hipSetDevice(h->device);
    // no more records than the volume can give: three crossings per voxel, M triangles per cell (below 2^32 by the count limit)
    const adc_tsdf_params& tp = h->tsdf_params;
    const size_t most_v = 3 * tsdf_voxels(tp), most_t = (size_t)TSDF_MC_MAX_TRIS * (size_t)(tp.nx - 1) * (size_t)(tp.ny - 1) * (size_t)(tp.nz - 1);
    size_t vcap = vertex_capacity < most_v ? (size_t)vertex_capacity : most_v, tcap = triangle_capacity < most_t ? (size_t)triangle_capacity : most_t;
    hipError_t e = hipSuccess;
    int rc = 0;
    if ((vertices && vcap > h->tsdfs_pts_cap) || (triangles && tcap > h->tsdfs_tri_cap)) {
        // a scratch would have to grow: count first, so that neither ever holds more records than the volume has (adc_tsdf_extract)
        rc = adc_tsdf_mesh_device(h, &p, vertices ? tsdf_count_only : nullptr, 0, triangles ? tsdf_count_only : nullptr, 0, nullptr);
        if (rc == 0) rc = adc_wait(h);
        if (rc != 0) return rc;
        if (h->tsdf_mreport.vertices < vcap) vcap = h->tsdf_mreport.vertices;
        if (h->tsdf_mreport.triangles < tcap) tcap = h->tsdf_mreport.triangles;
        if ((!vertices || vcap == 0) && (!triangles || tcap == 0)) { // (nothing to write: the counting pass was the call)
            if (report) *report = h->tsdf_mreport;
            return 0;
        }
    }
    if (vertices && vcap && (e = MEM_GROW(h->tsdfs_pts, h->tsdfs_pts_cap, vcap, sizeof(adc_point))) != hipSuccess) return scratch_failed(who);
    if (triangles && tcap && (e = MEM_GROW(h->tsdfs_tri, h->tsdfs_tri_cap, tcap, 3 * sizeof(uint32_t))) != hipSuccess) return scratch_failed(who);
    rc = adc_tsdf_mesh_device(h, &p, !vertices ? nullptr : vcap ? (void*)h->tsdfs_pts : (void*)tsdf_count_only, vertices ? vcap : 0,
                              !triangles ? nullptr : tcap ? (void*)h->tsdfs_tri : (void*)tsdf_count_only, triangles ? tcap : 0, nullptr);
    if (rc == 0) rc = adc_wait(h);
    if (rc != 0) return rc;
    const size_t nv = h->tsdf_mreport.vertices < vcap ? h->tsdf_mreport.vertices : vcap, nt = h->tsdf_mreport.triangles < tcap ? h->tsdf_mreport.triangles : tcap;
    if (vertices && nv && (e = ADC_HIP(hipMemcpy(vertices, h->tsdfs_pts, nv * sizeof(adc_point), hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_tsdf_mesh: vertex copy-out", e); return 2; }
    if (triangles && nt && (e = ADC_HIP(hipMemcpy(triangles, h->tsdfs_tri, nt * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_tsdf_mesh: triangle copy-out", e); return 2; }
    if (report) *report = h->tsdf_mreport;
    return 0;
}

int adc_get_tsdf_mesh_report(adc_handle* h, adc_tsdf_mesh_report* out)
{
    if (!h || !out) { g_last_error = "adc_get_tsdf_mesh_report: null argument"; return 1; }
    if (!h->tsdf_mreport_valid) { g_last_error = "adc_get_tsdf_mesh_report: no mesh call has completed on this handle"; return 1; }
    *out = h->tsdf_mreport;
    return 0;
}

// ------------------------------------------------------------------------------ ray cast of the TSDF volume (k_tsdf_raycast.hip)
// In the style of adc_tsdf_extract_device: enqueued on the object stream and completed by adc_wait, which moves the report words from
// pin_flags[ADC_PIN_TSDF_RAY..] into tsdf_rreport.  The volume is only read.  Every refusal stands in front of the first HIP call.
static int tsdf_raycast_check(adc_handle* h, const adc_tsdf_raycast_params* params, const void* depth, const void* normals, const void* bgr, const void* status,
                              bool device, const char* who)
{
    const char* why = nullptr;
    if (!h) why = "null handle";
    else if (!params) why = "null params";
    else if ((why = tsdf_raycast_refusal(*params)) != nullptr) {}
    else if (!depth && !normals && !bgr && !status) why = "no output requested";
    else if (device && ((uintptr_t)depth & 3u)) why = "d_depth must be 4-byte aligned";
    else if (device && ((uintptr_t)normals & 15u)) why = "d_normals must be 16-byte aligned";
    else if (!h->tsdf_set) why = "no volume (adc_tsdf_create first)";
    else if (bgr && !(h->tsdf_params.flags & ADC_TSDF_COLOR)) why = "bgr needs a colour volume (ADC_TSDF_COLOR)";
    else if (match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    return 0;
}

static hipError_t enqueue_tsdf_raycast(adc_handle* h, const AdcTsdfRayReq& r)
{
    HIP_OK(hipMemsetAsync(h->tsdf_rep + ADC_TSDF_REP_RAY, 0, ADC_TSDF_RAY_WORDS * sizeof(uint32_t), h->stream));
    HIP_OK(adc_launch_tsdf_raycast(h, r));
    HIP_OK(hipMemcpyAsync(h->pin_flags + ADC_PIN_TSDF_RAY, h->tsdf_rep + ADC_TSDF_REP_RAY, ADC_TSDF_RAY_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

int adc_tsdf_raycast_device(adc_handle* h, const adc_tsdf_raycast_params* params, void* d_depth, void* d_normals, void* d_bgr, void* d_status)
{
    const char* who = "adc_tsdf_raycast_device";
    if (tsdf_raycast_check(h, params, d_depth, d_normals, d_bgr, d_status, true, who) != 0) return 1;
    hipSetDevice(h->device);
    AdcTsdfRayReq r;
    r.view = *params;
    r.depth = static_cast<float*>(d_depth);
    r.normals = static_cast<float*>(d_normals);
    r.bgr = static_cast<uint8_t*>(d_bgr);
    r.status = static_cast<uint8_t*>(d_status);
    if (enqueue_tsdf_raycast(h, r) != hipSuccess) return fail_call(h, who);
    h->fly.tsdfr_pending = 1;
    return 0;
}

int adc_tsdf_raycast(adc_handle* h, const adc_tsdf_raycast_params* params, float* depth, float* normals, uint8_t* bgr, uint8_t* status,
                     adc_tsdf_raycast_report* report)
{
    const char* who = "adc_tsdf_raycast";
    if (tsdf_raycast_check(h, params, depth, normals, bgr, status, false, who) != 0) return 1;
    hipSetDevice(h->device);
    // the scratch: four planes behind one another, the normals first (16-byte aligned), then depth, bgr, status
    const size_t P = (size_t)params->width * (size_t)params->height;
    hipError_t e = MEM_GROW(h->tsdfs_ray, h->tsdfs_ray_cap, P, 24);
    if (e != hipSuccess) return scratch_failed(who);
    uint8_t* d_n = h->tsdfs_ray;
    uint8_t* d_d = d_n + 16 * P;
    uint8_t* d_c = d_d + 4 * P;
    uint8_t* d_s = d_c + 3 * P;
    int rc = adc_tsdf_raycast_device(h, params, depth ? d_d : nullptr, normals ? d_n : nullptr, bgr ? d_c : nullptr, status ? d_s : nullptr);
    if (rc == 0) rc = adc_wait(h);
    if (rc != 0) return rc;
    if (depth && (e = ADC_HIP(hipMemcpy(depth, d_d, 4 * P, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_tsdf_raycast: depth copy-out", e); return 2; }
    if (normals && (e = ADC_HIP(hipMemcpy(normals, d_n, 16 * P, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_tsdf_raycast: normals copy-out", e); return 2; }
    if (bgr && (e = ADC_HIP(hipMemcpy(bgr, d_c, 3 * P, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_tsdf_raycast: bgr copy-out", e); return 2; }
    if (status && (e = ADC_HIP(hipMemcpy(status, d_s, P, hipMemcpyDeviceToHost))) != hipSuccess) { set_error("adc_tsdf_raycast: status copy-out", e); return 2; }
    if (report) *report = h->tsdf_rreport;
    return 0;
}

int adc_get_tsdf_raycast_report(adc_handle* h, adc_tsdf_raycast_report* out)
{
    if (!h || !out) { g_last_error = "adc_get_tsdf_raycast_report: null argument"; return 1; }
    if (!h->tsdf_rreport_valid) { g_last_error = "adc_get_tsdf_raycast_report: no ray cast has completed on this handle"; return 1; }
    *out = h->tsdf_rreport;
    return 0;
}

// ------------------------------------------------------------------------------ frame-to-model tracking (k_tsdf_track.hip)
// In the style of adc_tsdf_raycast_device: enqueued on the object stream and completed by adc_wait, which moves the pinned record
// into track_result.  One clear of the state, `iterations` pairs of (reduce, solve) up front -- a pair behind a terminal status is a
// no-op on the device --, one read-back.  Every refusal stands in front of the first HIP call.
static int track_check(adc_handle* h, const void* map, const void* fnormals, const adc_tsdf_frame* frame, const adc_tsdf_raycast_params* model, const void* mdepth,
                       const void* mnormals, const adc_track_params* params, const void* result, bool device, bool needs_volume, adc_track_params* p, const char* who)
{
    const char* why = nullptr;
    *p = params ? *params : TRACK_DEFAULT;
    if (!h) why = "null handle";
    else if (!map) why = "null map";
    else if (!frame) why = "null frame";
    else if (device && !model) why = "null model view";
    else if (device && !mdepth) why = "null model depth";
    else if (device && !mnormals) why = "null model normals";
    else if ((why = tsdf_frame_refusal(*frame)) != nullptr) {}
    else if (device && (why = track_model_refusal(*model)) != nullptr) {}
    else if ((why = track_params_refusal(*p)) != nullptr) {}
    else if (device && ((uintptr_t)map & 3u)) why = "d_map must be 4-byte aligned";
    else if (device && ((uintptr_t)fnormals & 15u)) why = "d_frame_normals must be 16-byte aligned";
    else if (device && ((uintptr_t)mdepth & 3u)) why = "d_model_depth must be 4-byte aligned";
    else if (device && ((uintptr_t)mnormals & 15u)) why = "d_model_normals must be 16-byte aligned";
    else if (device && ((uintptr_t)result & 7u)) why = "d_result must be 8-byte aligned";
    else if (needs_volume && !h->tsdf_set) why = "no volume (adc_tsdf_create first)";
    else if (match_in_flight(h)) why = "a Match is pending (adc_wait first)";
    else if ((why = track_size_refusal(h->p.W, h->p.H, p->stride)) != nullptr) {}
    if (why) { g_last_error = std::string(who) + ": " + why; return 1; }
    return 0;
}

static hipError_t enqueue_track(adc_handle* h, const AdcTrackReq& r, void* d_result)
{
    HIP_OK(hipMemsetAsync(h->track_state, 0, sizeof(AdcTrackState), h->stream));
    for (uint32_t k = 0; k < r.params.iterations; k++) {
        HIP_OK(adc_launch_track_reduce(h, r, k));
        HIP_OK(adc_launch_track_solve(h, r, k));
    }
    if (d_result) HIP_OK(hipMemcpyAsync(d_result, &h->track_state->res, sizeof(adc_track_result), hipMemcpyDeviceToDevice, h->stream));
    HIP_OK(hipMemcpyAsync(h->track_pin, &h->track_state->res, sizeof(adc_track_result), hipMemcpyDeviceToHost, h->stream));
    return hipSuccess;
}

int adc_track_device(adc_handle* h, const void* d_map, const void* d_frame_normals, const adc_tsdf_frame* frame, const adc_tsdf_raycast_params* model_view,
                     const void* d_model_depth, const void* d_model_normals, const adc_track_params* params, void* d_result)
{
    const char* who = "adc_track_device";
    AdcTrackReq r;
    if (track_check(h, d_map, d_frame_normals, frame, model_view, d_model_depth, d_model_normals, params, d_result, true, false, &r.params, who) != 0) return 1;
    hipSetDevice(h->device);
    hipError_t e = MEM_ONCE(h->track_state, sizeof(AdcTrackState));
    if (e == hipSuccess) e = MEM_ONCE_PINNED(h->track_pin, sizeof(adc_track_result));
    if (e != hipSuccess) return scratch_failed(who);
    if (!h->track_cus) {
        int cus = 0;
        if ((e = ADC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device))) != hipSuccess) {
            set_error("adc_track_device: hipDeviceGetAttribute", e);
            (void)hipGetLastError();
            return 2;
        }
        h->track_cus = cus > 0 ? cus : 1;
    }
    r.frame = *frame;
    r.model = *model_view;
    r.map = static_cast<const float*>(d_map);
    r.fnormals = static_cast<const float*>(d_frame_normals);
    r.mdepth = static_cast<const float*>(d_model_depth);
    r.mnormals = static_cast<const float*>(d_model_normals);
    if (enqueue_track(h, r, d_result) != hipSuccess) return fail_call(h, who);
    h->fly.track_pending = 1;
    return 0;
}

int adc_tsdf_track(adc_handle* h, const float* map, const adc_tsdf_frame* frame, const adc_track_params* params, adc_track_result* result)
{
    const char* who = "adc_tsdf_track";
    adc_track_params p;
    if (track_check(h, map, nullptr, frame, nullptr, nullptr, nullptr, params, nullptr, false, true, &p, who) != 0) return 1;
    // the model: the volume as the frame's own camera sees it from the guess, as the CLI casts it
    adc_tsdf_raycast_params view;
    memset(&view, 0, sizeof(view));
    view.width = h->p.W; view.height = h->p.H;
    view.focal_px = frame->calib.focal_px; view.cx = frame->calib.cx; view.cy = frame->calib.cy;
    memcpy(view.R, frame->R, sizeof(view.R));
    memcpy(view.t, frame->t, sizeof(view.t));
    view.z_near = h->tsdf_params.voxel;
    view.z_far = 3.0e38f;
    view.step = h->tsdf_params.voxel * 0.5f;
    const float half = h->tsdf_params.trunc * 0.5f;
    view.skip = half > view.step ? half : view.step;
    view.min_weight = 1u;
    view.max_steps = TSDF_RAY_MAX_STEPS;
    const char* why = tsdf_raycast_refusal(view);
    if (why) { g_last_error = std::string(who) + ": the model view: " + why; return 1; }
    hipSetDevice(h->device);
    // the scratch: the model's normals first (16-byte aligned), then the map, then the model's depth
    const size_t P = (size_t)h->p.W * h->p.H;
    hipError_t e = MEM_ONCE(h->tracks_map, P * 24); // (a handle has one geometry: the first call's size is every call's)
    if (e != hipSuccess) return scratch_failed(who);
    float* d_n = h->tracks_map;
    float* d_map = d_n + 4 * P;
    float* d_d = d_map + P;
    if ((e = ADC_HIP(hipMemcpy(d_map, map, P * 4, hipMemcpyHostToDevice))) != hipSuccess) { set_error("adc_tsdf_track: upload", e); (void)hipGetLastError(); return 2; }
    int rc = adc_tsdf_raycast_device(h, &view, d_d, d_n, nullptr, nullptr);
    if (rc == 0) rc = adc_track_device(h, d_map, nullptr, frame, &view, d_d, d_n, &p, nullptr);
    if (rc == 0) rc = adc_wait(h);
    else if (h->stream) { hipStreamSynchronize(h->stream); (void)hipGetLastError(); h->fly.tsdfr_pending = 0; } // (a ray cast without its track: drained, not reported)
    if (rc != 0) return rc;
    if (result) *result = h->track_result;
    return 0;
}

int adc_get_track_result(adc_handle* h, adc_track_result* out)
{
    if (!h || !out) { g_last_error = "adc_get_track_result: null argument"; return 1; }
    if (!h->track_result_valid) { g_last_error = "adc_get_track_result: no track has completed on this handle"; return 1; }
    *out = h->track_result;
    return 0;
}

// ------------------------------------------------------------------------------ pair farm
struct adc_farm {
    std::vector<adc_handle*> pipes;
    std::vector<uint64_t> in_flight; // ticket of the pair in flight on each pipeline (0 = idle)
    uint64_t next_ticket = 1;
    int64_t delivered = 0;
};

adc_farm* adc_farm_create(int32_t width, int32_t height, const adc_option* opt, int device, int pipelines)
{
    if (pipelines < 1 || pipelines > 64) { g_last_error = "adc_farm_create: pipelines must be 1..64"; return nullptr; }
    adc_farm* f = new (std::nothrow) adc_farm();
    if (!f) return nullptr;
    for (int i = 0; i < pipelines; i++) {
        adc_handle* h = adc_create(width, height, opt, device);
        if (!h) { adc_farm_destroy(f); return nullptr; }
        f->pipes.push_back(h);
        f->in_flight.push_back(0);
    }
    return f;
}
void adc_farm_destroy(adc_farm* f)
{
    if (!f) return;
    for (size_t i = 0; i < f->pipes.size(); i++) {
        if (f->in_flight[i]) adc_wait(f->pipes[i]);
        adc_destroy(f->pipes[i]);
    }
    delete f;
}
static int farm_collect(adc_farm* f, size_t slot)
{
    if (!f->in_flight[slot]) return 0;
    const int rc = adc_wait(f->pipes[slot]);
    f->in_flight[slot] = 0;
    if (rc == 0) f->delivered++;
    return rc;
}
static int farm_submit_impl(adc_farm* f, const uint8_t* left, const uint8_t* right, float* disp, const adc_products* products, uint64_t* ticket)
{
    if (!f || !left || !right || !disp) return 1;
    if (products && products->out.cloud && !products->out.cloud_count) { // (there is no per-ticket getter: the count travels with the pair)
        g_last_error = "adc_farm_submit_products: a cloud needs cloud_count";
        return 1;
    }
    const uint64_t t = f->next_ticket;
    const size_t slot = (size_t)((t - 1) % f->pipes.size());
    // the pipeline's previous pair (if any) must be delivered before its staging is reused.  When THAT pair failed, the new
    // pair is still enqueued (the caller gets its ticket) and the failure is reported as ADC_FARM_PREVIOUS_FAILED with the
    // failed ticket in adc_last_error(): the caller can tell which output is invalid
    const uint64_t prev = f->in_flight[slot];
    const int rc_prev = farm_collect(f, slot);
    const std::string prev_error = rc_prev != 0 ? g_last_error : std::string();
    int rc = products ? adc_match_async_products(f->pipes[slot], left, right, disp, products) : adc_match_async(f->pipes[slot], left, right, disp);
    if (rc != 0) {
        // nothing was enqueued; when the pipeline's previous pair failed as well, say so first (its output is invalid too)
        if (rc_prev != 0)
            g_last_error = "adc_farm_submit: the pair with ticket " + std::to_string((unsigned long long)prev) + " failed (" + prev_error +
                           ") AND the new pair could not be enqueued (" + g_last_error + ")";
        return rc;
    }
    f->in_flight[slot] = t;
    f->next_ticket++;
    if (ticket) *ticket = t;
    if (rc_prev != 0) {
        g_last_error = "adc_farm_submit: the pair with ticket " + std::to_string((unsigned long long)prev) + " failed (" + prev_error + "); the new pair was enqueued";
        return ADC_FARM_PREVIOUS_FAILED;
    }
    return 0;
}
int adc_farm_submit(adc_farm* f, const uint8_t* left, const uint8_t* right, float* disp, uint64_t* ticket)
{
    return farm_submit_impl(f, left, right, disp, nullptr, ticket);
}
int adc_farm_submit_products(adc_farm* f, const uint8_t* left, const uint8_t* right, float* disp, const adc_products* products, uint64_t* ticket)
{
    return farm_submit_impl(f, left, right, disp, products, ticket);
}
int adc_farm_wait(adc_farm* f, uint64_t ticket)
{
    if (!f || ticket == 0 || ticket >= f->next_ticket) return 1;
    const size_t slot = (size_t)((ticket - 1) % f->pipes.size());
    if (f->in_flight[slot] && f->in_flight[slot] <= ticket) return farm_collect(f, slot);
    return 0; // already delivered (a later pair of the pipeline is in flight, or the pipeline is idle)
}
int64_t adc_farm_drain(adc_farm* f)
{
    if (!f) return -1;
    // oldest first
    for (size_t k = 0; k < f->pipes.size(); k++) {
        size_t best = f->pipes.size();
        for (size_t i = 0; i < f->pipes.size(); i++)
            if (f->in_flight[i] && (best == f->pipes.size() || f->in_flight[i] < f->in_flight[best])) best = i;
        if (best == f->pipes.size()) break;
        if (farm_collect(f, best) != 0) return -1;
    }
    return f->delivered;
}

int adc_farm_set_speckle_filter(adc_farm* f, int32_t max_size, float max_diff)
{
    if (!f) return 1;
    if (!speckle_args_ok(max_diff, "adc_farm_set_speckle_filter")) return 1;
    for (size_t i = 0; i < f->pipes.size(); i++)
        if (f->in_flight[i]) { g_last_error = "adc_farm_set_speckle_filter: a pair is in flight (adc_farm_drain first)"; return 1; }
    for (size_t i = 0; i < f->pipes.size(); i++) {
        const int rc = adc_set_speckle_filter(f->pipes[i], max_size, max_diff);
        if (rc != 0) return rc;
    }
    return 0;
}

static bool farm_idle(adc_farm* f, const char* who)
{
    for (size_t i = 0; i < f->pipes.size(); i++)
        if (f->in_flight[i]) { g_last_error = std::string(who) + ": a pair is in flight (adc_farm_drain first)"; return false; }
    return true;
}
int adc_farm_set_cloud_voxel_grid(adc_farm* f, const adc_voxel_grid* grid)
{
    if (!f) { g_last_error = "adc_farm_set_cloud_voxel_grid: null farm"; return 1; }
    if (grid && !voxel_grid_ok(grid, "adc_farm_set_cloud_voxel_grid")) return 1;
    if (!farm_idle(f, "adc_farm_set_cloud_voxel_grid")) return 1;
    for (size_t i = 0; i < f->pipes.size(); i++) {
        const int rc = grid ? adc_set_cloud_voxel_grid(f->pipes[i], grid) : adc_clear_cloud_voxel_grid(f->pipes[i]);
        if (rc != 0) return rc;
    }
    return 0;
}
int adc_farm_set_rectify_maps(adc_farm* f, int side, const adc_raw_format* raw, const float* map_x, const float* map_y)
{
    if (!f || !raw || !map_x || !map_y || !farm_idle(f, "adc_farm_set_rectify_maps")) return 1;
    for (size_t i = 0; i < f->pipes.size(); i++) {
        const int rc = adc_set_rectify_maps(f->pipes[i], side, raw, map_x, map_y);
        if (rc != 0) return rc;
    }
    return 0;
}
int adc_farm_set_rectify_model(adc_farm* f, int side, const adc_raw_format* raw, const adc_camera_model* model)
{
    if (!f || !raw || !model || !farm_idle(f, "adc_farm_set_rectify_model")) return 1;
    for (size_t i = 0; i < f->pipes.size(); i++) {
        const int rc = adc_set_rectify_model(f->pipes[i], side, raw, model);
        if (rc != 0) return rc;
    }
    return 0;
}
int adc_farm_set_input_format(adc_farm* f, int side, const adc_raw_format* raw)
{
    if (!f || !raw || !farm_idle(f, "adc_farm_set_input_format")) return 1;
    for (size_t i = 0; i < f->pipes.size(); i++) {
        const int rc = adc_set_input_format(f->pipes[i], side, raw);
        if (rc != 0) return rc;
    }
    return 0;
}

int adc_farm_clear_rectify(adc_farm* f)
{
    if (!f || !farm_idle(f, "adc_farm_clear_rectify")) return 1;
    for (size_t i = 0; i < f->pipes.size(); i++)
        if (adc_clear_rectify(f->pipes[i]) != 0) return 1;
    return 0;
}

// ------------------------------------------------------------------------------ misc plumbing
const char* adc_stage_name(int s)
{
    static const char* names[ADC_STAGE_COUNT] = {"cost", "arms", "aggregate", "scanline", "wta", "refine"};
    return (s >= 0 && s < ADC_STAGE_COUNT) ? names[s] : "";
}
int adc_set_paper_modes(adc_handle* h, uint32_t modes)
{
    if (!h) { g_last_error = "adc_set_paper_modes: null handle"; return 1; }
    if (modes & ~(ADC_PAPER_CENSUS5X5 | ADC_PAPER_SO_SUM | ADC_PAPER_RIGHT_ARMS)) {
        g_last_error = "adc_set_paper_modes: unknown mode bits " + std::to_string((unsigned)modes);
        return 1;
    }
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H;
    if ((modes & ADC_PAPER_RIGHT_ARMS) && !(h->arms_r && h->bgrx_r && h->armmax_r)) {
        // all three or none: a partial set left behind by a failed call must not pass for "allocated" in the next one
        if (MEM_ONCE(h->arms_r, P * 4) != hipSuccess || MEM_ONCE(h->bgrx_r, P * 4) != hipSuccess || MEM_ONCE(h->armmax_r, 4 * sizeof(int)) != hipSuccess) {
            dev_mem_release<HipMem>(&h->mem, &h->arms_r);
            dev_mem_release<HipMem>(&h->mem, &h->bgrx_r);
            dev_mem_release<HipMem>(&h->mem, &h->armmax_r);
            g_last_error = "adc_set_paper_modes: allocation failed: " + g_last_error;
            return 2;
        }
    }
    if ((modes & ADC_PAPER_SO_SUM) && MEM_ONCE(h->vol_c, P * h->p.Dp * sizeof(float)) != hipSuccess) { g_last_error = "adc_set_paper_modes: allocation failed: " + g_last_error; return 2; }
    h->paper = modes;
    return 0;
}
void adc_set_profiling(adc_handle* h, int on) { if (h) h->profiling = on; }
void adc_set_verbose(adc_handle* h, int on) { if (h) { h->verbose = on; if (on) h->profiling = 1; } }
int adc_get_stage_ms(adc_handle* h, float* ms, int n)
{
    if (!h || !ms) return 1;
    for (int i = 0; i < n && i < ADC_STAGE_COUNT; i++) ms[i] = h->stage_ms[i];
    return 0;
}
int adc_get_aggregate_pass_ms(adc_handle* h, float* avg_ms, int* launches)
{
    if (!h) return 1;
    if (avg_ms) *avg_ms = h->agg_pass_ms;
    if (launches) *launches = h->agg_launches - (h->agg_first_fused ? 1 : 0);
    return 0;
}
int adc_get_aggregate_info(adc_handle* h, float* avg_launch_ms, int* launches, int* passes, int* first_fused)
{
    if (!h) return 1;
    const int ff = h->agg_first_fused ? 1 : 0;
    if (avg_launch_ms) *avg_launch_ms = h->agg_pass_ms;
    if (launches) *launches = h->agg_launches - ff;
    if (passes) *passes = h->agg_passes - ff;
    if (first_fused) *first_fused = ff;
    return 0;
}
const char* adc_get_aggregate_kernel(adc_handle* h) { return (h && h->agg_kernel) ? h->agg_kernel : ""; }
void* adc_get_stream(adc_handle* h) { return h ? (void*)h->stream : nullptr; }
int adc_device_synchronize(void) { return hipDeviceSynchronize() == hipSuccess ? 0 : 1; }
void* adc_device_malloc(size_t bytes) { void* p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; }
void adc_device_free(void* p) { if (p) hipFree(p); }
double adc_device_copy_ms(void* dst, const void* src, size_t bytes, int reps)
{
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.0;
    double best = -1.0;
    for (int r = 0; r < (reps < 1 ? 1 : reps) + 1; r++) { // first copy = warm-up
        hipEventRecord(e0, 0);
        if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, 0) != hipSuccess) { best = -1.0; break; }
        hipEventRecord(e1, 0);
        if (hipEventSynchronize(e1) != hipSuccess) { best = -1.0; break; }
        float ms = 0.f;
        hipEventElapsedTime(&ms, e0, e1);
        if (r > 0 && (best < 0 || ms < best)) best = ms;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return best;
}
double adc_device_copy_kernel_ms(void* dst, const void* src, size_t bytes, int reps)
{
    hipEvent_t e0, e1;
    if ((bytes & 15) || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.0;
    double best = -1.0;
    const size_t n = bytes / 16;
    for (int variant = 0; variant < 6 && best > -2.0; variant++) {
        const unsigned grid = variant < 2 ? 8192u : (variant < 4 ? 32768u : 65536u);
        for (int r = 0; r < (reps < 1 ? 1 : reps) + 1; r++) { // first copy = warm-up
            hipEventRecord(e0, 0);
            if (variant & 1) hipLaunchKernelGGL((k_copy_yardstick<true>), dim3(grid), dim3(256), 0, 0, (const adc_vf4*)src, (adc_vf4*)dst, n);
            else hipLaunchKernelGGL((k_copy_yardstick<false>), dim3(grid), dim3(256), 0, 0, (const adc_vf4*)src, (adc_vf4*)dst, n);
            hipEventRecord(e1, 0);
            if (hipGetLastError() != hipSuccess || hipEventSynchronize(e1) != hipSuccess) { best = -3.0; break; }
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            if (r > 0 && (best < 0 || ms < best)) best = ms;
        }
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return best < 0 ? -1.0 : best;
}
int adc_memcpy_h2d(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : 1; }
int adc_memcpy_d2h(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1; }

// ------------------------------------------------------------------------------ debug surface
struct BufDesc { void* ptr; size_t bytes; bool volume; };
static BufDesc buf_desc(adc_handle* h, int which)
{
    const size_t P = (size_t)h->p.W * h->p.H;
    switch (which) {
    case ADC_BUF_GRAY_LEFT: return {h->gray_l, P, false};
    case ADC_BUF_GRAY_RIGHT: return {h->gray_r, P, false};
    case ADC_BUF_CENSUS_LEFT: return {h->census_l, P * 8, false};
    case ADC_BUF_CENSUS_RIGHT: return {h->census_r, P * 8, false};
    case ADC_BUF_ARMS: return {h->arms, P * 4, false};
    case ADC_BUF_SUPCOUNT_H: return {h->sup_h, P * 2, false};
    case ADC_BUF_SUPCOUNT_V: return {h->sup_v, P * 2, false};
    case ADC_BUF_VOLUME_A: return {h->vol_a, P * h->p.D * 4, true};
    case ADC_BUF_DISP_LEFT: return {h->disp_l, P * 4, false};
    case ADC_BUF_DISP_RIGHT: return {h->disp_r, P * 4, false};
    case ADC_BUF_OUTLIER_LABEL: return {h->label, P, false};
    default: return {nullptr, 0, false};
    }
}

int adc_debug_read(adc_handle* h, int which, void* dst)
{
    if (!h || !dst) return 1;
    hipSetDevice(h->device);
    const BufDesc b = buf_desc(h, which);
    if (!b.ptr) return 1;
    if (b.volume) { // de-pad through vol_b (scratch at stage boundaries)
        if (adc_launch_unpad_volume(h, h->vol_a, h->vol_b) != hipSuccess) return 2;
        if (hipMemcpyAsync(dst, h->vol_b, b.bytes, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return 2;
    } else if (hipMemcpyAsync(dst, b.ptr, b.bytes, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return 2;
    return hipStreamSynchronize(h->stream) == hipSuccess ? 0 : 2;
}

int adc_debug_write(adc_handle* h, int which, const void* src)
{
    if (!h || !src) return 1;
    hipSetDevice(h->device);
    const BufDesc b = buf_desc(h, which);
    if (!b.ptr) return 1;
    if (b.volume) {
        if (hipMemcpyAsync(h->vol_b, src, b.bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess) return 2;
        if (adc_launch_pad_volume(h, h->vol_b, h->vol_a) != hipSuccess) return 2;
    } else if (hipMemcpyAsync(b.ptr, src, b.bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess) return 2;
    return hipStreamSynchronize(h->stream) == hipSuccess ? 0 : 2;
}

int adc_debug_itp_code_geometry(adc_handle* h, int* pitch, int* rows, int* gx)
{
    if (!h || !pitch || !rows || !gx) return 1;
    if (h->itp_pitch == 0) { g_last_error = "adc_debug_itp_code_geometry: this handle has no code maps (itp_plan.h)"; return 1; }
    *pitch = h->itp_pitch;
    *rows = adc_itp_code_rows(h->p.H, h->itp_ms);
    *gx = h->itp_ms;
    return 0;
}

int adc_debug_read_itp_code(adc_handle* h, int pass, void* dst)
{
    int pitch, rows, gx;
    if (!dst || pass < 0 || pass > 1 || adc_debug_itp_code_geometry(h, &pitch, &rows, &gx) != 0) return 1;
    hipSetDevice(h->device);
    const uint8_t* code = h->itp_cells + adc_itp_code_offset(h->p.W, h->p.H) + (size_t)pass * adc_itp_code_stride(h->p.W, h->p.H, h->itp_ms);
    if (hipMemcpyAsync(dst, code, (size_t)pitch * rows, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return 2;
    return hipStreamSynchronize(h->stream) == hipSuccess ? 0 : 2;
}

int adc_debug_set_images(adc_handle* h, const uint8_t* left, const uint8_t* right)
{
    if (!h || !left || !right) return 1;
    hipSetDevice(h->device);
    const size_t P = (size_t)h->p.W * h->p.H;
    images_own(h, true); // (the packed left image is stale from here on, also behind a copy that fails half-way)
    if (hipMemcpy(h->img_l, left, P * 3, hipMemcpyHostToDevice) != hipSuccess) return 2;
    if (hipMemcpy(h->img_r, right, P * 3, hipMemcpyHostToDevice) != hipSuccess) return 2;
    return 0;
}

int adc_debug_run(adc_handle* h, int stage, int arg)
{
    if (!h) return 1;
    hipSetDevice(h->device);
    hipError_t e = hipSuccess;
    bool fuse_cost = false; AggArms arms = AGG_ARMS_UNKNOWN; // (ADC_RUN_AGGREGATE; unknown arms: two launches per pass, the kernels decide)
    switch (stage) {
    case ADC_RUN_GRAY_CENSUS: e = adc_launch_gray_census(h); break;
    case ADC_RUN_COST: e = adc_launch_cost(h, h->vol_a); break;
    case ADC_RUN_ARMS: e = adc_launch_arms(h); break;
    case ADC_RUN_AGGREGATE: // arg = iterations (default 4); arg >= 100: first pass with the fused cost computation
        e = hipMemsetAsync(h->armmax + ADC_NZ_BASE, 0, 2 * ADC_NZ_SHARDS * ADC_NZ_STRIDE * sizeof(int), h->heavy); // (the record densities: counted below)
        if (e == hipSuccess) e = adc_launch_records(h); // (needs ADC_RUN_GRAY_CENSUS before; reads the images instead of ADC_BUF_COST_INIT)
        // arg >= 200: additionally read the maximum arms back (needs ADC_RUN_ARMS before) so that the launcher picks
        // the ring depth on the host and fuses same-direction pass pairs -- the production pipeline's path
        if (e == hipSuccess && arg >= 200) {
            int am[2] = {0, 0};
            e = hipMemcpy(am, h->armmax, 2 * sizeof(int), hipMemcpyDeviceToHost);
            if (e == hipSuccess) learn_take_arms(&h->learned, am);
            if (e == hipSuccess) arms = AGG_ARMS_EXACT;
            // ... and the record densities of THIS image (the pipeline assumes the previous Match's)
            if (e == hipSuccess && h->pin_nz) e = hipMemcpyAsync(h->pin_nz, h->armmax + ADC_NZ_BASE, 2 * ADC_NZ_SHARDS * ADC_NZ_STRIDE * sizeof(int32_t), hipMemcpyDeviceToHost, h->heavy);
            if (e == hipSuccess && h->pin_nz) e = hipStreamSynchronize(h->heavy);
            if (e == hipSuccess && h->pin_nz) {
                long long nz[2];
                rec_nz_sums(h, nz);
                learn_take_densities(&h->learned, nz);
            }
            arg -= 200;
        }
        if (e == hipSuccess && arg >= 100) {
            if (h->paper & ADC_PAPER_RIGHT_ARMS) e = adc_launch_cost(h, h->vol_a); // (no fused form in this mode: recompute the volume)
            else { e = adc_launch_cost_records(h); fuse_cost = true; }
            arg -= 100;
        }
        if (e == hipSuccess) e = adc_launch_aggregate(h, arg > 0 ? arg : 4, arms, false, fuse_cost, false);
        break;
    case ADC_RUN_SCANLINE: // arg = passes (default 4); arg >= 100: the production form of the last pass, which also
                           // writes the left-view disparity map (ADC_BUF_DISP_LEFT) -- ADC_RUN_WTA then only adds the right view
        h->fly.wta_left_done = 0;
        e = adc_launch_scanline(h, arg >= 100 ? arg - 100 : arg, arg >= 100);
        break;
    case ADC_RUN_WTA: e = adc_launch_wta(h); break;
    case ADC_RUN_LRCHECK: e = adc_launch_lrcheck(h); break;
    case ADC_RUN_REGION_VOTING: // arg > 0: launch budget (kernels) of this run, e.g. 4 to force the continuation path
        if (arg < 0) { h->learned.irv_budget = -arg; return 0; } // test hook: only set the budget of the NEXT Match's chain (continuation inside adc_wait)
        if (arg > 0) h->learned.irv_budget = arg;
        e = adc_launch_sup_counts(h); // (the region boxes of the votes come out of the arms stage; here the arms may have been written by the test)
        if (e == hipSuccess) e = adc_run_region_voting(h);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) { int cont = 0; e = adc_voting_finish(h, &cont); }
        break;
    case ADC_RUN_INTERPOLATION: // arg 1: the f64 walk (k_interpolate_rays) also where the handle would take the table walk (itp_plan.h)
        e = adc_launch_interpolation(h, arg == 1);
        break;
    case ADC_RUN_DISCONTINUITY: e = adc_launch_discontinuity(h); break;
    case ADC_RUN_MEDIAN: // arg 100: test hook -- arm the fallback path of the NEXT adc_wait (as if a band had timed out)
        if (arg == 100) { h->fly.force_median_fallback = 1; return 0; }
        if (arg == 101) { h->fly.force_median_fallback = 2; return 0; } // ... as if a speculative seam had differed (chained form redone)
        e = adc_launch_median(h);
        break;
    default: return 1;
    }
    if (e != hipSuccess) { set_error("adc_debug_run launch", e); return 2; }
    e = hipStreamSynchronize(h->heavy);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { set_error("adc_debug_run sync", e); return 2; }
    if (stage == ADC_RUN_SCANLINE && h->so_nseg_last > 1) {
        // (round-4 advisor finding) the row passes ran as speculative segments; behind a Match adc_wait redoes the stage with whole
        // rows when a seam failed -- here the aggregated volume is gone (the passes ping-pong over it), so a failed seam is an
        // ERROR of the debug call instead of a silently inexact volume
        int fails = 0;
        if (hipMemcpy(&fails, h->armmax + 2, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) { set_error("adc_debug_run: seam flag", hipGetLastError()); return 2; }
        if (fails != 0) { // (as behind a Match: the handle's next scanline runs take whole rows, so a caller can write the volume again and rerun)
            learn_so_seam_failed(&h->learned);
            g_last_error = "adc_debug_run(ADC_RUN_SCANLINE): a speculative row segment failed its seam check; rerun with ADC_SO_SEG=1";
            return 3;
        }
    }
    if (stage == ADC_RUN_MEDIAN && h->pin_flags && h->pin_flags[ADC_PIN_MEDIAN] != 0) { // what adc_wait does behind a Match
        e = adc_median_fallback(h);
        h->pin_flags[ADC_PIN_MEDIAN] = 0;
        if (e != hipSuccess) { set_error("adc_debug_run: median fallback", e); return 2; }
    }
    return 0;
}

int64_t adc_debug_counter(adc_handle* h, int which)
{
    if (!h) return -1;
    switch (which) {
    case 0: return h->lstats.median_fallbacks;
    case 1: return h->lstats.irv_overflows;
    case 2: return h->lstats.arm_redos;
    case 9: return h->lstats.agg_switches;   // consecutive Matches that needed different aggregation plans
    case 10: return h->agg_dual_runs; // Matches whose aggregation was enqueued as two plans (the device chose)
    case 11: return h->lstats.redo_partial;  // redos that restarted at the aggregation (not the whole Match)
    case 12: return h->learned.agg_dual;      // > 0: the next Match enqueues both plans
    case 13: return h->agg_so_fusions; // Matches whose last aggregation pass ran inside the first scanline pass
    case 16: return h->agg_sparse_launches; // small-ring aggregation launches that ran in their sparse form (+ k_agg_apply)
    case 17: return (int64_t)(adc_agg_sparse_density() * 1e6 + 0.5); // density threshold of the sparse form, parts per million of the pixels
    case 20: return h->agg_gather_launches; // ... of which in the gather form (k_agg_gather + k_agg_apply)
    case 21: return (int64_t)(adc_agg_gather_density() * 1e6 + 0.5); // density threshold of the gather form, parts per million of the pixels
    case 22: return h->agg_flat_launches; // first aggregation launches that ran as k_cost_agg_flat (element-wise) instead of the small-ring march
    case 23: return (int64_t)(adc_cost_flat_density() * 1e6 + 0.5); // density threshold of the flat first launch, parts per million of the pixels
    case 24: { // first aggregation launch of the last Match in nanoseconds, from the aggregation marks (profiling on, one plan enqueued); else -1
        float ms = 0.f;
        if (!h->profiling || h->agg_dual_last || h->agg_launches < 1 || hipEventElapsedTime(&ms, h->ev_agg[0], h->ev_agg[1]) != hipSuccess) return -1;
        return (int64_t)((double)ms * 1e6 + 0.5);
    }
    case 18: return h->learned.rec_nz_known ? h->learned.rec_nz[0] : -1; // pixels with a pass-changing horizontal record the handle last saw
    case 19: return h->learned.rec_nz_known ? h->learned.rec_nz[1] : -1; // ... vertical record
    case 14: return h->irv_xcd_mode;   // the voting chain sweeps band -> XCD (the mapping was probed on this device)
    case 15: return h->med_seg_last;   // column segments per band link of the last banded median launch (1: whole rows)
    case 3: return h->learned.irv_budget;
    case 7: return h->lstats.med_spec_fails;
    case 8: return h->med_spec_last;
    case 4: return h->lstats.so_seam_redos;
    case 5: return h->so_nseg_last; // segments per row of the last scanline run
    case 6: { // seams that failed in the last scanline run (debug surface: nothing redoes it there)
        int v = -1;
        return hipMemcpy(&v, h->armmax + 2, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess ? v : -1;
    }
    default: return -1;
    }
}

int adc_debug_voting_stats(adc_handle* h, int64_t* rounds, int64_t* evaluations)
{
    if (!h) return 1;
    if (rounds) *rounds = h->vote_rounds;
    if (evaluations) *evaluations = h->vote_evals;
    return 0;
}

} // extern "C"
