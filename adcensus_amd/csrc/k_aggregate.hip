// k_aggregate.hip -- K4 cross-based cost aggregation (the roofline kernel of the pipeline).
//
// Replaces CrossAggregator::{Aggregate, AggregateInArms} (cross_aggregator.cpp:89-118,327-394):
// 4 iterations (H-first, V-first, H-first, V-first); per iteration two 1-D passes over the whole
// volume, each output = sequential f32 sum (from 0.0f, in the order t = -arm ... +arm, which is
// observable in the WTA result -- SURVEY.md A.4) of the inputs inside the pixel's own arm; the second
// pass of an iteration divides by the support count.
//
// MI355X mapping ("marching ring"):
//   * layout [y][x][Dp], lanes = disparities: a wave owns 64 consecutive floats (256 B) of every
//     pixel of ONE image line (a row for the H pass, a column for the V pass) and marches along it.
//     Arms and support counts are wave-uniform (scalar loads, no divergence).
//   * every input element is read from HBM exactly once per pass (+ the 34-pixel halo at segment
//     ends): the last 2L+1 line entries live in an LDS ring (256 B x (2L+1) per wave, each lane
//     only ever reads what it wrote itself, so no barriers), the next AGG_PF entries are in flight
//     in registers (software prefetch) -- that is what keeps ~10 MB of loads outstanding chip-wide.
//   * algorithmic bytes per pass: read V + write V (+4 B/pixel arms, +2 B/pixel counts), V = 4*W*H*Dp.
#include "adc_internal.h"
#include "adc_device_fn.h"
#include "agg_plan.h"
#include <mutex>
#include "k_aggregate_rr.h"
#include "k_aggregate_rr2.h"
#include "k_agg_gather.h"

// ---------------------------------------------------------------------------------- marching ring
// One 64-lane workgroup (= one wave) per line segment.
//   * LDS per wave = (2L+1) x 256 B (17.25 KiB at L = 34) => 9 waves per CU, 2304 chip-wide: all 2160
//     H-lines of a 1080p / D=128 volume run in ONE round;
//   * the next AGG_PF entries and their packed {arm_lo, arm_hi, count} records are in flight in
//     registers.  These prefetch loads are issued from inline asm and waited for with a hand-counted
//     s_waitcnt vmcnt: hipcc's loop-carried vmcnt model otherwise drains the queue to a depth of ~3 steps
//     (tools/ubench/agg_lean.hip vs agg_asm.hip).  VMEM ops per steady-state step, in program order:
//     [data load][record load] ... [output store]; vmcnt retires in order on gfx9-family hardware.
// Measured (tools/ubench): the same load/store structure without the ordered sum streams at the
// float4-copy rate (4.8-5.4 TB/s on MI355X); the full step is bound by its dependent chain
// (LDS write -> LDS reads -> ordered adds -> store) at 9 waves per CU.
#define AGG_PF 8
#ifndef ADC_K4_TAILLOOP
#define ADC_K4_TAILLOOP 0 // A/B switch: 1 = element-wise tail loop in the compact span sum
#endif
#ifndef ADC_K4_DIAG
#define ADC_K4_DIAG 0 // timing experiments only (wrong results): 1 = no span sums, 2 = no division, 3 = spans capped at 4
#endif

// ordered partial sum over cnt consecutive ring entries starting at q (lane-private column, stride 64 floats)
__device__ __forceinline__ float agg_run(float acc, const float* q, int cnt)
{
    while (cnt >= 8) {
        const float t0 = q[0], t1 = q[64], t2 = q[128], t3 = q[192], t4 = q[256], t5 = q[320], t6 = q[384], t7 = q[448];
        acc += t0; acc += t1; acc += t2; acc += t3; acc += t4; acc += t5; acc += t6; acc += t7;
        q += 512;
        cnt -= 8;
    }
    switch (cnt) { // exact-length tail (reads only what it adds)
    case 7: { const float t0 = q[0], t1 = q[64], t2 = q[128], t3 = q[192], t4 = q[256], t5 = q[320], t6 = q[384];
              acc += t0; acc += t1; acc += t2; acc += t3; acc += t4; acc += t5; acc += t6; } break;
    case 6: { const float t0 = q[0], t1 = q[64], t2 = q[128], t3 = q[192], t4 = q[256], t5 = q[320];
              acc += t0; acc += t1; acc += t2; acc += t3; acc += t4; acc += t5; } break;
    case 5: { const float t0 = q[0], t1 = q[64], t2 = q[128], t3 = q[192], t4 = q[256];
              acc += t0; acc += t1; acc += t2; acc += t3; acc += t4; } break;
    case 4: { const float t0 = q[0], t1 = q[64], t2 = q[128], t3 = q[192]; acc += t0; acc += t1; acc += t2; acc += t3; } break;
    case 3: { const float t0 = q[0], t1 = q[64], t2 = q[128]; acc += t0; acc += t1; acc += t2; } break;
    case 2: { const float t0 = q[0], t1 = q[64]; acc += t0; acc += t1; } break;
    case 1: acc += q[0]; break;
    default: break;
    }
    return acc;
}

// Compact form for the small-ring kernels (spans of at most 2*8+1 entries): same ordered sum, a fraction of the code --
// the fully unrolled form above is inlined four times per step of the pair kernel and made its steady-state loop
// ~38 KB of instructions.
// (V = float, or a pair of floats when a lane owns two disparities: the two sums are independent chains)
typedef float agg_f2 __attribute__((ext_vector_type(2)));
template <int VPL> struct AggT { typedef float V; };
template <> struct AggT<2> { typedef agg_f2 V; };
template <class V>
__device__ __forceinline__ V agg_run_compact(V acc, const V* q, int cnt)
{
#pragma nounroll
    for (; cnt >= 4; cnt -= 4, q += 256) {
        const V t0 = q[0], t1 = q[64], t2 = q[128], t3 = q[192];
        acc += t0; acc += t1; acc += t2; acc += t3;
    }
#if ADC_K4_TAILLOOP
#pragma nounroll
    for (; cnt > 0; cnt--, q += 64) acc += q[0];
#else
    // the last 1..3 entries with all their reads in flight at once (an element-wise loop pays one LDS round trip and
    // four scalar instructions per entry; on short-arm images almost every span ends here)
    if (cnt == 3) {
        const V t0 = q[0], t1 = q[64], t2 = q[128];
        acc += t0; acc += t1; acc += t2;
    } else if (cnt == 2) {
        const V t0 = q[0], t1 = q[64];
        acc += t0; acc += t1;
    } else if (cnt == 1) {
        acc += q[0];
    }
#endif
    return acc;
}
template <bool SMALL_, class V>
__device__ __forceinline__ V agg_sum(V acc, const V* q, int cnt)
{
    if constexpr (SMALL_) return agg_run_compact<V>(acc, q, cnt);
    else {
        static_assert(SMALL_ || sizeof(V) == sizeof(float), "the full ring is used with one disparity per lane");
        return agg_run(acc, q, cnt);
    }
}

// SMALL: the small-ring launch (own kernel name in profiles; compact summation code).
// COSTIN (first pass of the production pipeline, rows, non-dividing): there is no input volume -- each entry of the
// line, i.e. the AD-Census matching cost of pixel (x, y) for this wave's 64 disparities (cost_computor.cpp:82-121), is
// computed in registers.  Lane l owns disparity d = d_first + l and needs the right-image pixel of column x - d: as the
// wave marches in x that column moves one lane per step, so the window {bgrx, census} is a DPP wave_shr:1 shift with
// the one new column (x - d_first) entering at lane 0; the new column and the left pixel of x arrive as uniform
// 16-byte records (k_cost_records, rows padded with out-of-image markers), prefetched like the arm records.
// AD = v_sad_u8 of the packed colours, Hamming = two v_bcnt on the xor of the census words, cost = A[ad] - C[hm] from
// the host-built tables (in LDS behind the ring) -- bit-identical to k_cost.  Saves writing V and reading it back.
// (struct AggCostIn: k_aggregate_rr2.h)
typedef unsigned long long agg_u64;

// PAIR: TWO consecutive passes of the same direction in one launch (the dividing second pass of an iteration and the
// non-dividing first pass of the next one: V1+V2, H2+H3, V3+V4).  The first pass's outputs are not stored but pushed
// into a second ring (and their arm records into a small record ring); as soon as output m of the first pass
// exists, output m-L of the second pass can be summed from the second ring -- same ordered sums, same division, so
// the result is bit-identical, but the intermediate volume never travels to HBM and back (8 passes -> 5 launches).
// Needs two rings per wave, so it is used with the small ring only (armmax <= small_L, decided on the host).
// VPL = disparities per lane (1, or 2 with the small ring when Dp is a multiple of 128): with two, a wave owns 512
// contiguous bytes of every pixel of its line, all wave-uniform work of a step (records, ring slots, branches, waits) is
// shared by twice the data and the two sums of a lane are independent chains.
// REGRING (full ring, plain pass): the ring lives in REGISTERS -- VGPRs v56..v127, outside the range the compiler may
// allocate for this kernel (amdgpu_num_vgpr) -- and is addressed with the VGPR index mode (s_set_gpr_idx_on: the
// ring slots are wave-uniform, M0 holds the index).  A span entry costs one indexed v_add_f32 and one s_add on M0
// instead of an LDS round trip, there is no LDS allocation at all, and 128 VGPRs allow 16 waves per CU where the
// 17 KiB LDS ring allowed 9.  Same entries, same order, same adds: bit-identical (tools/ubench/regring.hip).
#define AGG_RING_V0 56
#define AGG_RING_REGS 72
#define AGG_RING_CLOBBERS                                                                                             \
    "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72",  \
        "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88",    \
        "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103",       \
        "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117",    \
        "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127"
// ring[slot] = v
__device__ __forceinline__ void agg_reg_push(int slot, float v)
{
    asm volatile("s_set_gpr_idx_on %0, gpr_idx(DST)\n\tv_mov_b32 v56, %1\n\ts_set_gpr_idx_off" ::"s"(slot), "v"(v)
                 : "m0", AGG_RING_CLOBBERS);
}
// acc += ring[idx], ring[idx+1], ... (cnt entries, no wrap), in this order: blocks of 16 indexed adds entered late
// through a computed jump.  The index register M0 is set ONCE per block: the adds name the registers v40..v55 and the
// hardware adds M0 = idx + c to the register number, so block position p reads v[40 + p + idx + c]; entering at position
// 16 - c makes that v[56 + idx] ... v[56 + idx + c - 1].  (v40..v55 only appear as encodings: every register actually
// read lies in the ring.)  One add = 4 bytes; 12 = the three scalar instructions between the value s_getpc returns and
// the first add.  A first version advanced M0 with an s_add per entry: 13 more scalar instructions per step on a
// kernel whose scalar unit is saturated (SQ counters).
__device__ __forceinline__ float agg_reg_sum(float acc, int idx, int cnt)
{
    static_assert(AGG_RING_V0 == 56, "the add block below names v40..v55 = AGG_RING_V0 - 16 + position");
    while (cnt > 0) {
        const int c = cnt < 16 ? cnt : 16;
        const int off = 12 + 4 * (16 - c);
        const int m = idx + c;
        asm volatile("s_set_gpr_idx_on %1, gpr_idx(SRC0)\n\t"
                     "s_getpc_b64 vcc\n\t"
                     "s_add_u32 vcc_lo, vcc_lo, %2\n\t"
                     "s_addc_u32 vcc_hi, vcc_hi, 0\n\t"
                     "s_setpc_b64 vcc\n\t"
                     "v_add_f32_e32 %0, v40, %0\n\tv_add_f32_e32 %0, v41, %0\n\tv_add_f32_e32 %0, v42, %0\n\tv_add_f32_e32 %0, v43, %0\n\t"
                     "v_add_f32_e32 %0, v44, %0\n\tv_add_f32_e32 %0, v45, %0\n\tv_add_f32_e32 %0, v46, %0\n\tv_add_f32_e32 %0, v47, %0\n\t"
                     "v_add_f32_e32 %0, v48, %0\n\tv_add_f32_e32 %0, v49, %0\n\tv_add_f32_e32 %0, v50, %0\n\tv_add_f32_e32 %0, v51, %0\n\t"
                     "v_add_f32_e32 %0, v52, %0\n\tv_add_f32_e32 %0, v53, %0\n\tv_add_f32_e32 %0, v54, %0\n\tv_add_f32_e32 %0, v55, %0\n\t"
                     "s_set_gpr_idx_off"
                     : "+v"(acc)
                     : "s"(m), "s"(off)
                     : "m0", "scc", "vcc", AGG_RING_CLOBBERS);
        idx += c;
        cnt -= c;
    }
    return acc;
}

// SPARSE (small ring, volume input): the launch issues the volume store of an output only when the pixel's own record
// makes a pass change it (adc_rec_changes_pixel) -- every other output is bit for bit what the launch READ at that index, so
// the result of the launch is "src with the stored pixels replaced"; k_agg_apply copies those back into src behind it.
// Loads, rings, sums, division, segments and halos are the dense form's.
template <bool VERT, bool DIVIDE, bool SMALL, bool COSTIN, bool PAIR, int VPL, bool REGRING, bool SPARSE = false>
__device__ __forceinline__ void agg_march_body(const float* __restrict__ src, float* __restrict__ dst,
                                               const uint32_t* __restrict__ rec, // {lo, hi, count16} per pixel, line-major
                                               int W, int H, int Dp, int L, int seg_len, int nseg, int per_xcd,
                                               const int* __restrict__ armmax, int small_variant, int small_L,
                                               const AggCostIn& ci)
{
    static_assert(!REGRING || (!SMALL && !PAIR && VPL == 1), "register ring here: the fused-cost first pass (plain passes and pairs: k_aggregate_rr.h)");
    static_assert(!COSTIN || (!VERT && !DIVIDE), "the fused cost is for the first (row, non-dividing) pass");
    static_assert(!PAIR || (DIVIDE && !COSTIN), "a fused pair = dividing pass + the following non-dividing pass");
    static_assert(VPL == 1 || (VPL == 2 && SMALL && !COSTIN), "two disparities per lane: small ring, no fused cost");
    static_assert(!SPARSE || (SMALL && !COSTIN && !REGRING), "sparse stores: the regular small-ring launches");
    typedef typename AggT<VPL>::V V;
    const V vzero = (V)(0.0f);
    // small_variant >= 0 (host does not know the arms, debug path): two launches per pass, the window depth follows
    // the data.  When no arm of this direction exceeds small_L (e.g. noise-like images) the small-ring variant runs at
    // 32 waves/CU and the full-ring variant exits at once, otherwise the other way round (armmax[0] = max horizontal
    // arm, armmax[1] = max vertical arm, from k_build_arms).  small_variant < 0: the host has read armmax and
    // launches only the variant that applies.
    // small_variant == 2: the host ASSUMED (from the previous Match of the handle) that no arm of this direction exceeds
    // small_L = the ring depth of this launch; when the assumption is wrong the pass is skipped and armmax[3] raised --
    // adc_wait then redoes the Match with the full ring.
    // small_variant 3 / 4: two plans enqueued back to back, exactly one of them works (agg_gate_skip, k_aggregate_rr.h)
    if (agg_gate_skip(armmax, small_variant, small_L, VERT)) return;
    extern __shared__ __attribute__((aligned(16))) float ring_all[];
    const int R = 2 * L + 1;
    const int lane = threadIdx.x;
    V* ring = reinterpret_cast<V*>(ring_all) + lane; // entry s at ring[s*64]; each lane only reads what it wrote

    const int chunks = Dp / (64 * VPL);         // (64*VPL)-float chunks per pixel
    const int N = VERT ? H : W;                 // length of a line
    const int nlines = (VERT ? W : H) * chunks; // independent lines
    // XCD-aware mapping: hardware places block b on XCD b % 8; give each XCD a contiguous band of lines
    const int b = (int)blockIdx.x;
    const int gw = (b & 7) * per_xcd + (b >> 3);
    if ((b >> 3) >= per_xcd || gw >= nlines * nseg) return;
    const int seg = gw / nlines;
    const int line = gw - seg * nlines;
    const int fixed = line / chunks; // x (V pass) or y (H pass)
    const int chunk = line - fixed * chunks;

    // [s0, s1) = the outputs this wave delivers; [m0, m1) = the outputs of the (first) pass it has to compute for them
    const int s0 = seg * seg_len;
    const int s1 = adc_imin(N, s0 + seg_len);
    if (s0 >= s1) return;
    const int m0 = PAIR ? adc_imax(0, s0 - L) : s0;
    const int m1 = PAIR ? adc_imin(N, s1 + L) : s1;
    const int lo = adc_imax(0, m0 - L);
    const int hi = adc_imin(N, m1 + L);

    // element m of this line
    const long long pix_step = VERT ? (long long)W : 1LL;
    const long long pix0 = VERT ? (long long)fixed : (long long)fixed * W;
    const long long fstep = pix_step * Dp;
    const float* sp = src + pix0 * Dp + chunk * (64 * VPL) + lane * VPL;
    float* dp = dst + pix0 * Dp + chunk * (64 * VPL) + lane * VPL;
    const uint32_t* rp = rec + (long long)fixed * N; // records of this line, contiguous along m

    // ---- fused cost state (COSTIN)
    float* lutA = ring_all + (REGRING ? 0 : R * 64); // A[766] then C[64] behind the LDS ring (COSTIN: VPL == 1)
    float* lutC = lutA + 768;
    uint32_t wB = 0, wC0 = 0, wC1 = 0;          // this lane's right-image pixel {bgrx, census} for the current entry
    const uint4* rrow = nullptr;                 // rrow[x] = right record of column x - d_first (lane 0's column)
    const uint4* lrow = nullptr;
    bool pad_lane = false;
    if constexpr (COSTIN) {
        for (int i = lane; i < 766; i += 64) lutA[i] = ci.lut_ad[i];
        lutC[lane] = ci.lut_census[lane];
        const int d_first = chunk * 64 + ci.dmin;
        pad_lane = chunk * 64 + lane >= ci.D;
        rrow = ci.rrec + (size_t)fixed * ci.rpitch + ci.padl - d_first;
        lrow = ci.lrec + (size_t)fixed * W;
        // window of the entry BEFORE the first one (column lo-1-d); the first real step shifts it into place
        const uint4* rbase = ci.rrec + (size_t)fixed * ci.rpitch;
        int gi = ci.padl - d_first + lo - 1 - lane;
        gi = gi < 0 ? 0 : (gi >= ci.rpitch ? ci.rpitch - 1 : gi); // index 0 is a marker column (padl >= 1)
        const uint4 g0 = rbase[gi];
        wB = g0.x; wC0 = g0.y; wC1 = g0.z;
    }
// matching cost of the next entry: (RB, RC0, RC1) = new right pixel {bgrx, census lo, census hi} entering at lane 0,
// (LB, LC0, LC1) = left pixel of the entry (both wave-uniform)
#define AGG_COST(RB, RC0, RC1, LB, LC0, LC1, OUT)                                                                  \
    do {                                                                                                           \
        wB = (uint32_t)__builtin_amdgcn_update_dpp((int)(RB), (int)wB, 0x138, 0xf, 0xf, false);                    \
        wC0 = (uint32_t)__builtin_amdgcn_update_dpp((int)(RC0), (int)wC0, 0x138, 0xf, 0xf, false);                 \
        wC1 = (uint32_t)__builtin_amdgcn_update_dpp((int)(RC1), (int)wC1, 0x138, 0xf, 0xf, false);                 \
        const uint32_t ad_ = __builtin_amdgcn_sad_u8(wB, (uint32_t)(LB), 0u);                                      \
        const uint32_t hm_ = __popc(wC0 ^ (uint32_t)(LC0)) + __popc(wC1 ^ (uint32_t)(LC1));                        \
        float cv_ = lutA[ad_ < 766u ? ad_ : 765u] - lutC[hm_ & 63u]; /* == ((1 - ea) + 1) - ec, cost_computor.cpp:117 */ \
        cv_ = wB == 0xFFFFFFFFu ? 1.0f : cv_; /* right pixel outside the image (:101-104) */                        \
        OUT = pad_lane ? 0.0f : cv_;                                                                               \
    } while (0)

    int slot_w = 0;          // ring slot of the next entry to be written
    int slot_m = m0 - lo;    // ring slot of entry m0 (<= L < R)
    float* dpn = dp + (long long)s0 * fstep; // outputs leave in increasing order, starting at s0
    // ---- second stage (PAIR): ring of first-pass outputs + their records, behind the first ring
    V* ring2 = reinterpret_cast<V*>(ring_all) + R * 64 + lane;
    uint32_t* recring = reinterpret_cast<uint32_t*>(reinterpret_cast<V*>(ring_all) + 2 * R * 64);
    int slot2_w = 0;           // slot of the next first-pass output to be written
    int slot2_s = s0 - m0;     // slot of first-pass output s0 (the next second-pass output)
    int mcur = m0;             // index of the next first-pass output
// second-pass output: ordered sum of first-pass outputs over the pixel's own arm span, no division
#define AGG_EMIT2()                                                                               \
    do {                                                                                          \
        const uint32_t r2_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)recring[slot2_s]);     \
        const int b_lo_ = (int)(r2_ & 255u), b_hi_ = (int)((r2_ >> 8) & 255u);                    \
        int i2_ = slot2_s - b_lo_;                                                                \
        if (i2_ < 0) i2_ += R;                                                                    \
        const int k_ = b_lo_ + b_hi_ + 1;                                                         \
        V acc2_;                                                                                  \
        if (k_ == 1) {                                                                            \
            acc2_ = vzero + ring2[i2_ * 64];                                                      \
        } else {                                                                                  \
            const int k1_ = adc_imin(k_, R - i2_);                                                \
            acc2_ = agg_sum<SMALL, V>(vzero, ring2 + i2_ * 64, k1_);                              \
            if (k_ > k1_) acc2_ = agg_sum<SMALL, V>(acc2_, ring2, k_ - k1_);                      \
        }                                                                                         \
        if (!SPARSE || adc_rec_changes_pixel(r2_, true)) ADC_VOL_STORE(reinterpret_cast<V*>(dpn), acc2_); \
        dpn += fstep;                                                                             \
        slot2_s = slot2_s + 1 == R ? 0 : slot2_s + 1;                                             \
    } while (0)
// what happens to a finished first-pass output
#define AGG_OUT(ACC, RECV)                                                                        \
    do {                                                                                          \
        if constexpr (PAIR) {                                                                     \
            ring2[slot2_w * 64] = (ACC);                                                          \
            recring[slot2_w] = (RECV); /* wave-uniform value, same address in every lane */       \
            slot2_w = slot2_w + 1 == R ? 0 : slot2_w + 1;                                         \
            const int s_ = mcur - L; /* its look-ahead (<= L) is complete now */                  \
            mcur++;                                                                               \
            if (s_ >= s0 && s_ < s1) AGG_EMIT2();                                                 \
        } else {                                                                                  \
            if (!SPARSE || adc_rec_changes_pixel((RECV), DIVIDE)) ADC_VOL_STORE(reinterpret_cast<V*>(dpn), (ACC)); \
            dpn += fstep;                                                                         \
        }                                                                                         \
    } while (0)

#define AGG_PUSH(V)                                \
    do {                                           \
        if constexpr (REGRING) agg_reg_push(slot_w, (V)); \
        else ring[slot_w * 64] = (V);              \
        slot_w = slot_w + 1 == R ? 0 : slot_w + 1; \
    } while (0)

#define AGG_EMIT(M, REC)                                                                          \
    do {                                                                                          \
        const uint32_t r_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(REC));                \
        const int a_lo_ = (int)(r_ & 255u), a_hi_ = (int)((r_ >> 8) & 255u);                      \
        int idx_ = slot_m - a_lo_;                                                                \
        if (idx_ < 0) idx_ += R;                                                                  \
        const int n_ = ADC_K4_DIAG == 1 ? 1 : (ADC_K4_DIAG == 3 ? adc_imin(4, a_lo_ + a_hi_ + 1) : a_lo_ + a_hi_ + 1); \
        V acc_;                                                                                   \
        if constexpr (REGRING) {                                                                  \
            const int n1_ = adc_imin(n_, R - idx_);                                               \
            acc_ = agg_reg_sum(vzero, idx_, n1_);                                                 \
            if (n_ > n1_) acc_ = agg_reg_sum(acc_, 0, n_ - n1_);                                  \
        } else if (n_ == 1) {                                                                     \
            acc_ = vzero + ring[idx_ * 64]; /* arms 0/0: the sum is the pixel itself */           \
        } else {                                                                                  \
            const int n1_ = adc_imin(n_, R - idx_);                                               \
            acc_ = agg_sum<SMALL, V>(vzero, ring + idx_ * 64, n1_); /* t = -arm .. +arm */         \
            if (n_ > n1_) acc_ = agg_sum<SMALL, V>(acc_, ring, n_ - n1_); /* wrapped part */      \
        }                                                                                         \
        if (DIVIDE && ADC_K4_DIAG != 2) {                                                         \
            const uint32_t c_ = r_ >> 16;                                                         \
            if (c_ != 1u) acc_ = acc_ / (float)c_; /* cross_aggregator.cpp:389 (x/1 == x) */     \
        }                                                                                         \
        AGG_OUT(acc_, r_);                                                                        \
        (void)(M);                                                                                \
        slot_m = slot_m + 1 == R ? 0 : slot_m + 1;                                                \
    } while (0)

    // ---- phase A: entries lo .. jB-1 that precede the first output's look-ahead (no output yet)
    const int jB = adc_imin(hi, m0 + L);
    if constexpr (COSTIN) {
        for (int j = lo; j < jB; j++) {
            const uint4 rn = rrow[j], ln = lrow[j];
            float v;
            AGG_COST(rn.x, rn.y, rn.z, ln.x, ln.y, ln.z, v);
            AGG_PUSH(v);
        }
    } else {
    for (int j = lo; j < jB; j += AGG_PF) {
        V t[AGG_PF];
#pragma unroll
        for (int u = 0; u < AGG_PF; u++) t[u] = *reinterpret_cast<const V*>(sp + (long long)adc_imin(j + u, jB - 1) * fstep);
#pragma unroll
        for (int u = 0; u < AGG_PF; u++)
            if (j + u < jB) AGG_PUSH(t[u]);
    }
    }

    // ---- phase B (steady state): entry jj arrives, output m = jj - L leaves.
    // All compiler-tracked VMEM traffic of phase A is drained first, so the manual vmcnt bookkeeping
    // below starts from an empty queue.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int j = jB;
    if constexpr (COSTIN) {
        // Same pipeline without the data load: VMEM ops per steady-state step = [arm record load] ... [output store].
        // The pixel records arrive in BULK: every 64 entries lane l loads the records of entry block_start + l (six
        // dword loads per block, issued a whole block ahead), and each step picks its entry's six dwords with
        // v_readlane (wave-uniform values).  The bulk loads make the hand-counted waits conservative (never unsafe).
        if (j + 2 * AGG_PF <= hi) {
            uint32_t cR0, cR1, cR2, cL0, cL1, cL2; // current block: records of entries bx0 + lane
            uint32_t nR0, nR1, nR2, nL0, nL1, nL2; // next block (in flight)
            uint32_t pr[AGG_PF];
            const uint4* rbase_ = ci.rrec + (size_t)fixed * ci.rpitch;
            const int roff_ = (int)(rrow - rbase_); // rrow[x] == rbase_[x + roff_]
            int bx0 = j, bpos = 0;
#define AGG_BULK_ISSUE(X0)                                                                                        \
    do {                                                                                                          \
        int ir_ = (X0) + lane + roff_;                                                                            \
        ir_ = ir_ < 0 ? 0 : (ir_ >= ci.rpitch ? ci.rpitch - 1 : ir_);                                             \
        const int il_ = adc_imin((X0) + lane, W - 1);                                                             \
        const uint4* pr_ = rbase_ + ir_;                                                                          \
        const uint4* pl_ = lrow + il_;                                                                            \
        asm volatile("global_load_dword %0, %1, off" : "=v"(nR0) : "v"(pr_) : "memory");                          \
        asm volatile("global_load_dword %0, %1, off offset:4" : "=v"(nR1) : "v"(pr_) : "memory");                 \
        asm volatile("global_load_dword %0, %1, off offset:8" : "=v"(nR2) : "v"(pr_) : "memory");                 \
        asm volatile("global_load_dword %0, %1, off" : "=v"(nL0) : "v"(pl_) : "memory");                          \
        asm volatile("global_load_dword %0, %1, off offset:4" : "=v"(nL1) : "v"(pl_) : "memory");                 \
        asm volatile("global_load_dword %0, %1, off offset:8" : "=v"(nL2) : "v"(pl_) : "memory");                 \
    } while (0)
#define AGG_BULK_TAKE(WAIT)                                                                                       \
    asm volatile(WAIT "v_mov_b32 %0, %6\n\tv_mov_b32 %1, %7\n\tv_mov_b32 %2, %8\n\tv_mov_b32 %3, %9\n\t"           \
                      "v_mov_b32 %4, %10\n\tv_mov_b32 %5, %11"                                                    \
                 : "=&v"(cR0), "=&v"(cR1), "=&v"(cR2), "=&v"(cL0), "=&v"(cL1), "=&v"(cL2)                         \
                 : "v"(nR0), "v"(nR1), "v"(nR2), "v"(nL0), "v"(nL1), "v"(nL2) : "memory")
            AGG_BULK_ISSUE(bx0);
            AGG_BULK_TAKE("s_waitcnt vmcnt(0)\n\t");
            AGG_BULK_ISSUE(bx0 + 64);
            const uint32_t* rpn = rp + (j - L);    // record of the output that entry triggers (>= m0)
#pragma unroll
            for (int u = 0; u < AGG_PF; u++) {
                asm volatile("global_load_dword %0, %1, off" : "=v"(pr[u]) : "v"(rpn) : "memory");
                rpn += 1;
            }
// next block: its loads were issued >= 64 steps (>= 128 VMEM operations) ago and at most 63 can be outstanding
#define AGG_BULK_NEXT()                                                                                           \
    if (bpos == 64) {                                                                                             \
        AGG_BULK_TAKE("");                                                                                        \
        bx0 += 64;                                                                                                \
        bpos = 0;                                                                                                 \
        AGG_BULK_ISSUE(bx0 + 64);                                                                                 \
    }
#define AGG_STEPC(U, WAITN, REFILL)                                                                               \
    do {                                                                                                          \
        uint32_t rr_;                                                                                             \
        asm volatile("s_waitcnt vmcnt(%2)\n\tv_mov_b32 %0, %1" : "=&v"(rr_) : "v"(pr[U]), "n"(WAITN) : "memory"); \
        if (REFILL) {                                                                                             \
            asm volatile("global_load_dword %0, %1, off" : "=v"(pr[U]) : "v"(rpn) : "memory");                    \
            rpn += 1;                                                                                             \
        }                                                                                                         \
        const int li_ = bpos + (U);                                                                               \
        const uint32_t rb_ = (uint32_t)__builtin_amdgcn_readlane((int)cR0, li_);                                  \
        const uint32_t rc0_ = (uint32_t)__builtin_amdgcn_readlane((int)cR1, li_);                                 \
        const uint32_t rc1_ = (uint32_t)__builtin_amdgcn_readlane((int)cR2, li_);                                 \
        const uint32_t lb_ = (uint32_t)__builtin_amdgcn_readlane((int)cL0, li_);                                  \
        const uint32_t lc0_ = (uint32_t)__builtin_amdgcn_readlane((int)cL1, li_);                                 \
        const uint32_t lc1_ = (uint32_t)__builtin_amdgcn_readlane((int)cL2, li_);                                 \
        float v_;                                                                                                 \
        AGG_COST(rb_, rc0_, rc1_, lb_, lc0_, lc1_, v_);                                                           \
        AGG_PUSH(v_);                                                                                             \
        AGG_EMIT(j + (U)-L, rr_); /* exactly one compiler-issued VMEM op (the store) */                           \
    } while (0)
            // first iteration: younger ops = 1 per not yet taken prologue slot + 2 per finished step
            static_assert(AGG_PF == 8, "the peeled first iteration below is written for AGG_PF == 8");
            AGG_STEPC(0, 7, true); AGG_STEPC(1, 8, true); AGG_STEPC(2, 9, true); AGG_STEPC(3, 10, true);
            AGG_STEPC(4, 11, true); AGG_STEPC(5, 12, true); AGG_STEPC(6, 13, true); AGG_STEPC(7, 14, true);
            j += AGG_PF;
            bpos += AGG_PF;
            for (; j + 2 * AGG_PF <= hi; j += AGG_PF) { // steady state: 2 ops per younger step (+ a bulk issue at times)
                AGG_BULK_NEXT();
                AGG_STEPC(0, 14, true); AGG_STEPC(1, 14, true); AGG_STEPC(2, 14, true); AGG_STEPC(3, 14, true);
                AGG_STEPC(4, 14, true); AGG_STEPC(5, 14, true); AGG_STEPC(6, 14, true); AGG_STEPC(7, 14, true);
                bpos += AGG_PF;
            }
            // drain: the AGG_PF records still in flight belong to entries j .. j+AGG_PF-1 (all < hi)
            AGG_BULK_NEXT();
            AGG_STEPC(0, 0, false); AGG_STEPC(1, 0, false); AGG_STEPC(2, 0, false); AGG_STEPC(3, 0, false);
            AGG_STEPC(4, 0, false); AGG_STEPC(5, 0, false); AGG_STEPC(6, 0, false); AGG_STEPC(7, 0, false);
            j += AGG_PF;
            // The bulk loads of the block that is never used are still in flight: wait for them and only THEN let their
            // destination registers die -- otherwise the compiler reuses those registers for the values of the
            // steps above and the late-landing loads overwrite them (found as one wrong entry per row segment).
            asm volatile("s_waitcnt vmcnt(0)" ::"v"(nR0), "v"(nR1), "v"(nR2), "v"(nL0), "v"(nL1), "v"(nL2) : "memory");
#undef AGG_BULK_ISSUE
#undef AGG_BULK_TAKE
#undef AGG_BULK_NEXT
#undef AGG_STEPC
        }
    } else {
    V pf[AGG_PF];
    uint32_t pr[AGG_PF];
// data load of one entry (VPL floats per lane) into a prefetch slot
#define AGG_LDV(DST, PTR)                                                                                         \
    do {                                                                                                          \
        if constexpr (VPL == 2) asm volatile("global_load_dwordx2 %0, %1, off" ADC_VOL_NT_STR : "=v"(DST) : "v"(PTR) : "memory");  \
        else asm volatile("global_load_dword %0, %1, off" ADC_VOL_NT_STR : "=v"(DST) : "v"(PTR) : "memory");                     \
    } while (0)
    // The asm-prefetch loop needs every refill index valid without clamping: j + 2*AGG_PF <= hi.
    if (j + 2 * AGG_PF <= hi) {
        const float* spn = sp + (long long)j * fstep;       // next entry to prefetch
        const uint32_t* rpn = rp + (j - L);                 // record of the output that entry triggers (>= m0)
#pragma unroll
        for (int u = 0; u < AGG_PF; u++) {
            AGG_LDV(pf[u], spn);
            asm volatile("global_load_dword %0, %1, off" : "=v"(pr[u]) : "v"(rpn) : "memory");
            spn += fstep;
            rpn += 1;
        }
// one steady-state step; WAITN = number of VMEM ops younger than slot U's two loads that may stay in flight
#define AGG_STEP(U, WAITN)                                                                                       \
    do {                                                                                                         \
        V v_;                                                                                                    \
        uint32_t rr_;                                                                                            \
        /* wait and read the landed registers in ONE statement: a separate "+v" wait lets hipcc copy the      */ \
        /* (not yet landed) registers ABOVE the wait (tied-operand copies), i.e. read garbage                 */ \
        if constexpr (VPL == 2)                                                                                  \
            asm volatile("s_waitcnt vmcnt(%4)\n\tv_mov_b64 %0, %2\n\tv_mov_b32 %1, %3"                          \
                         : "=&v"(v_), "=&v"(rr_) : "v"(pf[U]), "v"(pr[U]), "n"(WAITN) : "memory");               \
        else                                                                                                     \
            asm volatile("s_waitcnt vmcnt(%4)\n\tv_mov_b32 %0, %2\n\tv_mov_b32 %1, %3"                          \
                         : "=&v"(v_), "=&v"(rr_) : "v"(pf[U]), "v"(pr[U]), "n"(WAITN) : "memory");               \
        AGG_LDV(pf[U], spn);                                                                                     \
        asm volatile("global_load_dword %0, %1, off" : "=v"(pr[U]) : "v"(rpn) : "memory");                       \
        spn += fstep;                                                                                            \
        rpn += 1;                                                                                                \
        AGG_PUSH(v_);                                                                                            \
        AGG_EMIT(j + (U)-L, rr_); /* exactly one compiler-issued VMEM op (the store) */                          \
    } while (0)
        // first iteration: the younger ops are the prologue loads of slots U+1.. (2 each) and the U steps
        // already done (3 each): 2*(AGG_PF-1-U) + 3*U = 2*AGG_PF - 2 + U
        static_assert(AGG_PF == 8, "the peeled first iteration below is written for AGG_PF == 8");
        // (PAIR, SPARSE: a step may issue no store at all, so only the loads are counted -- a lower bound is always safe)
        constexpr bool NOST = PAIR || SPARSE;
        AGG_STEP(0, 14); AGG_STEP(1, NOST ? 14 : 15); AGG_STEP(2, NOST ? 14 : 16); AGG_STEP(3, NOST ? 14 : 17);
        AGG_STEP(4, NOST ? 14 : 18); AGG_STEP(5, NOST ? 14 : 19); AGG_STEP(6, NOST ? 14 : 20); AGG_STEP(7, NOST ? 14 : 21);
        j += AGG_PF;
        // steady state: younger ops = this slot's own store + 3 per younger step = 3*(AGG_PF-1)+1; we wait for
        // <= 3*(AGG_PF-1) outstanding (one stricter).  vmcnt retires in order (loads and stores) on gfx9-family.
        for (; j + 2 * AGG_PF <= hi; j += AGG_PF) {
#pragma unroll
            for (int u = 0; u < AGG_PF; u++) AGG_STEP(u, NOST ? 2 * (AGG_PF - 1) : 3 * (AGG_PF - 1));
        }
#undef AGG_STEP
        // the AGG_PF entries still in flight are entries j .. j+AGG_PF-1 (all < hi)
        // drain: the AGG_PF entries still in flight are entries j .. j+AGG_PF-1 (all < hi); read them inside the
        // same statement as the wait (see AGG_STEP)
        V df[AGG_PF];
        uint32_t dr[AGG_PF];
#define AGG_DRAIN(MOVD)                                                                                                        \
        asm volatile("s_waitcnt vmcnt(0)\n\t"                                                                                   \
                     MOVD " %0, %16\n\t" MOVD " %1, %17\n\t" MOVD " %2, %18\n\t" MOVD " %3, %19\n\t"                            \
                     MOVD " %4, %20\n\t" MOVD " %5, %21\n\t" MOVD " %6, %22\n\t" MOVD " %7, %23\n\t"                            \
                     "v_mov_b32 %8, %24\n\tv_mov_b32 %9, %25\n\tv_mov_b32 %10, %26\n\tv_mov_b32 %11, %27\n\t"                   \
                     "v_mov_b32 %12, %28\n\tv_mov_b32 %13, %29\n\tv_mov_b32 %14, %30\n\tv_mov_b32 %15, %31"                      \
                     : "=&v"(df[0]), "=&v"(df[1]), "=&v"(df[2]), "=&v"(df[3]), "=&v"(df[4]), "=&v"(df[5]), "=&v"(df[6]), "=&v"(df[7]), \
                       "=&v"(dr[0]), "=&v"(dr[1]), "=&v"(dr[2]), "=&v"(dr[3]), "=&v"(dr[4]), "=&v"(dr[5]), "=&v"(dr[6]), "=&v"(dr[7])  \
                     : "v"(pf[0]), "v"(pf[1]), "v"(pf[2]), "v"(pf[3]), "v"(pf[4]), "v"(pf[5]), "v"(pf[6]), "v"(pf[7]),         \
                       "v"(pr[0]), "v"(pr[1]), "v"(pr[2]), "v"(pr[3]), "v"(pr[4]), "v"(pr[5]), "v"(pr[6]), "v"(pr[7])          \
                     : "memory")
        if constexpr (VPL == 2) AGG_DRAIN("v_mov_b64");
        else AGG_DRAIN("v_mov_b32");
#undef AGG_DRAIN
#pragma unroll
        for (int u = 0; u < AGG_PF; u++) {
            AGG_PUSH(df[u]);
            AGG_EMIT(j + u - L, dr[u]);
        }
        j += AGG_PF;
    }
    }
    // ---- tail of phase B (< 2*AGG_PF entries): plain compiler-scheduled loads
    for (; j < hi; j++) {
        V v;
        if constexpr (COSTIN) {
            const uint4 rn = rrow[j], ln = lrow[j];
            AGG_COST(rn.x, rn.y, rn.z, ln.x, ln.y, ln.z, v);
        } else {
            v = *reinterpret_cast<const V*>(sp + (long long)j * fstep);
        }
        AGG_PUSH(v);
        const int m = j - L;
        if (m >= m0) AGG_EMIT(m, rp[m]);
    }
    // ---- phase C: outputs whose +L look-ahead ends beyond the last entry (image end)
    for (int m = adc_imax(m0, hi - L); m < m1; m++) AGG_EMIT(m, rp[m]);
    // ---- second pass: outputs whose look-ahead ends beyond the last first-pass output (image end)
    if constexpr (PAIR) {
        for (int s = adc_imax(s0, mcur - L); s < s1; s++) AGG_EMIT2();
    }
#undef AGG_LDV
#undef AGG_EMIT2
#undef AGG_OUT
#undef AGG_PUSH
#undef AGG_EMIT
#undef AGG_COST
}

template <bool VERT, bool DIVIDE, bool SMALL, bool COSTIN, bool PAIR, int VPL = 1, bool SPARSE = false>
__global__ __launch_bounds__(64) void k_agg_march(const float* __restrict__ src, float* __restrict__ dst,
                                                  const uint32_t* __restrict__ rec, int W, int H, int Dp, int L, int seg_len,
                                                  int nseg, int per_xcd, const int* __restrict__ armmax, int small_variant,
                                                  int small_L, AggCostIn ci)
{
    agg_march_body<VERT, DIVIDE, SMALL, COSTIN, PAIR, VPL, false, SPARSE>(src, dst, rec, W, H, Dp, L, seg_len, nseg, per_xcd, armmax,
                                                                          small_variant, small_L, ci);
}

// Behind a sparse launch: the outputs it stored (into the OTHER volume, at their own index -- the waves of neighbouring
// segments read each other's halos, so the launch itself must not write the volume it reads) go back into the volume the launch
// read, which then holds the whole result.  A wave takes 64 consecutive records of the direction's line-major record set (one
// coalesced load), and copies the Dp floats of every pixel whose record passes the launch's own predicate.  Runs after every
// kernel of the launch (stream order) with the same assumption gate, so it moves nothing when the launch was skipped.
template <bool VERT>
__global__ __launch_bounds__(256) void k_agg_apply(const float* __restrict__ from, float* __restrict__ to,
                                                   const uint32_t* __restrict__ rec, int W, int H, int Dp, int divide,
                                                   const int* __restrict__ armmax, int small_variant, int small_L)
{
    if (agg_gate_skip(armmax, small_variant, small_L, VERT)) return;
    const int lane = threadIdx.x & 63;
    const long long P = (long long)W * H;
    const long long i = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + lane; // record index: y * W + x, or x * H + y
    const bool take = i < P && adc_rec_changes_pixel(rec[i < P ? i : 0], divide != 0);
    unsigned long long todo = __ballot(take);
    const long long i0 = i - lane;
    while (todo) {
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const long long r = i0 + b;
        const long long pix = VERT ? (r % H) * W + r / H : r;
        const float* f = from + pix * Dp;
        float* t = to + pix * Dp;
        for (int d = lane; d < Dp; d += 64) t[d] = f[d];
    }
}

// GATHER form of a sparse small-ring launch (runs in place of k_agg_march<.., SPARSE>, with k_agg_apply behind it as before): the
// launch computes ONLY the pixels it stores.  Same walk as k_agg_apply -- a wave takes 64 consecutive records of the direction's
// line-major record set, ballots the launch's predicate and loops over the set bits -- and for every changed pixel the arithmetic
// of k_agg_gather.h on the input vectors of its span (a pair: of the spans of its span's pixels), which it reads from src (L2 serves
// the re-reads of neighbouring changed pixels: no streaming hint).  A lane holds the two disparities it holds in the VPL = 2 march.
// The records of a pixel's neighbours are wave-uniform: one load of the 64 records around it, picked with v_readlane (arms beyond
// the window -- never with the small ring -- fall back to a load of their own).  No ring and no depth: the arithmetic holds for
// any arm length, but the launch keeps the gate of the march it replaces -- in the short-arm plan the vertical pair launches are
// the only kernels that verify the ASSUMED vertical depth (the fused-cost pass, the horizontal pair and k_scanline_seg_agg are all
// horizontal), so it skips, and raises armmax[3], exactly when the march would.  Stores go to the OTHER volume: neighbours read src.
template <bool VERT, bool DIVIDE, bool PAIR>
__global__ __launch_bounds__(256) void k_agg_gather(const float* __restrict__ src, float* __restrict__ dst,
                                                    const uint32_t* __restrict__ rec, int W, int H, int Dp,
                                                    const int* __restrict__ armmax, int small_variant, int small_L)
{
    static_assert(!PAIR || DIVIDE, "a pair = dividing pass + the following non-dividing pass");
    if (agg_gate_skip(armmax, small_variant, small_L, VERT)) return;
    typedef AggT<2>::V V;
    const int lane = threadIdx.x & 63;
    const long long P = (long long)W * H;
    // (the wave's number through readfirstlane: everything per pixel below is then scalar work -- indices, records, loop bounds)
    const long long i0 = ((long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * 64;
    const long long i = i0 + lane; // record index: y * W + x, or x * H + y
    const uint32_t mine = rec[i < P ? i : 0];
    unsigned long long todo = __ballot(i < P && adc_rec_changes_pixel(mine, DIVIDE || PAIR));
    const long long fstep = (VERT ? (long long)W : 1LL) * Dp; // floats between neighbouring elements of a line
    while (todo) {
        const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        todo &= todo - 1;
        const long long r = i0 + b;
        const int N = VERT ? H : W;
        const long long line = r / N;
        const int s = (int)(r - line * N);
        // (arms as k_build_arms makes them end at the line's ends; the clip changes no valid record and keeps every read of a
        // damaged one inside the line)
        auto clip = [&](uint32_t q, int pos) -> uint32_t {
            const uint32_t lo = adc_imin((int)(q & 255u), pos), hi = adc_imin((int)((q >> 8) & 255u), N - 1 - pos);
            return (q & 0xFFFF0000u) | (hi << 8) | lo;
        };
        const uint32_t rs = clip((uint32_t)__builtin_amdgcn_readlane((int)mine, b), s);
        uint32_t win = 0; // lane l: record of the pixel l - 32 places along the line
        if constexpr (PAIR) {
            const long long wi = r - 32 + lane;
            win = rec[wi < 0 ? 0 : (wi >= P ? P - 1 : wi)];
        }
        auto rec_at = [&](int t) -> uint32_t { // (s + t lies inside the line: t comes from the clipped span of s)
            if (t >= -32 && t < 32) return clip((uint32_t)__builtin_amdgcn_readlane((int)win, t + 32), s + t);
            return clip((uint32_t)__builtin_amdgcn_readfirstlane((int)rec[r + t]), s + t);
        };
        const long long pix = VERT ? (long long)s * W + line : r;
        const float* ps = src + pix * Dp + lane * 2;
        float* pd = dst + pix * Dp + lane * 2;
        for (int c = 0; c < Dp; c += 128)
            *reinterpret_cast<V*>(pd + c) = agg_gather_pixel<V, DIVIDE, PAIR>(ps + c, fstep, rs, rec_at);
    }
}

// full ring in registers (2L+1 <= AGG_RING_REGS): the compiler keeps to v0..v55, ring 1 owns v56..v127, ring 2 (pairs)
// v128..v199.  Body: k_aggregate_rr.h.
template <bool VERT, bool DIVIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(AGG_RING_V0))) void k_agg_regring(
    const float* __restrict__ src, float* __restrict__ dst, const uint2* __restrict__ rec, int W, int H, int Dp, int L,
    int seg_len, int nseg, int per_xcd, const int* __restrict__ armmax, int small_variant, int small_L, float* __restrict__ sink)
{
    agg_rr_body<VERT, DIVIDE, false>(src, dst, rec, W, H, Dp, L, seg_len, nseg, per_xcd, armmax, small_variant, small_L, sink);
}
// pass pair on two register rings: dividing pass + the next iteration's first pass
template <bool VERT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(AGG_RING_V0))) void k_agg_regring_pair(
    const float* __restrict__ src, float* __restrict__ dst, const uint2* __restrict__ rec, int W, int H, int Dp, int L,
    int seg_len, int nseg, int per_xcd, const int* __restrict__ armmax, int small_variant, int small_L, float* __restrict__ sink)
{
    agg_rr_body<VERT, true, true>(src, dst, rec, W, H, Dp, L, seg_len, nseg, per_xcd, armmax, small_variant, small_L, sink);
}

// the same for the first pass of the pipeline (fused matching cost; its two tables stay in LDS)
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(AGG_RING_V0))) void k_agg_regring_cost(
    const float* __restrict__ src, float* __restrict__ dst, const uint32_t* __restrict__ rec, int W, int H, int Dp, int L,
    int seg_len, int nseg, int per_xcd, const int* __restrict__ armmax, int small_variant, int small_L, AggCostIn ci)
{
    agg_march_body<false, false, false, true, false, 1, true>(src, dst, rec, W, H, Dp, L, seg_len, nseg, per_xcd, armmax,
                                                               small_variant, small_L, ci);
}

// third generation (k_aggregate_rr2.h): two disparities per lane, ring slots = VGPR pairs v96..v239, packed adds; a wave =
// one chunk of the flattened (line-major) output index space
template <bool VERT, bool DIVIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(RR2_V0))) void k_agg_rr2(
    const float* __restrict__ src, float* __restrict__ dst, const uint2* __restrict__ rec, int W, int H, int Dp, int L,
    int chunk_len, int nwaves, int per_xcd, const int* __restrict__ armmax, int small_variant, int small_L)
{
    const AggCostIn none = {};
    agg_rr2_body<VERT, DIVIDE, false>(src, dst, rec, W, H, Dp, L, chunk_len, nwaves, per_xcd, armmax, small_variant, small_L, none);
}
// first pass of the pipeline on the same body: the matching cost is computed in registers (two lane windows)
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(RR2_V0))) void k_agg_rr2_cost(
    float* __restrict__ dst, const uint2* __restrict__ rec, int W, int H, int Dp, int L, int chunk_len, int nwaves, int per_xcd,
    const int* __restrict__ armmax, int small_variant, int small_L, AggCostIn ci)
{
    agg_rr2_body<false, false, true>(nullptr, dst, rec, W, H, Dp, L, chunk_len, nwaves, per_xcd, armmax, small_variant, small_L, ci);
}

// ------------------------------------------------------------------------------------------ host: plan (agg_plan.h), then launch
static_assert(AGG_PLAN_RING_REGS == AGG_RING_REGS && AGG_PLAN_RR2_SLOTS == RR2_SLOTS, "agg_plan.h plans for the rings of these kernels");

static int env_int(const char* name, int dflt)
{
    const char* s = getenv(name);
    return s ? atoi(s) : dflt;
}
static double env_double(const char* name, double dflt)
{
    const char* s = getenv(name);
    return s ? atof(s) : dflt;
}
// density thresholds (agg_plan.h) with their overrides, read per call: the sweeps and the tests vary them
double adc_agg_sparse_density(void) { return env_double("ADC_AGG_SPARSE_DENSITY", AGG_SPARSE_MAX_DENSITY); }
double adc_agg_gather_density(void) { return env_double("ADC_AGG_GATHER_DENSITY", AGG_GATHER_MAX_DENSITY); }
double adc_cost_flat_density(void) { return env_double("ADC_COST_FLAT_DENSITY", COST_FLAT_MAX_DENSITY); }

// The switches of the plan: the first group is latched by the first call of the process, the second read on every call.
static AggKnobs agg_knobs()
{
    static const AggKnobs latched = [] {
        AggKnobs k;
        k.small_L = env_int("ADC_AGG_SMALL_L", 8);
        k.vpl2 = env_int("ADC_AGG_VPL2", 1);
        k.regring = env_int("ADC_AGG_REGRING", 1) != 0;
        k.rr2 = env_int("ADC_AGG_RR2", 1) != 0;
        k.pair = env_int("ADC_AGG_PAIR", 1) != 0;
        k.pair_full = env_int("ADC_AGG_PAIR_FULL", 0);
        return k;
    }();
    AggKnobs k = latched;
    k.assume_margin = env_int("ADC_AGG_ASSUME_MARGIN", 1);
    k.sparse = env_int("ADC_AGG_SPARSE", 1) != 0;
    k.sparse_density = adc_agg_sparse_density();
    k.gather = env_int("ADC_AGG_GATHER", 1) != 0;
    k.gather_density = adc_agg_gather_density();
    k.cost_flat = env_int("ADC_COST_FLAT", 1) != 0;
    k.cost_flat_density = adc_cost_flat_density();
    k.dual = env_int("ADC_AGG_DUAL", 1) != 0;
    k.seg[0] = env_int("ADC_AGG_HSEG", 0);
    k.seg[1] = env_int("ADC_AGG_VSEG", 0);
    k.chunk[0] = env_int("ADC_AGG_HCHUNK", 0);
    k.chunk[1] = env_int("ADC_AGG_VCHUNK", 0);
    return k;
}

static_assert(AGG_ARMS_ASSUMED == LEARN_ARMS_ASSUMED && AGG_ARMS_FULL == LEARN_ARMS_FULL, "learn_plan.h names AggArms values");
// what the handle knows, by value (the aggregation only READS the handle's arm and density state)
static AggInputs agg_inputs(const adc_handle* h, const AggKnobs& kn, int iterations, AggArms arms, bool redo, bool fuse_cost, bool fuse_agg_so)
{
    AggInputs in = {};
    in.W = h->p.W; in.H = h->p.H; in.Dp = h->p.Dp; in.cross_L1 = h->p.opt.cross_L1; in.iterations = iterations;
    in.arms = arms;
    const AdcLearned& L = h->learned;
    for (int c = 0; c < 2; c++) { in.armmax[c] = L.armmax_host[c]; in.armmax_small[c] = L.armmax_small[c]; in.rec_nz[c] = L.rec_nz[c]; }
    in.rec_nz_known = L.rec_nz_known != 0;
    in.in_redo = redo;
    in.dual = L.agg_dual > 0;
    in.fuse_cost = fuse_cost;
    in.fuse_agg_so = fuse_agg_so;
    in.so_can_fuse = adc_so_can_fuse_agg(h);
    in.cost_flat_fits = adc_cost_agg_flat_fits(h, agg_assumed_depth(in, kn, false));
    return in;
}

// arm length up to which the small-ring variant is used (ADC_AGG_SMALL_L, 0 disables it)
int adc_agg_small_L(const adc_handle* h)
{
    AggInputs in = {};
    in.cross_L1 = h->p.opt.cross_L1;
    return agg_small_L(in, agg_knobs());
}

#define AGG_SEG_ARGS p.W, p.H, p.Dp, l.depth, l.seg_len, l.nseg, l.per_xcd, h->armmax, l.small_variant, l.small_L
#define AGG_CHUNK_ARGS p.W, p.H, p.Dp, l.depth, l.chunk_len, l.nwaves, l.per_xcd, h->armmax, l.small_variant, l.small_L
// One launch of a plan (+ k_agg_apply behind a sparse one: the result is then in src, not in dst).
template <bool VERT, bool DIVIDE, bool COSTIN, bool PAIR>
static hipError_t launch_form(adc_handle* h, const AggLaunch& l, const float* src, float* dst)
{
    const AdcParams& p = h->p;
    const dim3 grid(l.grid), block(l.block);
    const uint32_t* rec = VERT ? h->rec_v : h->rec_h;
    const uint2* rec2 = reinterpret_cast<const uint2*>(VERT ? h->rec2_v : h->rec2_h);
    AggCostIn ci;
    ci.rrec = reinterpret_cast<const uint4*>(h->cost_rrec);
    ci.lrec = reinterpret_cast<const uint4*>(h->cost_lrec);
    ci.lut_ad = h->lut_ad;
    ci.lut_census = h->lut_census;
    ci.rpitch = h->rrec_pitch; ci.padl = h->rrec_padl; ci.dmin = p.dmin; ci.D = p.D;
    switch (l.form) {
    case AGG_RR2_COST:
        if constexpr (COSTIN) hipLaunchKernelGGL(k_agg_rr2_cost, grid, block, l.lds, h->heavy, dst, rec2, AGG_CHUNK_ARGS, ci);
        break;
    case AGG_RR2:
        if constexpr (!COSTIN && !PAIR) hipLaunchKernelGGL((k_agg_rr2<VERT, DIVIDE>), grid, block, l.lds, h->heavy, src, dst, rec2, AGG_CHUNK_ARGS);
        break;
    case AGG_REGRING_COST:
        if constexpr (COSTIN) hipLaunchKernelGGL(k_agg_regring_cost, grid, block, l.lds, h->heavy, src, dst, rec, AGG_SEG_ARGS, ci);
        break;
    case AGG_REGRING_PAIR:
        if constexpr (!COSTIN && PAIR) hipLaunchKernelGGL((k_agg_regring_pair<VERT>), grid, block, l.lds, h->heavy, src, dst, rec2, AGG_SEG_ARGS, h->agg_sink);
        break;
    case AGG_REGRING:
        if constexpr (!COSTIN && !PAIR) hipLaunchKernelGGL((k_agg_regring<VERT, DIVIDE>), grid, block, l.lds, h->heavy, src, dst, rec2, AGG_SEG_ARGS, h->agg_sink);
        break;
    case AGG_GATHER:
        if constexpr (!COSTIN)
            hipLaunchKernelGGL((k_agg_gather<VERT, DIVIDE, PAIR>), grid, block, l.lds, h->heavy, src, dst, rec, p.W, p.H, p.Dp, h->armmax, l.small_variant, l.small_L);
        break;
    case AGG_MARCH_SPARSE:
        if constexpr (!COSTIN) hipLaunchKernelGGL((k_agg_march<VERT, DIVIDE, true, false, PAIR, 2, true>), grid, block, l.lds, h->heavy, src, dst, rec, AGG_SEG_ARGS, ci);
        break;
    case AGG_MARCH_SMALL2:
        if constexpr (!COSTIN) hipLaunchKernelGGL((k_agg_march<VERT, DIVIDE, true, false, PAIR, 2>), grid, block, l.lds, h->heavy, src, dst, rec, AGG_SEG_ARGS, ci);
        break;
    case AGG_COST_FLAT: return adc_launch_cost_agg_flat(h, dst, l.depth, l.small_variant, l.small_L); // (one launch for one launch, same gate)
    case AGG_MARCH_SMALL: hipLaunchKernelGGL((k_agg_march<VERT, DIVIDE, true, COSTIN, PAIR>), grid, block, l.lds, h->heavy, src, dst, rec, AGG_SEG_ARGS, ci); break;
    case AGG_MARCH_FULL: hipLaunchKernelGGL((k_agg_march<VERT, DIVIDE, false, COSTIN, PAIR>), grid, block, l.lds, h->heavy, src, dst, rec, AGG_SEG_ARGS, ci); break;
    default: return hipErrorInvalidValue;
    }
    if constexpr (!COSTIN)
        if (l.apply)
            hipLaunchKernelGGL((k_agg_apply<VERT>), dim3((unsigned)(((long long)p.W * p.H + 255) / 256)), dim3(256), 0, h->heavy, dst, const_cast<float*>(src), rec,
                               p.W, p.H, p.Dp, (DIVIDE || PAIR) ? 1 : 0, h->armmax, l.small_variant, l.small_L);
    return hipSuccess;
}
#undef AGG_SEG_ARGS
#undef AGG_CHUNK_ARGS

// the pass kinds a plan holds: fused first pass | first passes H, V | dividing passes V, H, each single or as a pair
static hipError_t launch_one(adc_handle* h, const AggLaunch& l, float* const vol[2])
{
    const float* src = vol[l.src];
    float* dst = vol[l.dst];
    switch ((l.vert ? 8 : 0) | (l.divide ? 4 : 0) | (l.costin ? 2 : 0) | (l.pair ? 1 : 0)) {
    case 2: return launch_form<false, false, true, false>(h, l, src, dst);
    case 0: return launch_form<false, false, false, false>(h, l, src, dst);
    case 8: return launch_form<true, false, false, false>(h, l, src, dst);
    case 12: return launch_form<true, true, false, false>(h, l, src, dst); // / sup_h
    case 13: return launch_form<true, true, false, true>(h, l, src, dst);
    case 4: return launch_form<false, true, false, false>(h, l, src, dst); // / sup_v
    case 5: return launch_form<false, true, false, true>(h, l, src, dst);
    default: return hipErrorInvalidValue;
    }
}

// Walks a plan.  marks: record the profiling events (only the ones adc_wait reads: start of the first / first regular launch
// step, end) and the launch statistics of this plan.
static hipError_t agg_execute(adc_handle* h, const AggPlan& plan, float* const vol[2], bool marks)
{
    const bool prof = marks && h->profiling;
    const size_t n = plan.launch.size();
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < n && e == hipSuccess; i++) {
        const AggLaunch& l = plan.launch[i];
        const bool first = i == 0 || plan.launch[i - 1].step != l.step, last = i + 1 == n || plan.launch[i + 1].step != l.step;
        if (prof && first && l.step < 2) hipEventRecord(h->ev_agg[l.step], h->heavy);
        e = launch_one(h, l, vol);
        if (l.label) h->agg_kernel = l.label; // (two launches per pass, debug surface: the label is then the last one)
        if (e == hipSuccess && last) e = hipGetLastError();
    }
    if (prof) hipEventRecord(h->ev_agg[adc_imin(plan.steps, 8)], h->heavy);
    if (marks) {
        h->agg_first_fused = plan.first_fused ? 1 : 0;
        h->agg_launches = adc_imin(plan.steps, 8);
        h->agg_passes = plan.passes;
    }
    h->agg_sparse_launches += plan.sparse;
    h->agg_gather_launches += plan.gather;
    h->agg_flat_launches += plan.flat;
    if (plan.sparse) h->agg_sparse_last = 1;
    return e;
}

// vol_a -> (H,V | V,H alternating) -> vol_a.  Every iteration is two launches: a -> b -> a.
//   fuse_cost    the first pass computes the matching cost itself (k_agg_march<.., COSTIN>: vol_a holds nothing yet)
//   fuse_agg_so  the last pass may move into the first scanline pass (fly.so_agg_fused)
//   arms, redo   what the caller knows about the arm maxima of this image (AggArms, agg_plan.h); adc_wait is redoing the Match
hipError_t adc_launch_aggregate(adc_handle* h, int iterations, AggArms arms, bool redo, bool fuse_cost, bool fuse_agg_so)
{
    if ((h->paper & ADC_PAPER_RIGHT_ARMS) && h->arms_r) return adc_paper_aggregate(h, iterations); // opt-in paper mode (k_paper.hip)
    {   // allow > 64 KiB dynamic LDS for the ring (large cross_L1): a per-DEVICE function attribute -- set once for every
        // device this process drives (a farm on device 1 after one on device 0), under a lock (handles on several threads)
        static std::mutex attr_mu;
        static bool attr_set[64] = {false};
        std::lock_guard<std::mutex> lk(attr_mu);
        const int dv = (h->device >= 0 && h->device < 64) ? h->device : 0;
        if (!attr_set[dv]) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agg_march<false, false, false, false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agg_march<false, false, false, true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agg_march<false, true, false, false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agg_march<true, false, false, false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agg_march<true, true, false, false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agg_march<true, true, false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agg_march<false, true, false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            attr_set[dv] = true;
        }
    }
    h->agg_first_fused = 0;
    h->agg_dual_last = 0;
    h->agg_sparse_last = 0;
    h->fly.so_agg_fused = 0; // (a new plan; a Match that failed between this stage and the scanline stage went through abort_match, whose one reset of fly covers it)
    const AggKnobs kn = agg_knobs();
    const AggInputs in = agg_inputs(h, kn, iterations, arms, redo, fuse_cost, fuse_agg_so);
    float* const vol[2] = {h->vol_a, h->vol_b};
    hipError_t e = hipSuccess;
    AggPlan plan;
    if (agg_dual_wanted(in, kn)) { // two plans back to back (agg_plan.h): S with the marks, then F
        AggPlan f;
        agg_plan_dual(in, kn, &plan, &f);
        if (f.result != plan.result) return hipErrorUnknown; // (agg_plan_dual aligns them)
        e = agg_execute(h, plan, vol, true);
        if (e == hipSuccess) e = agg_execute(h, f, vol, false);
        h->agg_dual_last = 1;
        h->agg_dual_runs++;
    } else {
        plan = agg_plan(in, kn, AggGate{0, 0}, false);
        e = agg_execute(h, plan, vol, true);
    }
    if (plan.tail_moved) { h->fly.so_agg_fused = 1; h->agg_so_fusions++; }
    // the result must be in vol_a (cost_aggr_): swap the two volume pointers if it ended up in the other one
    if (e == hipSuccess && plan.result != 0) { h->vol_a = vol[1]; h->vol_b = vol[0]; }
    return e;
}

// The dividing H pass of the last iteration that adc_launch_aggregate left to the scanline stage (fly.so_agg_fused), as a launch of
// its own: what run_so falls back to when its segment plan at scanline time cannot take the pass over after all (round-5 advisor
// finding: that used to fail the Match).  Full ring: valid whatever the arms are -- agg_plan_tail reads neither the arm knowledge nor "redo".
hipError_t adc_launch_aggregate_tail(adc_handle* h)
{
    const AggKnobs kn = agg_knobs();
    AggPlan plan;
    plan.launch.push_back(agg_plan_tail(agg_inputs(h, kn, 1, AGG_ARMS_UNKNOWN, false, false, false), kn));
    float* const vol[2] = {h->vol_a, h->vol_b};
    const hipError_t e = agg_execute(h, plan, vol, false);
    if (e == hipSuccess) { h->vol_a = vol[1]; h->vol_b = vol[0]; }
    return e;
}

