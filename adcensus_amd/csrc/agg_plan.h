// agg_plan.h -- what the aggregation stage (K4, k_aggregate.hip) launches, decided as plain values.  Host-only C++ shared by the
// product and the CPU tests (tests/emul/emul_agg_plan.cpp): no HIP header, no handle.  The caller states what it knows (AggInputs)
// and what the ADC_AGG_* / ADC_COST_FLAT* switches say (AggKnobs); agg_plan() returns the ordered launches of one plan, and the
// executor in k_aggregate.hip walks them.  Nothing here launches, reads the environment or keeps state.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#define AGG_PLAN_RING_REGS 72 // ring entries of the register-ring kernels (AGG_RING_REGS, k_aggregate.hip)
#define AGG_PLAN_RR2_SLOTS 72 // ... of the VGPR-pair ring (RR2_SLOTS, k_aggregate_rr2.h)

// Largest fraction of pixels with a pass-changing record (per direction, of the previous Match) up to which the small-ring
// launches of that direction run in their sparse form: half of the measured break-even density against the dense form (0.211
// on 1080p noise pairs with planted copies: tools/gpu_sparse_sweep.py, profiles/sparse_agg_density_sweep.md).
#define AGG_SPARSE_MAX_DENSITY 0.105
// Density up to which a sparse launch runs in its GATHER form (k_agg_gather: computes only the pixels it stores, from the vectors of
// their spans) instead of marching over the whole volume with the stores masked.  Rule: half of the measured break-even density
// against the sparse march.  Measured (tools/gpu_sparse_sweep.py 5 gather, profiles/gather_agg_density_sweep.md: 1080p noise pairs
// with planted copies): gather is faster at every density up to 0.30 and breaks even at 0.42, half of which (0.211) lies above the
// whole range in which the sparse march runs -- so the threshold EQUALS AGG_SPARSE_MAX_DENSITY: every sparse launch gathers.
#define AGG_GATHER_MAX_DENSITY AGG_SPARSE_MAX_DENSITY
// Density (horizontal pass-changing records of the previous Match) up to which the FIRST launch of the short-arm plan -- fused cost,
// small ring -- runs as the element-wise k_cost_agg_flat (k_cost.hip) instead of k_agg_march<.., COSTIN>.  Rule: half of the measured
// break-even density against the march, never above AGG_SPARSE_MAX_DENSITY (agg_sparse_wanted is part of the predicate).
#define COST_FLAT_MAX_DENSITY AGG_SPARSE_MAX_DENSITY

// what the host knows about the arm maxima of the image: UNKNOWN = debug surface (two launches per pass, the kernels decide),
// EXACT = read back, ASSUMED = from the previous Match of the handle (the small-ring kernels verify on the device),
// FULL = unknown in the pipeline: the full ring, valid for every image
enum AggArms { AGG_ARMS_UNKNOWN = 0, AGG_ARMS_EXACT = 1, AGG_ARMS_ASSUMED = 2, AGG_ARMS_FULL = 3 };

struct AggInputs {
    int W, H, Dp, cross_L1, iterations;
    AggArms arms;
    int armmax[2];       // maximum horizontal / vertical arm (EXACT, ASSUMED)
    int armmax_small[2]; // arm maxima of the last image that fitted the small rings (0 = none seen): depths of plan S of a two-plan run
    long long rec_nz[2]; // pixels with a pass-changing horizontal / vertical record the handle last saw
    bool rec_nz_known;
    bool in_redo;        // a Match is being redone: no sparse launches
    bool dual;           // the stream alternates between short-arm and long-arm images: enqueue two plans
    bool fuse_cost;      // the first pass computes the matching cost itself (it has no input volume)
    bool fuse_agg_so;    // the last pass may move into the first scanline pass (short-arm plan)
    bool so_can_fuse;    // ... and the scanline stage can take it (adc_so_can_fuse_agg)
    bool cost_flat_fits; // k_cost_agg_flat fits its LDS at the depth agg_assumed_depth(.., false) (adc_cost_agg_flat_fits)
};

struct AggKnobs {
    // latched once per process
    int small_L = 8;         // ADC_AGG_SMALL_L: arm length up to which the small-ring variant is used (0 disables it)
    int vpl2 = 1;            // ADC_AGG_VPL2: two disparities per lane with the small ring (1 = every launch, 2 = pass pairs only, 0 = off)
    bool regring = true;     // ADC_AGG_REGRING: full ring of a plain pass in registers when it fits (0: LDS ring)
    bool rr2 = true;         // ADC_AGG_RR2: ... as VGPR pairs, two disparities per lane (0: the one-float register ring)
    bool pair = true;        // ADC_AGG_PAIR: a dividing pass and the next first pass share a launch
    // ADC_AGG_PAIR_FULL, pairs with the full ring: 0 (default) = never, 1 = when both rings fit into registers (k_agg_regring_pair),
    // 2 = also as two 17 KiB LDS rings per wave.  Measured on MI355X (structured 1080p pair, rocprofv3): a register-ring pair
    // launch takes 0.95-1.02 ms against 2 x 0.42 ms for two single passes -- 200 VGPRs leave 2 waves per SIMD, and this
    // kernel family runs at ~8.7 cycles per instruction and wave whatever the occupancy, so halving the waves doubles
    // the time per step while the saved HBM round trip (0.2 ms at the copy rate) does not pay for it; two LDS rings were
    // 3x slower.  The single pass itself now runs at the device copy rate.
    int pair_full = 0;
    // read on every call (the tests and the sweeps vary them within one process)
    int assume_margin = 1;   // ADC_AGG_ASSUME_MARGIN: ring entries added to ASSUMED maxima
    bool sparse = true;      // ADC_AGG_SPARSE
    double sparse_density = AGG_SPARSE_MAX_DENSITY; // ADC_AGG_SPARSE_DENSITY
    bool gather = true;      // ADC_AGG_GATHER
    double gather_density = AGG_GATHER_MAX_DENSITY; // ADC_AGG_GATHER_DENSITY
    bool cost_flat = true;   // ADC_COST_FLAT
    double cost_flat_density = COST_FLAT_MAX_DENSITY; // ADC_COST_FLAT_DENSITY
    bool dual = true;        // ADC_AGG_DUAL
    int seg[2] = {0, 0};     // ADC_AGG_HSEG / ADC_AGG_VSEG: segments per line (< 1: pick_nseg)
    int chunk[2] = {0, 0};   // ADC_AGG_HCHUNK / ADC_AGG_VCHUNK: chunk length of the VGPR-pair ring (< 1: pick_chunk)
};

// One plan of a two-plan run: the gate code (3 = plan S, 4 = plan F) and the packed depths every kernel of it receives instead of
// its own gate (agg_gate_skip, k_aggregate_rr.h).  code 0: a plan on its own.
struct AggGate { int code, thr; };

enum AggForm {
    AGG_MARCH_FULL,   // k_agg_march, LDS full ring (also with the fused cost, also as a pair)
    AGG_MARCH_SMALL,  // k_agg_march<.., SMALL>, one disparity per lane (also with the fused cost, also as a pair)
    AGG_MARCH_SMALL2, // ... two disparities per lane
    AGG_MARCH_SPARSE, // ... storing only the changed pixels
    AGG_GATHER,       // k_agg_gather: computes only the changed pixels
    AGG_REGRING,      // k_agg_regring
    AGG_REGRING_PAIR, // k_agg_regring_pair
    AGG_REGRING_COST, // k_agg_regring_cost
    AGG_RR2,          // k_agg_rr2
    AGG_RR2_COST,     // k_agg_rr2_cost
    AGG_COST_FLAT,    // k_cost_agg_flat (k_cost.hip)
    AGG_FORM_COUNT
};
// kernel family of a launch [form][pair] (the fused-cost launches carry none)
static const char* const agg_form_label[AGG_FORM_COUNT][2] = {
    {"k_agg_march (LDS full ring, one pass per launch)", "k_agg_march (LDS full ring, one pass per launch)"},
    {"k_agg_march<.., SMALL> (LDS small ring, one pass per launch)", "k_agg_march<.., PAIR> (LDS small rings: dividing pass + next first pass per launch)"},
    {"k_agg_march<.., SMALL> (LDS small ring, one pass per launch)", "k_agg_march<.., PAIR> (LDS small rings: dividing pass + next first pass per launch)"},
    {"k_agg_march<.., SMALL, SPARSE> + k_agg_apply (LDS small ring, one pass per launch, only changed pixels stored)",
     "k_agg_march<.., PAIR, SPARSE> + k_agg_apply (LDS small rings: dividing pass + next first pass per launch, only changed pixels stored)"},
    {"k_agg_gather + k_agg_apply (SPARSE launch, gather form: one pass per launch, only changed pixels computed)",
     "k_agg_gather<.., PAIR> + k_agg_apply (SPARSE launch, gather form: dividing pass + next first pass, only changed pixels computed)"},
    {"k_agg_regring (register ring, 1 disparity per lane, one pass per launch)", nullptr},
    {nullptr, "k_agg_regring_pair (two register rings, dividing pass + next first pass per launch)"},
    {nullptr, nullptr},
    {"k_agg_rr2 (register ring of VGPR pairs, 2 disparities per lane, one pass per launch)", nullptr},
    {nullptr, nullptr},
    {nullptr, nullptr},
};

struct AggLaunch {
    AggForm form;
    bool vert, divide, costin, pair;
    int step;                    // index of the pass (or pass pair) this launch belongs to: two launches share one when the kernels choose the ring
    int depth;                   // ring depth L the kernel receives
    int seg_len, nseg, per_xcd;  // the segment forms; AGG_RR2*: chunk_len, nwaves (and per_xcd)
    int chunk_len, nwaves;
    unsigned grid, block;        // (AGG_COST_FLAT: chosen by its launcher in k_cost.hip)
    size_t lds;
    int small_variant, small_L;  // the gate pair
    bool apply;                  // k_agg_apply follows (sparse forms): the result is then in src
    int src, dst;                // 0 / 1 = the volume that held the stage's input / the other one
    const char* label;
};

struct AggPlan {
    std::vector<AggLaunch> launch;
    int steps = 0, passes = 0;   // launch steps, and the algorithmic passes (2 per iteration) they cover
    bool first_fused = false;    // the first launch computes the matching cost
    bool tail_moved = false;     // the last pass is left to the scanline stage
    int result = 0;              // volume that holds the result
    int sparse = 0, gather = 0, flat = 0; // counters the run bumps
};

inline int agg_full_L(const AggInputs& in) { return std::max(0, std::min(in.cross_L1, 255)); }
inline int agg_small_L(const AggInputs& in, const AggKnobs& kn) { return std::min(kn.small_L, agg_full_L(in)); }
inline bool agg_small_ok(const AggInputs& in, const AggKnobs& kn) { return agg_small_L(in, kn) > 0 && agg_small_L(in, kn) < agg_full_L(in); }
// the first pass fits its ring and the two cost tables into LDS
inline bool agg_cost_lds_fits(const AggInputs& in) { return (size_t)(2 * agg_full_L(in) + 1) * 64 * sizeof(float) + (768 + 64) * sizeof(float) <= 150 * 1024; }

// Picks the number of line segments: all waves of a "round" run concurrently (9 per CU), a pass costs
// rounds x (segment length + halo) steps.
inline int pick_nseg(long long nlines, int N, int L, int slots)
{
    int best = 1;
    long long best_cost = -1;
    for (int ns = 1; ns <= 16; ns++) {
        const int seg = (N + ns - 1) / ns;
        if (ns > 1 && seg < 2 * L) break;
        const long long rounds = (nlines * ns + slots - 1) / slots;
        const long long cost = rounds * (seg + (ns > 1 ? 2 * L : 0));
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = ns; }
    }
    return best;
}

// Chunk length of the pair-register-ring kernels (a wave = chunk_len consecutive outputs of the line-major index space,
// k_aggregate_rr2.h).  Candidates: whole-line segmentations N / k and equal shares of the whole pass per wave slot (1x, 2x, 3x
// the slots); cost model = rounds x (steps + 2L halo entries + a fixed price per piece for its prologue / slow tail).
inline int pick_chunk(long long nlines, int N, int L, int slots)
{
    const long long total = nlines * N;
    long long best_cost = -1;
    int best = N;
    auto consider = [&](long long c) {
        if (c < 1) c = 1;
        if (c < N && c < 4 * (long long)L) return; // halo-dominated
        if (c > total) c = total;
        const long long waves = (total + c - 1) / c;
        const long long rounds = (waves + slots - 1) / slots;
        const bool aligned = c >= N ? (c % N == 0) : (N % c == 0);
        const long long pieces = aligned ? (c >= N ? c / N : 1) : (c >= N ? c / N + 2 : 2);
        const long long halo = (c < N || !aligned) ? 2LL * L : 0;
        const long long cost = rounds * (c + halo + 60 * pieces);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = (int)c; }
    };
    for (int k = 1; k <= 16; k++) consider((N + k - 1) / k);
    for (int k = 1; k <= 3; k++) consider((total + (long long)slots * k - 1) / ((long long)slots * k));
    return best;
}

// Ring depth of a small-ring launch along one direction when the host works with arm maxima: the longest arm, plus a margin when
// the maxima are ASSUMED from an earlier Match of the handle (the next image of a similar stream may have a longest arm of 3 after
// 2, and a wrong depth costs a redo or the full-ring plan).
inline int agg_assumed_depth(const AggInputs& in, const AggKnobs& kn, bool vert)
{
    const int Lknown = std::max(1, in.armmax[vert ? 1 : 0]) + (in.arms == AGG_ARMS_ASSUMED ? kn.assume_margin : 0);
    return std::min(agg_small_L(in, kn), Lknown);
}

inline bool agg_small_vpl2(const AggInputs& in, const AggKnobs& kn, bool pair)
{
    return (kn.vpl2 == 1 || (kn.vpl2 == 2 && pair)) && in.Dp % 128 == 0;
}
inline bool agg_density_within(const AggInputs& in, bool vert, double density)
{
    return (double)in.rec_nz[vert ? 1 : 0] <= density * (double)in.W * (double)in.H;
}
// Does a small-ring launch of this direction run sparse?  Only in the plain short-arm plan of the pipeline (arms read back or
// assumed, one plan enqueued, not a redo), with two disparities per lane, when the record density the handle last saw is low.
// Both forms give the same bits for every image: a wrong guess costs time, never a redo.
inline bool agg_sparse_wanted(const AggInputs& in, const AggKnobs& kn, AggGate gate, bool vert, bool pair)
{
    if (!kn.sparse || gate.code || in.in_redo || !(in.arms == AGG_ARMS_EXACT || in.arms == AGG_ARMS_ASSUMED) || !in.rec_nz_known) return false;
    return agg_small_vpl2(in, kn, pair) && agg_density_within(in, vert, kn.sparse_density);
}
// Does a sparse launch of this direction (never a first Match, a two-plan Match or a redo) gather?  Every form gives the same bits.
inline bool agg_gather_wanted(const AggInputs& in, const AggKnobs& kn, bool vert)
{
    return kn.gather && agg_density_within(in, vert, kn.gather_density);
}
// Does the first launch run flat?  Only where the horizontal small-ring launches run sparse, with the host knowing or assuming the
// arms (small ring only).  Both forms give the same bits and keep the same gate.
inline bool agg_cost_flat_wanted(const AggInputs& in, const AggKnobs& kn, AggGate gate, bool small_only)
{
    return kn.cost_flat && small_only && agg_sparse_wanted(in, kn, gate, false, false) && in.cost_flat_fits && agg_density_within(in, false, kn.cost_flat_density);
}

// full ring of a plain pass: in registers when it fits
inline bool agg_regring_fits(const AggKnobs& kn, int depth) { return kn.regring && depth >= 1 && 2 * depth + 1 <= AGG_PLAN_RING_REGS; }

// ring choice of a pass: the kernels choose (two launches: full ring, then small ring), or the host has
enum AggRing { AGG_RING_BOTH = 0, AGG_RING_SMALL = 1, AGG_RING_FULL = 2 };
struct AggPass { bool vert, divide, costin, pair, sparse; AggRing ring; int step, src, dst; };

// Which kernel form a launch takes.  small = the small-ring launch of the pass, depth = its ring depth.
inline AggForm agg_pick_form(const AggInputs& in, const AggKnobs& kn, AggGate gate, const AggPass& ps, bool small, int depth)
{
    const bool regring = !small && agg_regring_fits(kn, depth);
    if (regring && kn.rr2 && !ps.pair && in.Dp % 128 == 0 && 2 * depth + 1 <= AGG_PLAN_RR2_SLOTS) return ps.costin ? AGG_RR2_COST : AGG_RR2;
    if (regring) return ps.costin ? AGG_REGRING_COST : (ps.pair ? AGG_REGRING_PAIR : AGG_REGRING);
    if (!small) return AGG_MARCH_FULL;
    if (ps.costin) return agg_cost_flat_wanted(in, kn, gate, ps.ring == AGG_RING_SMALL) ? AGG_COST_FLAT : AGG_MARCH_SMALL;
    if (!agg_small_vpl2(in, kn, ps.pair)) return AGG_MARCH_SMALL;
    if (!ps.sparse) return AGG_MARCH_SMALL2;
    return agg_gather_wanted(in, kn, ps.vert) ? AGG_GATHER : AGG_MARCH_SPARSE;
}

// One launch of a pass: form, geometry and gate.
inline AggLaunch agg_plan_launch(const AggInputs& in, const AggKnobs& kn, AggGate gate, const AggPass& ps, bool small)
{
    AggLaunch l = {};
    const int N = ps.vert ? in.H : in.W, small_L = agg_small_L(in, kn);
    // the ring only has to be as deep as the longest arm of this direction when the host knows it
    const int Lv = !small ? agg_full_L(in) : ((ps.ring == AGG_RING_SMALL && in.arms != AGG_ARMS_UNKNOWN) ? agg_assumed_depth(in, kn, ps.vert) : small_L);
    l.form = agg_pick_form(in, kn, gate, ps, small, Lv);
    l.vert = ps.vert; l.divide = ps.divide; l.costin = ps.costin; l.pair = ps.pair;
    l.step = ps.step; l.src = ps.src; l.dst = ps.dst; l.depth = Lv;
    const bool regring = l.form == AGG_REGRING || l.form == AGG_REGRING_PAIR || l.form == AGG_REGRING_COST || l.form == AGG_RR2 || l.form == AGG_RR2_COST;
    const bool rr2 = l.form == AGG_RR2 || l.form == AGG_RR2_COST;
    const int vpl = (rr2 || l.form == AGG_MARCH_SMALL2 || l.form == AGG_MARCH_SPARSE || l.form == AGG_GATHER) ? 2 : 1;
    const long long nlines = (long long)(ps.vert ? in.W : in.H) * (in.Dp / (64 * vpl));
    // the fused-cost variant keeps the two cost tables (768 + 64 floats) behind the ring, the pair variant a second ring and a record ring
    const size_t ring_bytes = regring ? 0 : (size_t)(2 * Lv + 1) * 64 * sizeof(float) * vpl;
    const size_t ldsv = ring_bytes + (ps.costin ? (768 + 64) * sizeof(float) : 0) + ((ps.pair && !regring) ? ring_bytes + (2 * Lv + 1) * 4 + 64 : 0);
    // register rings: 128 VGPRs -> 4 waves per SIMD; a pair (two rings, 200 VGPRs) or a ring of pairs (240) -> 2
    const int waves_per_cu = regring ? ((ps.pair || rr2) ? 8 : 16) : std::max(1, std::min(32, (int)((160 * 1024) / ((ldsv + 511) / 512 * 512))));
    int nseg = kn.seg[ps.vert ? 1 : 0];
    if (nseg < 1) nseg = pick_nseg(nlines, N, ps.pair ? 2 * Lv : Lv, 256 * waves_per_cu);
    l.seg_len = std::max(1, (N + nseg - 1) / nseg);
    l.nseg = (N + l.seg_len - 1) / l.seg_len;
    l.per_xcd = (int)((nlines * l.nseg + 7) / 8);
    l.grid = (unsigned)l.per_xcd * 8; l.block = 64;
    l.lds = ldsv;
    if (rr2) {
        l.chunk_len = kn.chunk[ps.vert ? 1 : 0];
        if (l.chunk_len < 1) l.chunk_len = pick_chunk(nlines, N, Lv, 256 * waves_per_cu);
        l.nwaves = (int)((nlines * N + l.chunk_len - 1) / l.chunk_len);
        l.per_xcd = (l.nwaves + 7) / 8;
        l.grid = (unsigned)l.per_xcd * 8;
    }
    if (l.form == AGG_GATHER) { l.grid = (unsigned)(((long long)in.W * in.H + 255) / 256); l.block = 256; l.lds = 0; }
    l.apply = l.form == AGG_GATHER || l.form == AGG_MARCH_SPARSE;
    // gate: a launch of a pair the kernels choose from (0 / 1), a ring assumed from the previous Match (2, verified on the device), none
    const bool both = ps.ring == AGG_RING_BOTH && agg_small_ok(in, kn), verify = small && ps.ring == AGG_RING_SMALL && in.arms == AGG_ARMS_ASSUMED;
    l.small_variant = gate.code ? gate.code : (both ? (small ? 1 : 0) : (verify ? 2 : -1));
    l.small_L = gate.code ? gate.thr : (both ? small_L : (verify ? Lv : 0x7fffffff));
    l.label = ps.costin ? nullptr : agg_form_label[l.form][ps.pair ? 1 : 0];
    return l;
}

// The launches of one pass: full ring, then small ring when the kernels choose; else the one the host chose.
inline void agg_plan_pass(const AggInputs& in, const AggKnobs& kn, AggGate gate, const AggPass& ps, AggPlan* plan)
{
    const bool small_ok = agg_small_ok(in, kn);
    const bool full = !(ps.ring == AGG_RING_SMALL && small_ok), small = small_ok && ps.ring != AGG_RING_FULL;
    for (int v = full ? 0 : 1; v <= (small ? 1 : 0); v++) {
        const AggLaunch l = agg_plan_launch(in, kn, gate, ps, v == 1);
        plan->sparse += l.apply ? 1 : 0;
        plan->gather += l.form == AGG_GATHER ? 1 : 0;
        plan->flat += l.form == AGG_COST_FLAT ? 1 : 0;
        plan->launch.push_back(l);
    }
}

// ring of a direction: the host picks it from the arm maxima when it has them
inline AggRing agg_ring(const AggInputs& in, const AggKnobs& kn, bool vert)
{
    if (in.arms == AGG_ARMS_UNKNOWN) return AGG_RING_BOTH;
    if (in.arms == AGG_ARMS_FULL) return AGG_RING_FULL; // nothing known about this image: the full ring is valid for every image
    return (agg_small_ok(in, kn) && in.armmax[vert ? 1 : 0] <= agg_small_L(in, kn)) ? AGG_RING_SMALL : AGG_RING_FULL;
}

// The LAST pass (horizontal, dividing) of a short-arm image moves into the first scanline pass (k_scanline_seg_agg: one launch and
// 2 V of traffic less): arms up to 4, assumed or known; the other horizontal passes verify the depth.  Never in a two-plan run.
inline bool agg_tail_moves(const AggInputs& in, const AggKnobs& kn, AggGate gate)
{
    return in.iterations == 4 && in.fuse_agg_so && !gate.code && agg_ring(in, kn, false) == AGG_RING_SMALL &&
           (in.arms == AGG_ARMS_EXACT || in.arms == AGG_ARMS_ASSUMED) && agg_assumed_depth(in, kn, false) <= 4 && in.so_can_fuse;
}

// One plan of the aggregation.  Pass sequence (cross_aggregator.cpp:100-118): iteration k = [first direction][second direction,
// divided by the support count]; the direction order alternates (horizontal first, :100), so the dividing pass of iteration k and the
// first pass of iteration k+1 run along the SAME direction and can share one launch (pair) when the small ring is in use.
//   first_into_cur  the first launch writes the volume it would have READ (only with the fused cost, which has no input volume):
//                   flips which of the two volumes the plan ends in
inline AggPlan agg_plan(const AggInputs& in, const AggKnobs& kn, AggGate gate, bool first_into_cur)
{
    AggPlan plan;
    const AggRing ring[2] = {agg_ring(in, kn, false), agg_ring(in, kn, true)};
    int cur = 0;             // holds the input of the next launch
    bool second_done = false; // the first pass of this iteration was already computed by the previous pair launch
    for (int k = 0; k < in.iterations; k++) {
        const bool hf = k % 2 == 0;
        if (!second_done) { // first pass of the iteration; of the pipeline: the matching cost is computed inside the pass
            const bool fused = k == 0 && in.fuse_cost && agg_cost_lds_fits(in);
            if (k == 0) plan.first_fused = fused;
            AggPass ps = {!hf, false, fused, false, false, ring[hf ? 0 : 1], plan.steps, cur, (fused && first_into_cur) ? cur : 1 - cur};
            ps.sparse = !fused && ps.ring == AGG_RING_SMALL && agg_sparse_wanted(in, kn, gate, ps.vert, false);
            agg_plan_pass(in, kn, gate, ps, &plan);
            if (ps.dst != cur && !ps.sparse) cur = 1 - cur; // (a sparse launch leaves its result in the volume it read)
            plan.steps++;
            plan.passes++;
        }
        // second pass of the iteration (dividing): vertical after a horizontal first pass and vice versa
        const AggRing rsec = ring[hf ? 1 : 0];
        if (!hf && k + 1 == in.iterations && agg_tail_moves(in, kn, gate)) { plan.tail_moved = true; break; }
        const bool pair = kn.pair && k + 1 < in.iterations &&
                          (rsec == AGG_RING_SMALL || (rsec == AGG_RING_FULL && (kn.pair_full >= 2 || (kn.pair_full == 1 && agg_regring_fits(kn, agg_full_L(in))))));
        const bool sparse = rsec == AGG_RING_SMALL && agg_sparse_wanted(in, kn, gate, hf, pair);
        agg_plan_pass(in, kn, gate, AggPass{hf, true, false, pair, sparse, rsec, plan.steps, cur, 1 - cur}, &plan);
        if (!sparse) cur = 1 - cur;
        plan.steps++;
        plan.passes += pair ? 2 : 1;
        second_done = pair;
    }
    plan.result = cur;
    return plan;
}

// The dividing H pass of the last iteration as a launch of its own, full ring (valid whatever the arms are): volume 0 -> 1.
inline AggLaunch agg_plan_tail(const AggInputs& in, const AggKnobs& kn)
{
    return agg_plan_launch(in, kn, AggGate{0, 0}, AggPass{false, true, false, false, false, AGG_RING_FULL, 0, 0, 1}, false);
}

// Two plans (a stream that alternates between short-arm and long-arm images; pipeline only: the arm maxima are not known on the
// host): plan S = small rings of the depth the last short-arm image needed (+ margin) with pass pairs, plan F = the full ring; every
// kernel of S runs iff both directions fit the assumed depths, every kernel of F iff not (agg_gate_skip).  Needs the fused cost: its
// first pass has no input volume, so plan F can start by writing the volume it would have read when that makes both plans END in the
// same volume (S: 5 launches, F: 8).
inline bool agg_dual_wanted(const AggInputs& in, const AggKnobs& kn)
{
    return kn.dual && in.dual && in.arms >= AGG_ARMS_ASSUMED && in.fuse_cost && in.iterations >= 1 && agg_small_ok(in, kn) && agg_cost_lds_fits(in);
}
inline void agg_plan_dual(const AggInputs& in, const AggKnobs& kn, AggPlan* s, AggPlan* f)
{
    AggInputs si = in, fi = in;
    si.arms = AGG_ARMS_ASSUMED;
    for (int c = 0; c < 2; c++) si.armmax[c] = in.armmax_small[c] > 0 ? in.armmax_small[c] : agg_small_L(in, kn);
    fi.arms = AGG_ARMS_FULL;
    const int thr = agg_assumed_depth(si, kn, false) | (agg_assumed_depth(si, kn, true) << 16);
    *s = agg_plan(si, kn, AggGate{3, thr}, false);
    *f = agg_plan(fi, kn, AggGate{4, thr}, false);
    if (f->result != s->result) *f = agg_plan(fi, kn, AggGate{4, thr}, true);
}
