// learn_plan.h -- what a handle LEARNS from one Match for the next, and every host rule that moves it.  Host-only C++ shared by the
// product and the CPU tests (tests/emul/emul_learn.cpp): no HIP header, no handle, no environment.  The caller states what the device
// reported about the Match just drained (AdcMatchReport); the functions below answer "redo it?", "what does the next one assume?",
// "which form of the median runs next?", "how long is the next voting chain?" and write what is to be remembered into AdcLearned.
// Nothing here launches or synchronises; the .hip files launch what it says.
//
// A hold of N covers the Match that set it (its redo) and the N - 1 after it; agg_dual is set BEHIND the switching Match and covers
// the N after it.  The two median holds count side by side.
#pragma once
#include <stddef.h>
#include "adc_device_fn.h" // adc_so_seg_ok, ADC_SO_WARM, ADC_SO_MAX_SEG (plain inline functions under g++)

#define LEARN_HOLD_PLAN_SWITCH 64 // Matches that enqueue both aggregation plans after consecutive images needed different ones
#define LEARN_HOLD_SO_SEAM 64     // ... that run whole scanline rows after a row segment failed its seam
#define LEARN_HOLD_MED_BAND 64    // ... that run the chained median after a speculative band seam differed
#define LEARN_HOLD_MED_COLUMN 64  // ... that run the median's bands on whole rows after a column-segment seam differed
#define LEARN_MAX_REDOS 2         // attempts of adc_wait before "redo did not clear the speculation flags"
#define LEARN_IRV_FIRST 256       // voting chain budget of a handle's first Match
#define LEARN_IRV_FLOOR 4         // ... of any Match, at least (also the budget behind an EMPTY work list: chains of <= 2 kernels)
#define LEARN_IRV_MAX (1 << 16)
#define LEARN_IRV_HISTORY 8       // the budget follows the longest chain of this many Matches
#define LEARN_ARMS_ASSUMED 2      // AGG_ARMS_ASSUMED / AGG_ARMS_FULL of agg_plan.h (k_aggregate.hip asserts the equality)
#define LEARN_ARMS_FULL 3
#define LEARN_CF_TX 128           // pixels per workgroup and LDS limit of k_cost_agg_flat (k_cost.hip asserts the equality)
#define LEARN_CF_LDS_MAX (48 * 1024)

// Everything a handle carries from one Match into the next.  All zero = a new handle (adc_create then sets irv_budget = LEARN_IRV_FIRST).
struct AdcLearned {
    int arm_known;          // armmax_host holds the maxima of the previous Match
    int armmax_host[2];     // maximum horizontal / vertical arm of the previous pair (or read back: ADC_AGG_HOST_ARMS, debug surface)
    int armmax_small[2];    // arm maxima of the last image that fitted the small rings (0 = none seen)
    long long rec_nz[2];    // pixels with a pass-changing horizontal / vertical record, previous Match (or read back: debug surface)
    int rec_nz_known;
    int agg_last_plan;      // plan the previous Match's image needed: 0 none yet, 1 small rings, 2 full ring
    int agg_dual;           // > 0: enqueue both plans and let the device choose
    int so_seg_off;         // > 0: scanline row passes run whole
    int so_seg_probe;       // a seam failed and no segmented Match has held its seams since: segments come back WITHOUT the moved tail
    int med_spec_off;       // > 0: the banded median runs in its chained form
    int med_seg_off;        // > 0: the banded median runs on whole rows
    int irv_budget;         // kernels the next Match enqueues for the voting chain
    int irv_used_hist[LEARN_IRV_HISTORY];
    unsigned irv_used_pos;
};

// The counters of the debug surface (adc_debug_counter) the rules bump
struct AdcLearnStats {
    int arm_redos, so_seam_redos, redo_partial, agg_switches; // counters 2, 4, 11, 9
    int med_spec_fails, median_fallbacks, irv_overflows;      // counters 7, 0, 1
};

// What the device reported about the Match just drained
struct AdcMatchReport {
    int armmax[2];
    int ring_shallow;       // != 0: an assumed small ring was too shallow, aggregation passes were skipped
    int seam_fails;         // scanline seams that failed
    long long rec_nz[2];
    bool rec_nz_valid;
    int so_nseg_last, med_spec_last, med_seg_last; // forms the Match ran: segments per scanline row, median bands / column segments
    bool agg_first_fused;   // the first aggregation pass computed the cost itself: a redo can restart there
    bool paper_right_arms;  // ... unless this paper mode is on
};

// ---------------------------------------------------------------------------------------------------- aggregation and scanline redo
// AggArms of the next Match: assumed from the previous one, else the full ring (valid for every image)
inline int learn_arm_assumption(const AdcLearned& L) { return L.arm_known ? LEARN_ARMS_ASSUMED : LEARN_ARMS_FULL; }

// maxima / densities read back for THIS image (commit; ADC_AGG_HOST_ARMS; debug surface)
inline void learn_take_arms(AdcLearned* L, const int armmax[2]) { L->armmax_host[0] = armmax[0]; L->armmax_host[1] = armmax[1]; }
inline void learn_take_densities(AdcLearned* L, const long long nz[2]) { L->rec_nz[0] = nz[0]; L->rec_nz[1] = nz[1]; L->rec_nz_known = 1; }
// abort_match: the densities of a Match that never finished are not this handle's
inline void learn_forget_densities(AdcLearned* L) { L->rec_nz_known = 0; }

// a scanline seam failed: whole rows for the hold, and the segments come back on their own first (adc_wait; adc_debug_run)
inline void learn_so_seam_failed(AdcLearned* L) { L->so_seg_off = LEARN_HOLD_SO_SEAM; L->so_seg_probe = 1; }

enum AdcRedo { ADC_REDO_NONE, ADC_REDO_FROM_AGGREGATION, ADC_REDO_WHOLE };
inline bool learn_redo_wanted(const AdcMatchReport& r) { return r.ring_shallow != 0 || r.seam_fails != 0; }
// Does the Match run again, and from where?  (at most LEARN_MAX_REDOS times; the report is read again behind each)
// A too-shallow ring skipped aggregation passes: the row passes and their seam check then ran on a stale volume -- a seam that failed
// THERE says nothing about this image and must not cost a hold of whole rows; the redo re-checks the seams on the real volume.
// EVERY redo runs whole rows: its volume differs from the first run's, so a seam could fail there that did not fail before.
inline AdcRedo learn_redo(AdcLearned* L, AdcLearnStats* S, const AdcMatchReport& r)
{
    if (!learn_redo_wanted(r)) return ADC_REDO_NONE;
    if (r.ring_shallow != 0) { S->arm_redos++; L->arm_known = 0; }
    else { S->so_seam_redos++; learn_so_seam_failed(L); }
    if (L->so_seg_off < 1) L->so_seg_off = 1;
    const bool partial = r.agg_first_fused && !r.paper_right_arms; // pixel records, arms and aggregation records are still in HBM
    if (partial) S->redo_partial++;
    return partial ? ADC_REDO_FROM_AGGREGATION : ADC_REDO_WHOLE;
}

// Once the flags are clear.  The maxima are taken by every call; the rest once per Match (pending: a second adc_wait without a
// Match in between must not count again).  small_L: arm length up to which the small rings are used (agg_small_L).
inline void learn_commit(AdcLearned* L, AdcLearnStats* S, const AdcMatchReport& r, bool pending, int small_L)
{
    learn_take_arms(L, r.armmax);
    L->arm_known = 1;
    if (!pending) return;
    if (r.rec_nz_valid) learn_take_densities(L, r.rec_nz);
    if (L->so_seg_off > 0) L->so_seg_off--;
    // the segments are back and this Match's seams held (a redo runs whole rows: so_nseg_last is then 1): the tail may move again
    if (L->so_seg_probe && r.so_nseg_last > 1) L->so_seg_probe = 0;
    // which plan did this image need?  Consecutive Matches that need different plans = a mixed stream: the next Matches enqueue
    // both plans and let the device choose instead of assuming and redoing
    const int plan = (r.armmax[0] <= small_L && r.armmax[1] <= small_L) ? 1 : 2;
    if (plan == 1)
        for (int c = 0; c < 2; c++) L->armmax_small[c] = r.armmax[c] > 0 ? r.armmax[c] : 1;
    if (L->agg_last_plan != 0 && plan != L->agg_last_plan) { S->agg_switches++; L->agg_dual = LEARN_HOLD_PLAN_SWITCH; }
    else if (L->agg_dual > 0) L->agg_dual--;
    L->agg_last_plan = plan;
}

// ---------------------------------------------------------------------------------------------------- median
// The fallback ladder behind a Match whose banded median reported an error word (1 hand-off time-out, 2 a speculative seam
// differed) or whose fallback was forced (test hook: 1 as if timed out, 2 as if a band seam had differed).  prev = the form that
// just ran (AS_ENQUEUED: the Match's own), err = the word it left; -> the form to run next, DONE when the map is whole.
//   column segments were on:  bands on whole rows (hold: columns) -> chained bands (hold: bands) -> single workgroup
//   no segments / forced 2:   chained bands (hold: bands) -> single workgroup
//   time-out / forced 1:      single workgroup (no inter-workgroup dependency)
enum AdcMedianForm { ADC_MED_AS_ENQUEUED, ADC_MED_BANDS_WHOLE_ROWS, ADC_MED_CHAINED, ADC_MED_SINGLE_WG, ADC_MED_DONE };
inline AdcMedianForm learn_median_next(AdcLearned* L, AdcLearnStats* S, AdcMedianForm prev, int err, int spec_last, int seg_last, int forced)
{
    if (prev == ADC_MED_AS_ENQUEUED) {
        S->median_fallbacks++;
        if (!(spec_last && (err == 2 || forced == 2) && forced != 1)) return ADC_MED_SINGLE_WG;
        S->med_spec_fails++;
        if (seg_last > 1 && forced != 2) { L->med_seg_off = LEARN_HOLD_MED_COLUMN; return ADC_MED_BANDS_WHOLE_ROWS; }
    } else if (prev == ADC_MED_SINGLE_WG || err == 0) {
        return ADC_MED_DONE;
    } else if (prev == ADC_MED_CHAINED) {
        return ADC_MED_SINGLE_WG;
    }
    L->med_spec_off = LEARN_HOLD_MED_BAND;
    return ADC_MED_CHAINED;
}
// every adc_wait: each hold counts while its own safe form ran (side by side: a handle that set both has its segments back with the bands)
inline void learn_median_commit(AdcLearned* L, int spec_last, int seg_last)
{
    if (L->med_spec_off > 0 && spec_last == 0) L->med_spec_off--;
    if (L->med_seg_off > 0 && seg_last <= 1) L->med_seg_off--;
}
inline bool learn_median_speculates(const AdcLearned& L) { return L.med_spec_off == 0; }
inline bool learn_median_whole_rows(const AdcLearned& L) { return L.med_seg_off > 0; }

// ---------------------------------------------------------------------------------------------------- voting chain budget
inline int learn_voting_budget(AdcLearned* L)
{
    if (L->irv_budget < LEARN_IRV_FLOOR) L->irv_budget = LEARN_IRV_FLOOR;
    return L->irv_budget;
}
// used = kernels the chain needed, continued = the budget was too small, fixed = ADC_IRV_BUDGET (> 0 overrides).
// The longest chain of the last Matches of the handle (the pairs of a stream differ: a budget taken from the predecessor alone
// overran on 3 of 23 structured KITTI-size pairs) + 40 % (at least 2) + 2: a surplus kernel is a 2.5 us no-op, an overrun a
// synchronous continuation (~1.5 ms).  An EMPTY work list (BEGIN, then DONE: no round whose count could vary) needs only the floor.
inline void learn_voting_commit(AdcLearned* L, AdcLearnStats* S, int used, bool continued, int fixed)
{
    if (continued) S->irv_overflows++;
    L->irv_used_hist[L->irv_used_pos++ % LEARN_IRV_HISTORY] = used;
    int longest = 0;
    for (int i = 0; i < LEARN_IRV_HISTORY; i++) longest = adc_imax(longest, L->irv_used_hist[i]);
    L->irv_budget = fixed > 0 ? fixed : (longest <= 2 ? LEARN_IRV_FLOOR : adc_imin(LEARN_IRV_MAX, longest + adc_imax(2 * longest / 5, 2) + 2));
}

// ---------------------------------------------------------------------------------------------------- geometry + learned flags
struct AdcSoEnv {
    int seg;  // ADC_SO_SEG: -1 unset, 0 / 1 segments off, N >= 2 forces N
    int warm; // ADC_SO_WARM: warm-up steps (unset: the constant of that name)
    int fast; // ADC_SO_FAST: -1 unset, 0 / 1 forces k_scanline / k_scanline_pin everywhere
};
// Verified segments a scanline row pass is cut into (1 = whole rows).  Automatic choice: enough chains for two to three waves on every
// SIMD of the chip (1080 rows -> 3 x 1080, 375 rows -> 5 x 375; three instead of two at 1080 rows: profiles/r6_ab_scanline_segments.txt)
inline int learn_so_segments(int W, int H, int VPL, bool seam_buf, const AdcLearned& L, const AdcSoEnv& env)
{
    if (VPL > 2 || L.so_seg_off || !seam_buf || env.seg == 0 || env.seg == 1) return 1;
    int n = env.seg >= 2 ? env.seg : (2048 + H / 2) / H;
    if (env.seg < 2 && n == 2 && 3 * H <= 4096) n = 3;
    if (n > ADC_SO_MAX_SEG) n = ADC_SO_MAX_SEG;
    while (n >= 2 && !adc_so_seg_ok(W, n, env.warm)) n--;
    return n >= 2 ? n : 1;
}
// lone-wave chains (fewer paths than the 1024 SIMDs of the chip) run the pinned family
inline bool learn_so_uses_pin(int npaths, int nseg, int fast_env) { return fast_env >= 0 ? fast_env != 0 : npaths * nseg < 1024; }
// Can the first row pass of the next scanline run take over the last aggregation pass?  Needs the segment form of the
// compiler-allocated family with two disparities per lane; enabled = ADC_FUSE_AGG_SO, dpp = ADC_SO_DPP.  While the probe is set the
// segments run without it: that Match tries exactly the speculation that failed.
inline bool learn_so_can_fuse_agg(int W, int H, int VPL, bool seam_buf, const AdcLearned& L, const AdcSoEnv& env, bool enabled, bool dpp, unsigned paper)
{
    if (!enabled || VPL != 2 || !dpp || paper || L.so_seg_probe) return false;
    const int nseg = learn_so_segments(W, H, VPL, seam_buf, L, env);
    return nseg > 1 && !learn_so_uses_pin(H, nseg, env.fast);
}
// LDS bytes of k_cost_agg_flat at ring depth cap (two tables + three staged record rows), and whether the geometry fits
inline size_t learn_cost_flat_lds(int Dp, int cap) { return (size_t)(768 + 64 + 3 * (LEARN_CF_TX + Dp - 1 + 2 * cap)) * 4; }
inline bool learn_cost_flat_fits(int Dp, int cap) { return Dp % 128 == 0 && cap >= 0 && learn_cost_flat_lds(Dp, cap) <= LEARN_CF_LDS_MAX; }
