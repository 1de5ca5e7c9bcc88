// emul_learn -- drives adcensus_amd/csrc/learn_plan.h (what a handle learns from one Match for the next) on the CPU, the way
// adc_wait, run_heavy, adc_median_fallback and adc_voting_finish drive it, with a stand-in for the device: the "ring too shallow" word
// comes from the gates of the launches agg_plan.h plans (agg_gate_skip, variant 2), the seam and median words from the facts given.
//   consts            the hold lengths, budget constants and the literals tests/stream_model.py needs, as key=value
//   stream            stdin: one "G key=val.." line (the handle), then one "M key=val.." line per Match (the image and what fails);
//                     prints one line per Match: redo decision, assumption, plan inputs and the state afterwards
//   grid              stdin: "W H VPL seg_off probe seg_env so_fast Dp cap" per line -> "nseg can fits"
//   random SEED N     N Matches in handles of random geometry, invariants checked against independent bookkeeping
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <map>
#include <random>
#include <sstream>
#include <string>

#include "../../adcensus_amd/csrc/agg_plan.h"
#include "../../adcensus_amd/csrc/learn_plan.h"

static_assert(AGG_ARMS_ASSUMED == LEARN_ARMS_ASSUMED && AGG_ARMS_FULL == LEARN_ARMS_FULL, "learn_plan.h names AggArms values");

struct Geometry {
    int W = 160, H = 48, VPL = 2, Dp = 128, L1 = 34;
    AdcSoEnv so = {-1, ADC_SO_WARM, -1};
    int med_spec = 2, med_nseg = 3; // ADC_MEDIAN_SPEC and the column segments median_segments() would give this width
    int irv_fixed = 0;              // ADC_IRV_BUDGET
};
struct Facts { // one image, and what the device will say about its speculations
    int am[2] = {0, 0};
    long long nz[2] = {0, 0};
    int seam = 0;    // 1: a scanline seam fails where segments run, 2: ... and the word stays set behind every redo
    int mcol = 0, mband = 0, mtime = 0; // the median: a column seam / a band seam differs, a banded form times out
    int forced = 0;  // force_median_fallback
    int used = 3;    // kernels the voting chain needs
    bool pending = true;
};
struct Outcome {
    int arms, dual, can, fits, nseg;      // the first run: AggArms, the inputs of the plan, segments per scanline row
    int redos, shallow[2], partial, stuck; // redos run, the gate(s) that raised the ring word, restarted at the aggregation, never cleared
    int redo_nseg_max;                    // most segments per row any redo ran
    int med_spec, med_seg, med_rungs, med_last; // the median as enqueued; fallback launches; the last form
    int budget, continued;
    AdcMatchReport rep;                   // the report that was committed
};

struct Handle {
    Geometry g;
    AdcLearned L = {};
    AdcLearnStats S = {};
    AggKnobs kn;
    int so_nseg_last = 1, med_spec_last = 0, med_seg_last = 1;
    bool first_fused = false;
    Handle() { L.irv_budget = LEARN_IRV_FIRST; }

    AggInputs inputs(int arms, bool in_redo) const
    { // agg_inputs of k_aggregate.hip for adc_launch_aggregate(h, 4, true, true)
        AggInputs in = {};
        in.W = g.W; in.H = g.H; in.Dp = g.Dp; in.cross_L1 = g.L1; in.iterations = 4;
        in.arms = (AggArms)arms;
        for (int c = 0; c < 2; c++) { in.armmax[c] = L.armmax_host[c]; in.armmax_small[c] = L.armmax_small[c]; in.rec_nz[c] = L.rec_nz[c]; }
        in.rec_nz_known = L.rec_nz_known != 0; in.in_redo = in_redo; in.dual = L.agg_dual > 0; in.fuse_cost = true; in.fuse_agg_so = true;
        in.so_can_fuse = learn_so_can_fuse_agg(g.W, g.H, g.VPL, true, L, g.so, true, true, 0);
        in.cost_flat_fits = learn_cost_flat_fits(g.Dp, agg_assumed_depth(in, kn, false));
        return in;
    }
    // one run of the heavy stages: -> the report adc_wait builds behind it
    AdcMatchReport run(const Facts& f, int arms, bool in_redo, int shallow[2])
    {
        const AggInputs in = inputs(arms, in_redo);
        AdcMatchReport r = {};
        shallow[0] = shallow[1] = 0;
        if (!agg_dual_wanted(in, kn)) {
            const AggPlan plan = agg_plan(in, kn, AggGate{0, 0}, false);
            first_fused = plan.first_fused;
            for (const AggLaunch& l : plan.launch)
                if (l.small_variant == 2 && f.am[l.vert ? 1 : 0] > l.small_L) shallow[l.vert ? 1 : 0] = 1;
        } else {
            first_fused = true;
        }
        so_nseg_last = learn_so_segments(g.W, g.H, g.VPL, true, L, g.so);
        r.armmax[0] = f.am[0]; r.armmax[1] = f.am[1];
        r.ring_shallow = shallow[0] | shallow[1];
        r.seam_fails = f.seam == 2 || (f.seam == 1 && so_nseg_last > 1) ? 1 : 0;
        r.rec_nz[0] = f.nz[0]; r.rec_nz[1] = f.nz[1]; r.rec_nz_valid = true;
        r.so_nseg_last = so_nseg_last; r.med_spec_last = med_spec_last; r.med_seg_last = med_seg_last;
        r.agg_first_fused = first_fused; r.paper_right_arms = false;
        return r;
    }
    int median_launch(const Facts& f, int spec)
    { // launch_median_banded: the forms it records, the error word it leaves
        const int nseg = learn_median_whole_rows(L) ? 1 : g.med_nseg;
        med_spec_last = spec;
        med_seg_last = spec ? nseg : 1;
        if (f.mtime) return 1;
        return spec && ((f.mcol && med_seg_last > 1) || f.mband) ? 2 : 0;
    }

    Outcome match(const Facts& f)
    {
        Outcome o = {};
        // run_heavy
        o.arms = learn_arm_assumption(L);
        const AggInputs in0 = inputs(o.arms, false);
        o.dual = agg_dual_wanted(in0, kn); o.can = in0.so_can_fuse; o.fits = in0.cost_flat_fits;
        AdcMatchReport rep = run(f, o.arms, false, o.shallow);
        o.nseg = so_nseg_last;
        // the tail: median as enqueued, voting chain
        o.med_spec = learn_median_speculates(L) ? g.med_spec : 0;
        int med_err = median_launch(f, o.med_spec);
        o.med_seg = med_seg_last;
        o.budget = learn_voting_budget(&L);
        // adc_wait
        for (int attempt = 0; attempt < LEARN_MAX_REDOS; attempt++) {
            const AdcRedo redo = learn_redo(&L, &S, rep);
            if (redo == ADC_REDO_NONE) break;
            o.redos++;
            o.partial += redo == ADC_REDO_FROM_AGGREGATION;
            int sh[2];
            rep = run(f, redo == ADC_REDO_FROM_AGGREGATION ? LEARN_ARMS_FULL : learn_arm_assumption(L), true, sh);
            o.redo_nseg_max = std::max(o.redo_nseg_max, so_nseg_last);
            med_err = median_launch(f, learn_median_speculates(L) ? g.med_spec : 0);
        }
        o.stuck = learn_redo_wanted(rep);
        rep.med_spec_last = med_spec_last; rep.med_seg_last = med_seg_last;
        o.rep = rep;
        if (o.stuck) return o; // (adc_wait: error, abort_match)
        learn_commit(&L, &S, rep, f.pending, agg_small_L(in0, kn));
        o.continued = f.used > o.budget;
        learn_voting_commit(&L, &S, f.used, o.continued != 0, g.irv_fixed);
        if (med_err != 0 || f.forced) { // adc_median_fallback
            AdcMedianForm form = ADC_MED_AS_ENQUEUED;
            for (;;) {
                form = learn_median_next(&L, &S, form, med_err, med_spec_last, med_seg_last, f.forced);
                if (form == ADC_MED_DONE) break;
                o.med_rungs++;
                o.med_last = form;
                if (form == ADC_MED_SINGLE_WG) continue;
                med_err = median_launch(f, form == ADC_MED_BANDS_WHOLE_ROWS ? med_spec_last : 0);
            }
        }
        learn_median_commit(&L, med_spec_last, med_seg_last);
        return o;
    }
};

static std::string show(const AdcLearned& L, const AdcLearnStats& S)
{
    char buf[1024];
    int n = snprintf(buf, sizeof buf, "arm_known=%d ah=%d av=%d sh=%d sv=%d nzk=%d nzh=%lld nzv=%lld last_plan=%d agg_dual=%d so_seg_off=%d so_seg_probe=%d med_spec_off=%d "
                     "med_seg_off=%d irv_budget=%d hist=", L.arm_known, L.armmax_host[0], L.armmax_host[1], L.armmax_small[0], L.armmax_small[1], L.rec_nz_known,
                     L.rec_nz[0], L.rec_nz[1], L.agg_last_plan, L.agg_dual, L.so_seg_off, L.so_seg_probe, L.med_spec_off, L.med_seg_off, L.irv_budget);
    for (int i = 0; i < LEARN_IRV_HISTORY; i++) n += snprintf(buf + n, sizeof buf - (size_t)n, "%d,", L.irv_used_hist[i]);
    snprintf(buf + n, sizeof buf - (size_t)n, "%u | arm_redos=%d so_seam_redos=%d redo_partial=%d agg_switches=%d med_spec_fails=%d median_fallbacks=%d irv_overflows=%d",
             L.irv_used_pos, S.arm_redos, S.so_seam_redos, S.redo_partial, S.agg_switches, S.med_spec_fails, S.median_fallbacks, S.irv_overflows);
    return buf;
}

typedef std::map<std::string, std::string> KV;
static KV parse(const std::string& line)
{
    std::stringstream ss(line);
    std::string tok;
    KV kv;
    while (ss >> tok) {
        const size_t eq = tok.find('=');
        if (eq != std::string::npos) kv[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    return kv;
}
static long long num(const KV& kv, const char* k, long long dflt)
{
    const auto it = kv.find(k);
    return it == kv.end() ? dflt : atoll(it->second.c_str());
}

static int run_consts()
{
    const AggKnobs kn;
    printf("plan_switch=%d so_seam=%d med_band=%d med_column=%d max_redos=%d irv_first=%d irv_floor=%d irv_max=%d irv_history=%d so_warm=%d so_max_seg=%d "
           "cf_tx=%d cf_lds_max=%d small_L=%d assume_margin=%d\n", LEARN_HOLD_PLAN_SWITCH, LEARN_HOLD_SO_SEAM, LEARN_HOLD_MED_BAND, LEARN_HOLD_MED_COLUMN,
           LEARN_MAX_REDOS, LEARN_IRV_FIRST, LEARN_IRV_FLOOR, LEARN_IRV_MAX, LEARN_IRV_HISTORY, ADC_SO_WARM, ADC_SO_MAX_SEG, LEARN_CF_TX, LEARN_CF_LDS_MAX,
           kn.small_L, kn.assume_margin);
    return 0;
}

static int run_stream()
{
    Handle h;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.size() < 2 || line[1] != ' ') continue;
        const KV kv = parse(line.substr(2));
        if (line[0] == 'G') {
            h = Handle();
            Geometry& g = h.g;
            g.W = (int)num(kv, "W", g.W); g.H = (int)num(kv, "H", g.H); g.VPL = (int)num(kv, "VPL", g.VPL); g.Dp = 64 * g.VPL; g.L1 = (int)num(kv, "L1", g.L1);
            g.so.seg = (int)num(kv, "seg", -1); g.so.warm = (int)num(kv, "warm", ADC_SO_WARM); g.so.fast = (int)num(kv, "so_fast", -1);
            g.med_nseg = (int)num(kv, "med_nseg", g.med_nseg); g.irv_fixed = (int)num(kv, "irv_fixed", 0);
            h.kn.sparse_density = h.kn.gather_density = h.kn.cost_flat_density = (double)num(kv, "density_ppm", (long long)(AGG_SPARSE_MAX_DENSITY * 1e6 + 0.5)) * 1e-6;
            continue;
        }
        if (line[0] != 'M') continue;
        Facts f;
        f.am[0] = (int)num(kv, "ah", 0); f.am[1] = (int)num(kv, "av", 0); f.nz[0] = num(kv, "nzh", 0); f.nz[1] = num(kv, "nzv", 0);
        f.seam = (int)num(kv, "seam", 0); f.mcol = (int)num(kv, "mcol", 0); f.mband = (int)num(kv, "mband", 0); f.mtime = (int)num(kv, "mtime", 0);
        f.forced = (int)num(kv, "forced", 0); f.used = (int)num(kv, "used", 3); f.pending = num(kv, "pending", 1) != 0;
        const Outcome o = h.match(f);
        printf("arms=%d dual=%d can=%d fits=%d nseg=%d redos=%d redo_h=%d redo_v=%d partial=%d stuck=%d med_spec=%d med_seg=%d med_rungs=%d med_last=%d budget=%d "
               "continued=%d | %s\n", o.arms, o.dual, o.can, o.fits, o.nseg, o.redos, o.shallow[0], o.shallow[1], o.partial, o.stuck, o.med_spec, o.med_seg, o.med_rungs,
               o.med_last, o.budget, o.continued, show(h.L, h.S).c_str());
    }
    return 0;
}

static int run_grid()
{
    long long W, H, VPL, off, probe, seg, fast, Dp, cap;
    while (std::cin >> W >> H >> VPL >> off >> probe >> seg >> fast >> Dp >> cap) {
        AdcLearned L = {};
        L.so_seg_off = (int)off; L.so_seg_probe = (int)probe;
        const AdcSoEnv env = {(int)seg, ADC_SO_WARM, (int)fast};
        printf("%d %d %d\n", learn_so_segments((int)W, (int)H, (int)VPL, true, L, env),
               learn_so_can_fuse_agg((int)W, (int)H, (int)VPL, true, L, env, true, true, 0) ? 1 : 0, learn_cost_flat_fits((int)Dp, (int)cap) ? 1 : 0);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- invariants
static long g_bad = 0;
#define REQUIRE(cond, what) do { if (!(cond)) { if (g_bad++ < 10) printf("VIOLATION %s (handle %ld, Match %ld)\n", what, hid, i); } } while (0)

static int run_random(unsigned seed, long n)
{
    std::mt19937 rng(seed);
    auto R = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    long seams = 0, rings = 0, both_median = 0, forced = 0, short_chains = 0, long_chains = 0, switches = 0, returns = 0, done = 0;
    for (long hid = 0; done < n; hid++) {
        Handle h;
        const int geo[][3] = {{160, 48, 2}, {203, 40, 2}, {321, 37, 4}, {160, 48, 1}, {1920, 1080, 2}, {1242, 375, 2}, {640, 480, 1}};
        const int gi = R(0, 6);
        h.g.W = geo[gi][0]; h.g.H = geo[gi][1]; h.g.VPL = geo[gi][2]; h.g.Dp = 64 * h.g.VPL;
        h.g.L1 = R(0, 3) ? 34 : (R(0, 1) ? 9 : 8);
        h.g.so.fast = R(0, 2) - 1;
        h.g.med_nseg = R(0, 3) ? R(2, 6) : 1;
        const int base_nseg = learn_so_segments(h.g.W, h.g.H, h.g.VPL, true, AdcLearned{}, h.g.so);
        const int small_L = std::min(h.kn.small_L, std::max(0, std::min(h.g.L1, 255)));
        // independent bookkeeping: the first Match that speculates again, per hold; the last Match that runs two plans
        long so_back = 0, band_back = 0, col_back = 0, dual_last = -1;
        int last_plan = 0, probe = 0;
        std::deque<int> uses(LEARN_IRV_HISTORY, 0);
        const long len = R(0, 3) ? R(70, 200) : R(1, 20);
        const int calm = R(0, 2); // 0: events all the time, else mostly quiet (the holds run out)
        for (long i = 0; i < len && done < n; i++, done++) {
            Facts f;
            const bool quiet = calm && R(0, 40) != 0;
            const int cls = quiet ? 0 : R(0, 3); // short arms / medium / long
            for (int c = 0; c < 2; c++) f.am[c] = cls == 0 ? R(0, 2) : (cls < 3 ? R(0, small_L > 0 ? small_L : 1) : R(9, 34));
            for (int c = 0; c < 2; c++) f.nz[c] = (long long)h.g.W * h.g.H * R(0, 300) / 1000;
            f.seam = quiet ? 0 : (R(0, 5) == 0 ? 1 : 0);
            f.mcol = !quiet && R(0, 6) == 0; f.mband = !quiet && R(0, 6) == 0; f.mtime = !quiet && R(0, 30) == 0;
            f.forced = quiet ? 0 : (R(0, 12) == 0 ? R(1, 2) : 0);
            f.used = R(0, 4) == 0 ? R(1, 400) : R(1, 80);
            const AdcLearned before = h.L;
            const int budget_want = std::max(before.irv_budget, LEARN_IRV_FLOOR);
            const Outcome o = h.match(f);
            const AdcLearned& L = h.L;
            REQUIRE(!o.stuck, "a redo clears the flags");
            // holds: the Match that set one and the N - 1 after it run the safe form, the N-th after it speculates again
            REQUIRE((o.nseg > 1) == (base_nseg > 1 && i >= so_back), "scanline segments run exactly outside the seam hold");
            REQUIRE((o.med_spec > 0) == (i >= band_back), "the median speculates exactly outside the band hold");
            REQUIRE((o.med_seg > 1) == (o.med_spec > 0 && h.g.med_nseg > 1 && i >= col_back), "column segments run exactly outside the column hold (side by side with the band hold)");
            REQUIRE((before.agg_dual > 0) == (i <= dual_last), "two plans are wanted for exactly the hold behind a switch");
            REQUIRE(o.arms == (i == 0 ? LEARN_ARMS_FULL : LEARN_ARMS_ASSUMED), "the first Match runs the full ring, every later one assumes");
            REQUIRE(!probe || !o.can, "while the probe is set the tail never moves");
            REQUIRE(o.redos == 0 || o.redo_nseg_max == 1, "every redo runs whole rows");
            const bool ring_failed = (o.shallow[0] | o.shallow[1]) != 0, seam_failed = o.nseg > 1 && f.seam != 0;
            REQUIRE(o.redos == (ring_failed || seam_failed ? 1 : 0) && o.partial == o.redos, "one redo clears both flags (full ring, whole rows), from the aggregation on");
            rings += ring_failed; seams += seam_failed;
            // (a ring failure alone sets no hold; the seam that fails in ITS redo cannot: redos run whole rows)
            if (seam_failed && !ring_failed) { so_back = i + LEARN_HOLD_SO_SEAM; probe = 1; }
            else if (probe && o.rep.so_nseg_last > 1) probe = 0;
            REQUIRE(!(ring_failed && !before.so_seg_off) || L.so_seg_off == 0, "a ring failure never sets the seam hold");
            REQUIRE(L.so_seg_probe == probe, "the probe is set by a failed seam and cleared only by a Match that ran segments");
            REQUIRE(L.so_seg_off == (int)std::max(0L, so_back - i - 1), "so_seg_off counts the Matches left in the hold");
            // the median ladder
            const bool spec_failed = o.med_spec > 0 && f.forced != 1 && (f.forced == 2 || (!f.mtime && (f.mband || (f.mcol && o.med_seg > 1))));
            const bool col_rung = spec_failed && o.med_seg > 1 && f.forced != 2;
            const bool band_rung = spec_failed && (!col_rung || f.mband);
            if (col_rung) col_back = i + LEARN_HOLD_MED_COLUMN;
            if (band_rung) band_back = i + LEARN_HOLD_MED_BAND;
            both_median += col_rung && band_rung; forced += f.forced != 0;
            REQUIRE(L.med_seg_off == (int)std::max(0L, col_back - i - 1) && L.med_spec_off == (int)std::max(0L, band_back - i - 1), "the median holds count side by side");
            REQUIRE(o.med_rungs == 0 || o.med_last == ADC_MED_SINGLE_WG || !f.mtime, "a time-out ends in the single-workgroup kernel");
            // plan history
            const int plan = (f.am[0] <= small_L && f.am[1] <= small_L) ? 1 : 2;
            if (last_plan && plan != last_plan) { dual_last = i + LEARN_HOLD_PLAN_SWITCH; switches++; }
            last_plan = plan;
            REQUIRE(L.agg_last_plan == plan && L.agg_dual == (int)std::max(0L, dual_last - i), "agg_dual covers the N Matches after the switching one");
            REQUIRE(plan != 1 || (L.armmax_small[0] == std::max(1, f.am[0]) && L.armmax_small[1] == std::max(1, f.am[1])), "armmax_small has a floor of 1");
            REQUIRE(L.arm_known == 1 && L.armmax_host[0] == f.am[0] && L.armmax_host[1] == f.am[1] && L.rec_nz[0] == f.nz[0] && L.rec_nz_known == 1, "maxima and densities taken");
            returns += (base_nseg > 1 && i == so_back && i > 0) + (i == band_back && i > 0) + (i == col_back && i > 0);
            // voting budget: recomputed here from the last uses
            REQUIRE(o.budget == budget_want && o.continued == (f.used > o.budget), "the chain runs with the budget, floor 4, and continues when it needed more");
            uses.pop_front(); uses.push_back(f.used);
            int longest = 0;
            for (int u : uses) longest = std::max(longest, u);
            const int want = longest <= 2 ? 4 : std::min(1 << 16, longest + std::max(2 * longest / 5, 2) + 2);
            REQUIRE(L.irv_budget == want && L.irv_budget >= 4, "budget = longest of the last 8 + 40 % (at least 2) + 2, never below 4");
            short_chains += f.used <= 2; long_chains += f.used >= 300;
            // a commit without a pending Match changes nothing
            AdcLearned again = h.L;
            AdcLearnStats sagain = h.S;
            learn_commit(&again, &sagain, o.rep, false, small_L);
            REQUIRE(show(again, sagain) == show(h.L, h.S), "a commit without a pending Match changes nothing");
        }
    }
    printf("matches=%ld seam_failures=%ld shallow_rings=%ld both_median_seams=%ld forced_fallbacks=%ld chains_le2=%ld chains_ge300=%ld plan_switches=%ld "
           "holds_ended=%ld violations=%ld\n", done, seams, rings, both_median, forced, short_chains, long_chains, switches, returns, g_bad);
    return g_bad ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc >= 2 ? argv[1] : "";
    if (argc == 2 && mode == "consts") return run_consts();
    if (argc == 2 && mode == "stream") return run_stream();
    if (argc == 2 && mode == "grid") return run_grid();
    if (argc == 4 && mode == "random") return run_random((unsigned)atol(argv[2]), atol(argv[3]));
    fprintf(stderr, "usage: emul_learn consts | stream | grid | random SEED N\n");
    return 2;
}
