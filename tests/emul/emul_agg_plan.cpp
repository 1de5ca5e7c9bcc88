// CPU driver of adcensus_amd/csrc/agg_plan.h, the header the product plans its aggregation launches with (compiled here under g++,
// alone).  Test infrastructure (tests/test_emul_agg_plan.py):
//   emul_agg_plan table FILE    plans every scenario line ("S name key=val ...") of the characterisation table and prints each plan as
//                               the launches, events and end state it stands for, in the format of the table
//   emul_agg_plan random SEED N draws N random inputs / knobs and checks the invariants of a plan; prints the violations
//   emul_agg_plan one key=val.. plans ONE AggInputs (the keys of an S line; fits= states cost_flat_fits, env= the per-call switches) and prints
//                               "sparse= gather= flat= tail_moved= first_fused= dual= forms=" with the form of every launch; "one -" reads one
//                               such scenario per line of the standard input (tests/stream_model.py)
#include "../../adcensus_amd/csrc/agg_plan.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <random>
#include <sstream>
#include <string>

// the switches as the product reads them from the environment (k_aggregate.hip: agg_knobs), from "NAME=V,NAME=V"
static void apply_env(const std::string& env, AggKnobs* k)
{
    if (env == "-") return;
    std::stringstream ss(env);
    std::string kv;
    while (std::getline(ss, kv, ',')) {
        const size_t eq = kv.find('=');
        const std::string n = kv.substr(0, eq), v = kv.substr(eq + 1);
        const int i = atoi(v.c_str());
        if (n == "ADC_AGG_SMALL_L") k->small_L = i;
        else if (n == "ADC_AGG_VPL2") k->vpl2 = i;
        else if (n == "ADC_AGG_REGRING") k->regring = i != 0;
        else if (n == "ADC_AGG_RR2") k->rr2 = i != 0;
        else if (n == "ADC_AGG_PAIR") k->pair = i != 0;
        else if (n == "ADC_AGG_PAIR_FULL") k->pair_full = i;
        else if (n == "ADC_AGG_ASSUME_MARGIN") k->assume_margin = i;
        else if (n == "ADC_AGG_SPARSE") k->sparse = i != 0;
        else if (n == "ADC_AGG_SPARSE_DENSITY") k->sparse_density = atof(v.c_str());
        else if (n == "ADC_AGG_GATHER") k->gather = i != 0;
        else if (n == "ADC_AGG_GATHER_DENSITY") k->gather_density = atof(v.c_str());
        else if (n == "ADC_COST_FLAT") k->cost_flat = i != 0;
        else if (n == "ADC_COST_FLAT_DENSITY") k->cost_flat_density = atof(v.c_str());
        else if (n == "ADC_AGG_DUAL") k->dual = i != 0;
        else if (n == "ADC_AGG_HSEG") k->seg[0] = i;
        else if (n == "ADC_AGG_VSEG") k->seg[1] = i;
        else if (n == "ADC_AGG_HCHUNK") k->chunk[0] = i;
        else if (n == "ADC_AGG_VCHUNK") k->chunk[1] = i;
        else { fprintf(stderr, "unknown switch %s\n", n.c_str()); exit(2); }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the table
// A plan written out the way the launcher's launches were recorded (tests/golden/agg_plan_table.txt): one L line per kernel launch
// with the kernel's name, grid, block, LDS bytes and arguments in order, E lines for the profiling events, an R line for the state
// of the handle afterwards.  Buffers go by name; D and dmin are only passed on (AggCostIn).
struct Scen { int W, H, D, Dp, dmin, prof, valid, ah, av; };
static const char* tf(bool b) { return b ? "true" : "false"; }
static const char* vol(int v) { return v ? "volB" : "volA"; }

static void print_launch(const AggLaunch& l, const Scen& sc)
{
    char k[96], ci[64], seg[96], gate[48];
    const bool small = l.form != AGG_MARCH_FULL, two = l.form == AGG_MARCH_SMALL2 || l.form == AGG_MARCH_SPARSE;
    snprintf(ci, sizeof ci, " ci{tables %d 256 %d %d}", sc.W + 512, sc.dmin, sc.D);
    snprintf(gate, sizeof gate, "armmax %d %d", l.small_variant, l.small_L);
    const bool chunks = l.form == AGG_RR2 || l.form == AGG_RR2_COST;
    snprintf(seg, sizeof seg, "%d %d %d %d %d %d %d", sc.W, sc.H, sc.Dp, l.depth, chunks ? l.chunk_len : l.seg_len, chunks ? l.nwaves : l.nseg, l.per_xcd);
    const char* rec = l.vert ? "rec_v" : "rec_h";
    const char* rec2 = l.vert ? "rec2_v" : "rec2_h";
    if (l.form == AGG_COST_FLAT) { printf("L k_cost_agg_flat : %s %d %d %d\n", vol(l.dst), l.depth, l.small_variant, l.small_L); return; }
    switch (l.form) {
    case AGG_RR2_COST: snprintf(k, sizeof k, "k_agg_rr2_cost"); break;
    case AGG_RR2: snprintf(k, sizeof k, "k_agg_rr2<%s,%s>", tf(l.vert), tf(l.divide)); break;
    case AGG_REGRING_COST: snprintf(k, sizeof k, "k_agg_regring_cost"); break;
    case AGG_REGRING_PAIR: snprintf(k, sizeof k, "k_agg_regring_pair<%s>", tf(l.vert)); break;
    case AGG_REGRING: snprintf(k, sizeof k, "k_agg_regring<%s,%s>", tf(l.vert), tf(l.divide)); break;
    case AGG_GATHER: snprintf(k, sizeof k, "k_agg_gather<%s,%s,%s>", tf(l.vert), tf(l.divide), tf(l.pair)); break;
    default: snprintf(k, sizeof k, "k_agg_march<%s,%s,%s,%s,%s,%d,%s>", tf(l.vert), tf(l.divide), tf(small), tf(l.costin), tf(l.pair), two ? 2 : 1, tf(l.form == AGG_MARCH_SPARSE));
    }
    printf("L %s g=%u b=%u lds=%zu :", k, l.grid, l.block, l.lds);
    if (l.form == AGG_RR2_COST) printf(" %s %s %s %s%s\n", vol(l.dst), rec2, seg, gate, ci);
    else if (l.form == AGG_RR2) printf(" %s %s %s %s %s\n", vol(l.src), vol(l.dst), rec2, seg, gate);
    else if (l.form == AGG_REGRING_COST) printf(" %s %s %s %s %s%s\n", vol(l.src), vol(l.dst), rec, seg, gate, ci);
    else if (l.form == AGG_REGRING_PAIR || l.form == AGG_REGRING) printf(" %s %s %s %s %s sink\n", vol(l.src), vol(l.dst), rec2, seg, gate);
    else if (l.form == AGG_GATHER) printf(" %s %s %s %d %d %d %s\n", vol(l.src), vol(l.dst), rec, sc.W, sc.H, sc.Dp, gate);
    else printf(" %s %s %s %s %s%s\n", vol(l.src), vol(l.dst), rec, seg, gate, ci);
    if (l.apply)
        printf("L k_agg_apply<%s> g=%u b=256 lds=0 : %s %s %s %d %d %d %d %s\n", tf(l.vert), (unsigned)(((long long)sc.W * sc.H + 255) / 256), vol(l.dst), vol(l.src), rec,
               sc.W, sc.H, sc.Dp, (l.divide || l.pair) ? 1 : 0, gate);
}

// the launches of a plan with the marks of the run: events before the first launch of steps 0 and 1 and at the end (profiling)
static void print_plan(const AggPlan& plan, const Scen& sc, bool marks, const char** label)
{
    for (size_t i = 0; i < plan.launch.size(); i++) {
        const AggLaunch& l = plan.launch[i];
        if (marks && sc.prof && l.step < 2 && (i == 0 || plan.launch[i - 1].step != l.step)) printf("E ev_agg[%d] heavy\n", l.step);
        print_launch(l, sc);
        if (l.label) *label = l.label;
    }
    if (marks && sc.prof) printf("E ev_agg[%d] heavy\n", std::min(plan.steps, 8));
}

static int run_table(const char* path)
{
    std::ifstream f(path);
    std::string line;
    std::map<std::string, std::string> dflt;
    while (std::getline(f, line)) {
        if (line.size() < 2 || (line[0] != 'S' && line[0] != 'D') || line[1] != ' ') continue;
        std::stringstream ss(line.substr(2));
        std::string name, tok;
        if (line[0] == 'S') ss >> name;
        std::map<std::string, std::string> kv = dflt;
        while (ss >> tok) { const size_t eq = tok.find('='); kv[tok.substr(0, eq)] = tok.substr(eq + 1); }
        if (line[0] == 'D') { dflt = kv; continue; } // (the defaults every S line starts from)
        auto I = [&](const char* k) { return atoi(kv[k].c_str()); };
        AggKnobs kn;
        apply_env(kv["penv"], &kn);
        apply_env(kv["env"], &kn);
        AggInputs in = {};
        in.W = I("W"); in.H = I("H"); in.Dp = I("Dp"); in.cross_L1 = I("L1"); in.iterations = I("it");
        in.arms = (AggArms)I("valid");
        in.armmax[0] = I("ah"); in.armmax[1] = I("av"); in.armmax_small[0] = I("sh"); in.armmax_small[1] = I("sv");
        in.rec_nz_known = I("nzk") != 0; in.rec_nz[0] = atoll(kv["nzh"].c_str()); in.rec_nz[1] = atoll(kv["nzv"].c_str());
        in.in_redo = I("redo") != 0; in.dual = I("dual") > 0; in.fuse_cost = I("fc") != 0; in.fuse_agg_so = I("fso") != 0;
        in.so_can_fuse = I("can") != 0;
        in.cost_flat_fits = agg_assumed_depth(in, kn, false) <= I("fitcap");
        const Scen sc = {in.W, in.H, I("D"), in.Dp, I("dmin"), I("prof"), I("valid"), I("ah"), I("av")};
        const char* label = "(none)";
        printf("S %s\n", name.c_str());
        AggPlan plan, f;
        const bool tail = I("tail") != 0, dual = !tail && agg_dual_wanted(in, kn);
        if (tail) { plan.launch.push_back(agg_plan_tail(in, kn)); plan.result = 1; }
        else if (dual) agg_plan_dual(in, kn, &plan, &f);
        else plan = agg_plan(in, kn, AggGate{0, 0}, false);
        print_plan(plan, sc, !tail, &label);
        if (dual) print_plan(f, sc, false, &label);
        if (dual && f.result != plan.result) printf("PLANS END IN DIFFERENT VOLUMES\n");
        printf("R err=0 end=%s other=%s first_fused=%d dual_last=%d sparse_last=%d so_agg_fused=%d launches=%d passes=%d sparse=%d gather=%d flat=%d so_fusions=%d"
               " dual_runs=%d valid=%d ah=%d av=%d label=%s\n", vol(plan.result), vol(1 - plan.result), plan.first_fused, dual, plan.sparse > 0, plan.tail_moved,
               std::min(plan.steps, 8), plan.passes, plan.sparse, plan.gather, plan.flat, plan.tail_moved, dual, sc.valid, sc.ah, sc.av, label);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- invariants
static long g_bad = 0;
#define REQUIRE(cond, what) do { if (!(cond)) { if (g_bad++ < 10) printf("VIOLATION %s (draw %ld)\n", what, draw); } } while (0)

static void check_plan(const AggInputs& in, const AggKnobs& kn, AggGate gate, const AggPlan& plan, bool first_into_cur, long draw)
{
    const bool quiet = !(in.arms == AGG_ARMS_EXACT || in.arms == AGG_ARMS_ASSUMED) || gate.code != 0 || in.in_redo || !in.rec_nz_known;
    int sparse = 0, gather = 0, flat = 0, cur = 0, step = -1;
    for (size_t i = 0; i < plan.launch.size(); i++) {
        const AggLaunch& l = plan.launch[i];
        const bool sp = l.apply || l.form == AGG_MARCH_SPARSE || l.form == AGG_GATHER;
        sparse += sp; gather += l.form == AGG_GATHER; flat += l.form == AGG_COST_FLAT;
        REQUIRE(!(quiet && (sp || l.form == AGG_COST_FLAT)), "sparse / gather / flat launch with arms unknown or full ring, in a two-plan run, in a redo or without densities");
        REQUIRE(l.form != AGG_GATHER || (l.apply && agg_sparse_wanted(in, kn, gate, l.vert, l.pair)), "gather implies sparse");
        REQUIRE(l.apply == (l.form == AGG_GATHER || l.form == AGG_MARCH_SPARSE), "k_agg_apply follows exactly the sparse forms");
        if (l.form == AGG_COST_FLAT)
            REQUIRE(i == 0 && agg_ring(in, kn, false) == AGG_RING_SMALL && in.Dp % 128 == 0 && l.costin && in.cost_flat_fits, "flat implies small ring only, Dp % 128 == 0, first launch");
        if (l.costin) REQUIRE(l.step == 0 && plan.first_fused && l.dst == (first_into_cur ? 0 : 1), "a fused-cost launch is the first pass and writes the volume asked for");
        else REQUIRE(l.src != l.dst && l.src == cur, "every launch reads the volume that holds the state and writes the other");
        REQUIRE(l.src >= 0 && l.src <= 1 && l.dst >= 0 && l.dst <= 1 && l.grid >= 1u - (l.form == AGG_COST_FLAT) && l.depth >= 0 && l.depth <= 255, "volumes, grid and depth in range");
        REQUIRE(l.step == step || l.step == step + 1, "steps count up");
        step = l.step;
        const bool last_of_step = i + 1 == plan.launch.size() || plan.launch[i + 1].step != l.step;
        if (last_of_step) cur = sp ? l.src : l.dst; // (a sparse launch leaves its result in the volume it read)
    }
    REQUIRE(step + 1 == plan.steps, "every step has a launch");
    REQUIRE(cur == plan.result, "the plan ends where its last launch left the result");
    REQUIRE(sparse == plan.sparse && gather == plan.gather && flat == plan.flat && gather <= sparse, "counters equal the launches");
    REQUIRE(plan.passes == 2 * std::max(0, in.iterations) - (plan.tail_moved ? 1 : 0), "passes == 2 x iterations, minus one when the tail moved");
    REQUIRE(!plan.tail_moved || (gate.code == 0 && in.fuse_agg_so && in.so_can_fuse && in.iterations == 4), "the tail only moves when asked and possible");
}

static int run_random(unsigned seed, long n)
{
    std::mt19937 rng(seed);
    auto R = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    const int L1s[] = {0, 1, 4, 8, 9, 17, 34, 35, 36, 40, 49, 255, 300, -3};
    long duals = 0;
    for (long draw = 0; draw < n; draw++) {
        AggInputs in = {};
        in.W = R(0, 3) ? R(1, 2000) : R(1, 8); in.H = R(0, 3) ? R(1, 1200) : R(1, 8); in.Dp = 64 * R(1, 4);
        in.cross_L1 = R(0, 1) ? L1s[R(0, 13)] : R(0, 60);
        in.iterations = R(0, 3) ? 4 : R(0, 6);
        in.arms = (AggArms)R(0, 3);
        for (int c = 0; c < 2; c++) { in.armmax[c] = R(0, 2) ? R(0, 9) : R(0, 60); in.armmax_small[c] = R(0, 9); }
        const long long P = (long long)in.W * in.H;
        for (int c = 0; c < 2; c++) in.rec_nz[c] = R(0, 1) ? (long long)(P * (R(0, 300) / 1000.0)) : R(0, 1) * P;
        in.rec_nz_known = R(0, 3) != 0; in.in_redo = R(0, 5) == 0; in.dual = R(0, 3) == 0; in.fuse_cost = R(0, 3) != 0; in.fuse_agg_so = R(0, 3) != 0;
        in.so_can_fuse = R(0, 3) != 0;
        AggKnobs kn;
        if (R(0, 2) == 0) {
            kn.small_L = R(0, 2) ? 8 : R(0, 12); kn.vpl2 = R(0, 2); kn.regring = R(0, 1); kn.rr2 = R(0, 1); kn.pair = R(0, 1); kn.pair_full = R(0, 2);
            kn.assume_margin = R(0, 3); kn.sparse = R(0, 3) != 0; kn.gather = R(0, 3) != 0; kn.cost_flat = R(0, 3) != 0; kn.dual = R(0, 3) != 0;
            kn.sparse_density = R(0, 300) / 1000.0; kn.gather_density = R(0, 300) / 1000.0; kn.cost_flat_density = R(0, 300) / 1000.0;
            for (int c = 0; c < 2; c++) { kn.seg[c] = R(0, 3) ? 0 : R(1, 40); kn.chunk[c] = R(0, 3) ? 0 : R(1, 100000); }
        }
        in.cost_flat_fits = in.Dp % 128 == 0 && R(0, 3) != 0;
        if (agg_dual_wanted(in, kn)) {
            AggPlan s, f;
            agg_plan_dual(in, kn, &s, &f);
            duals++;
            REQUIRE(s.result == f.result, "both plans of a two-plan run end in the same volume");
            REQUIRE(s.sparse + s.gather + s.flat + f.sparse + f.gather + f.flat == 0 && !s.tail_moved && !f.tail_moved, "a two-plan run has no sparse / gather / flat launch and keeps its tail");
            REQUIRE(s.first_fused && f.first_fused, "both plans start with the fused cost");
            for (const AggLaunch& l : s.launch) REQUIRE(l.small_variant == 3, "every launch of plan S carries gate 3");
            for (const AggLaunch& l : f.launch) REQUIRE(l.small_variant == 4 && l.small_L == s.launch[0].small_L, "every launch of plan F carries gate 4 and the depths of S");
        } else {
            const bool fic = in.fuse_cost && R(0, 7) == 0;
            check_plan(in, kn, AggGate{0, 0}, agg_plan(in, kn, AggGate{0, 0}, fic), fic, draw);
        }
    }
    printf("draws=%ld two_plan=%ld violations=%ld\n", n, duals, g_bad);
    return g_bad ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- one plan
static const char* const form_name[AGG_FORM_COUNT] = {"march_full", "march_small", "march_small2", "march_sparse", "gather", "regring", "regring_pair",
                                                      "regring_cost", "rr2", "rr2_cost", "cost_flat"};

static int run_one(const std::string& line)
{
    std::stringstream ss(line);
    std::string tok;
    std::map<std::string, std::string> kv = {{"it", "4"}, {"fc", "1"}, {"fso", "1"}, {"env", "-"}, {"redo", "0"}, {"dual", "0"}, {"nzk", "0"}, {"nzh", "0"},
                                             {"nzv", "0"}, {"sh", "0"}, {"sv", "0"}, {"ah", "0"}, {"av", "0"}, {"can", "0"}, {"fits", "0"}};
    while (ss >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) { fprintf(stderr, "not key=val: %s\n", tok.c_str()); return 2; }
        kv[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    for (const char* need : {"W", "H", "Dp", "L1", "valid"})
        if (!kv.count(need)) { fprintf(stderr, "missing %s=\n", need); return 2; }
    auto I = [&](const char* k) { return atoi(kv[k].c_str()); };
    AggKnobs kn;
    apply_env(kv["env"], &kn);
    AggInputs in = {};
    in.W = I("W"); in.H = I("H"); in.Dp = I("Dp"); in.cross_L1 = I("L1"); in.iterations = I("it");
    in.arms = (AggArms)I("valid");
    in.armmax[0] = I("ah"); in.armmax[1] = I("av"); in.armmax_small[0] = I("sh"); in.armmax_small[1] = I("sv");
    in.rec_nz_known = I("nzk") != 0; in.rec_nz[0] = atoll(kv["nzh"].c_str()); in.rec_nz[1] = atoll(kv["nzv"].c_str());
    in.in_redo = I("redo") != 0; in.dual = I("dual") > 0; in.fuse_cost = I("fc") != 0; in.fuse_agg_so = I("fso") != 0;
    in.so_can_fuse = I("can") != 0; in.cost_flat_fits = I("fits") != 0;
    AggPlan plan, f;
    const bool dual = agg_dual_wanted(in, kn);
    if (dual) agg_plan_dual(in, kn, &plan, &f);
    else plan = agg_plan(in, kn, AggGate{0, 0}, false);
    printf("sparse=%d gather=%d flat=%d tail_moved=%d first_fused=%d dual=%d forms=", plan.sparse + f.sparse, plan.gather + f.gather, plan.flat + f.flat,
           plan.tail_moved ? 1 : 0, plan.first_fused ? 1 : 0, dual ? 1 : 0);
    bool sep = false;
    for (const AggPlan* p : {&plan, &f})
        for (const AggLaunch& l : p->launch) {
            printf("%s%s%s:%d", sep ? "," : "", form_name[l.form], l.pair ? "+pair" : "", l.depth);
            sep = true;
        }
    printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && std::string(argv[1]) == "one" && std::string(argv[2]) == "-") {
        std::string line;
        int rc = 0;
        while (rc == 0 && std::getline(std::cin, line))
            if (!line.empty()) rc = run_one(line);
        return rc;
    }
    if (argc >= 3 && std::string(argv[1]) == "one") {
        std::string line;
        for (int i = 2; i < argc; i++) line += std::string(argv[i]) + " ";
        return run_one(line);
    }
    if (argc == 3 && std::string(argv[1]) == "table") return run_table(argv[2]);
    if (argc == 4 && std::string(argv[1]) == "random") return run_random((unsigned)atol(argv[2]), atol(argv[3]));
    fprintf(stderr, "usage: emul_agg_plan table FILE | random SEED N | one key=val... | one -\n");
    return 2;
}
