"""A model of the host rules that decide what a Match launches from what its handle has learned: a plain, independent restatement of
adcensus_amd/csrc/learn_plan.h -- the commit behind a Match, the arm assumption of the next one, the scanline segments, whether the
tail may move, whether the flat first launch fits.  It is the check, not the thing checked: tests/test_stream_model.py compares it with
the header on the CPU (tests/emul/emul_learn.cpp), tests/test_gpu_streams.py with the device.  Only the named constants (hold lengths,
warm-up, segment limit, the two knob defaults) come from the product, through `emul_learn consts`.  The plan itself comes from the
product's own header through tests/emul/emul_agg_plan.cpp ("one").  The model is fed the oracle's facts about every image of a stream (tests/streams.py:
arm maxima and record densities) and predicts, per Match, the deltas of debug counters 2, 10, 11, 16, 20, 22 and whether the last
aggregation pass may move into the scanline stage (counter 13).  It reads nothing back from the product except the density thresholds
(counters 17, 21, 23)."""
import functools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adcensus_amd", "csrc")

AGG_ARMS_ASSUMED, AGG_ARMS_FULL = 2, 3
CF_TX, CF_LDS_MAX = 128, 48 * 1024  # k_cost.hip
# SMALL_L_KNOB, ASSUME_MARGIN (defaults of ADC_AGG_SMALL_L / ADC_AGG_ASSUME_MARGIN), SO_WARM, SO_MAX_SEG (adc_device_fn.h): from the
# product, the first time one is asked for
_FROM_CONSTS = {"SMALL_L_KNOB": "small_L", "ASSUME_MARGIN": "assume_margin", "SO_WARM": "so_warm", "SO_MAX_SEG": "so_max_seg"}


def __getattr__(name):
    if name in _FROM_CONSTS:
        return consts()[_FROM_CONSTS[name]]
    raise AttributeError(name)


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def consts():
    """`emul_learn consts`: the named constants of learn_plan.h, adc_device_fn.h and the knob defaults of agg_plan.h"""
    out = subprocess.check_output([build_emul("emul_learn"), "consts"], text=True)
    return {k: int(v) for k, v in (t.split("=", 1) for t in out.split())}


def holds():
    """The lengths of the four "hold for N Matches" counters, from the code that sets them (by the field each one sets)."""
    c = consts()
    return {"agg_dual": c["plan_switch"], "so_seg_off": c["so_seam"], "med_seg_off": c["med_column"], "med_spec_off": c["med_band"]}


def default_thresholds_ppm():
    """counters 17, 21, 23 of a process with no density override, from agg_plan.h"""
    v = float(re.search(r"#define AGG_SPARSE_MAX_DENSITY ([0-9.]+)", _src("agg_plan.h")).group(1))
    ppm = int(v * 1e6 + 0.5)
    return {"sparse": ppm, "gather": ppm, "flat": ppm}  # (AGG_GATHER_MAX_DENSITY and COST_FLAT_MAX_DENSITY are defined as the first)


def build_emul(name="emul_agg_plan"):
    out_dir = os.path.join(ROOT, "tests", "emul", "_build")
    exe = os.path.join(out_dir, name)
    deps = [os.path.join(ROOT, "tests", "emul", name + ".cpp"), os.path.join(CSRC, "agg_plan.h")]
    if name == "emul_learn":
        deps += [os.path.join(CSRC, "learn_plan.h"), os.path.join(CSRC, "adc_device_fn.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        os.makedirs(out_dir, exist_ok=True)
        tmp = "%s.%d" % (exe, os.getpid())  # (built aside and renamed: another process may be running the old one)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", deps[0], "-o", tmp])
        os.replace(tmp, exe)
    return exe


def plan_many(exe, scenarios):
    """[{key: value}] -> [{sparse, gather, flat, tail_moved, first_fused, dual, forms}] through `emul_agg_plan one -`"""
    text = "".join(" ".join("%s=%s" % kv for kv in s.items()) + "\n" for s in scenarios)
    out = subprocess.run([exe, "one", "-"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(scenarios), (len(out), len(scenarios))
    res = []
    for line in out:
        kv = dict(t.split("=", 1) for t in line.split())
        res.append({k: (v.split(",") if k == "forms" else int(v)) for k, v in kv.items()})
    return res


# ---- facts about the handle (not about the image)
def vpl_of(d):
    return 1 if d <= 64 else 2 if d <= 128 else 4 if d <= 256 else 8 if d <= 512 else 16 if d <= 1024 else 32


def so_seg_start(plen, nseg, warm, s):
    if s <= 0:
        return 0
    if s >= nseg:
        return plen
    t = (plen + (nseg - 1) * (warm + 1) + nseg - 1) // nseg
    return ((t + (s - 1) * (t - warm - 1)) & ~3) + 1


def so_seg_ok(plen, nseg, warm):
    if nseg < 2 or nseg > consts()["so_max_seg"] or warm < 16 or (warm & 15):
        return False
    return all(so_seg_start(plen, nseg, warm, s) - so_seg_start(plen, nseg, warm, s - 1) >= 32 + (warm + 1 if s == 1 else 0)
               for s in range(1, nseg + 1))


def so_segments(w, h, vpl, so_seg_off, seg_env=-1, warm=None):
    """adc_so_segments; seg_env / warm: ADC_SO_SEG / ADC_SO_WARM (unset: -1 and the production warm-up)"""
    warm = consts()["so_warm"] if warm is None else warm
    if vpl > 2 or so_seg_off or seg_env in (0, 1):
        return 1
    n = seg_env if seg_env >= 2 else (2048 + h // 2) // h
    if seg_env < 2 and n == 2 and 3 * h <= 4096:
        n = 3
    n = min(n, consts()["so_max_seg"])
    while n >= 2 and not so_seg_ok(w, n, warm):
        n -= 1
    return n if n >= 2 else 1


def so_can_fuse(w, h, vpl, so_seg_off, so_fast, so_seg_probe=0, seg_env=-1):
    """adc_so_can_fuse_agg; so_fast: None (ADC_SO_FAST unset: the pinned family below 1024 chains) or 0 / 1; so_seg_probe: a seam of
    the handle failed and no segmented Match has held since (no seam fails in the model's streams: the handles there never set it)"""
    if vpl != 2 or so_seg_probe:
        return False
    nseg = so_segments(w, h, vpl, so_seg_off, seg_env)
    pin = (so_fast != 0) if so_fast is not None else h * nseg < 1024
    return nseg > 1 and not pin


def cost_flat_fits(dp, cap):
    return dp % 128 == 0 and cap >= 0 and (768 + 64 + 3 * (CF_TX + dp - 1 + 2 * cap)) * 4 <= CF_LDS_MAX


class HandleModel:
    """One handle.  match(facts) -> the prediction for this Match, and the state moves on as adc_wait moves it."""

    def __init__(self, exe, w, h, dmin, dmax, cross_L1=34, so_fast=None, thresholds_ppm=None, hold=None):
        self.exe, self.w, self.h = exe, w, h
        self.vpl = vpl_of(dmax - dmin)
        self.dp = 64 * self.vpl
        self.L1 = cross_L1
        self.so_fast = so_fast
        self.thr = thresholds_ppm or default_thresholds_ppm()
        self.hold = hold if hold is not None else holds()["agg_dual"]
        self.full_L = max(0, min(cross_L1, 255))
        self.small_L = min(consts()["small_L"], self.full_L)
        self.small_ok = 0 < self.small_L < self.full_L
        self.arm_known = 0
        self.armmax_host = [0, 0]
        self.armmax_small = [0, 0]
        self.rec_nz = [0, 0]
        self.rec_nz_known = 0
        self.agg_dual = 0
        self.agg_last_plan = 0
        self.so_seg_off = 0

    def _depth(self, c):  # agg_assumed_depth with ASSUMED arms
        return min(self.small_L, max(1, self.armmax_host[c]) + consts()["assume_margin"])

    def scenario(self):
        valid = AGG_ARMS_ASSUMED if self.arm_known else AGG_ARMS_FULL  # run_heavy: the AggArms it passes
        cap = min(self.small_L, max(1, self.armmax_host[0]) + (consts()["assume_margin"] if valid == AGG_ARMS_ASSUMED else 0))
        env = "ADC_AGG_SPARSE_DENSITY=%de-6,ADC_AGG_GATHER_DENSITY=%de-6,ADC_COST_FLAT_DENSITY=%de-6" % (
            self.thr["sparse"], self.thr["gather"], self.thr["flat"])
        return {"W": self.w, "H": self.h, "Dp": self.dp, "L1": self.L1, "it": 4, "valid": valid, "ah": self.armmax_host[0],
                "av": self.armmax_host[1], "sh": self.armmax_small[0], "sv": self.armmax_small[1], "nzk": self.rec_nz_known,
                "nzh": self.rec_nz[0], "nzv": self.rec_nz[1], "redo": 0, "dual": 1 if self.agg_dual > 0 else 0, "fc": 1, "fso": 1,
                "can": 1 if so_can_fuse(self.w, self.h, self.vpl, self.so_seg_off, self.so_fast) else 0,
                "fits": 1 if cost_flat_fits(self.dp, cap) else 0, "env": env}

    def match(self, facts):
        plan = plan_many(self.exe, [self.scenario()])[0]
        return self.apply(plan, facts)

    def apply(self, plan, facts):
        """plan: what emul_agg_plan says for scenario(); facts: of the image being matched"""
        am, nz = facts["armmax"], facts["nz"]
        assumed = bool(self.arm_known)
        gate = [False, False]  # a small ring of this direction, assumed from the previous image, is too shallow: armmax[3] is raised
        if assumed and not plan["dual"]:
            for c in range(2):
                small = self.small_ok and self.armmax_host[c] <= self.small_L  # agg_ring
                gate[c] = small and am[c] > self._depth(c)
        redo = gate[0] or gate[1]
        pred = {"first": not assumed, "assumed": assumed and not plan["dual"], "dual": plan["dual"], "redo": int(redo), "redo_h": gate[0], "redo_v": gate[1],
                "d2": int(redo), "d11": int(redo and plan["first_fused"]), "d10": plan["dual"], "d16": plan["sparse"], "d20": plan["gather"],
                "d22": plan["flat"], "fuse": plan["tail_moved"], "forms": plan["forms"]}
        # adc_wait
        if redo:
            self.arm_known = 0
            self.so_seg_off = max(self.so_seg_off, 1)  # whole rows in every redo (full ring, no sparse launch, no moved tail)
        self.armmax_host = list(am)
        self.arm_known = 1
        self.rec_nz, self.rec_nz_known = list(nz), 1
        if self.so_seg_off > 0:
            self.so_seg_off -= 1
        p = 1 if (am[0] <= self.small_L and am[1] <= self.small_L) else 2
        if p == 1:
            self.armmax_small = [max(am[0], 1), max(am[1], 1)]
        if self.agg_last_plan != 0 and p != self.agg_last_plan:
            self.agg_dual = self.hold
        elif self.agg_dual > 0:
            self.agg_dual -= 1
        self.agg_last_plan = p
        return pred


def predict_stream(exe, geometry, opt_fields, so_fast, keys, table, thresholds_ppm=None):
    """keys: the image key of every Match of one handle; table: {key: facts}.  -> [prediction per Match]"""
    w, h, dmin, dmax = geometry
    m = HandleModel(exe, w, h, dmin, dmax, cross_L1=opt_fields.get("cross_L1", 34), so_fast=so_fast, thresholds_ppm=thresholds_ppm)
    return [m.match(table[k]) for k in keys]


KINDS = ("first_or_full", "assumed_dense", "sparse_gather_flat", "fused", "two_plans", "redo_h_only", "redo_v_only", "after_redo")


def kinds_of(preds):
    """the coverage kinds of tests/test_stream_model.py each Match of a stream belongs to"""
    out = []
    for i, p in enumerate(preds):
        k = set()
        if p["first"] or (p["assumed"] and not any(f.startswith(("march_small", "march_sparse", "gather", "cost_flat")) for f in p["forms"])):
            k.add("first_or_full")
        if p["assumed"] and p["d16"] == 0 and any(f.startswith("march_small2") for f in p["forms"]):  # (two disparities per lane: sparse was possible)
            k.add("assumed_dense")
        if p["d16"] > 0 and p["d20"] > 0 and p["d22"] > 0:
            k.add("sparse_gather_flat")
        if p["fuse"]:
            k.add("fused")
        if p["dual"]:
            k.add("two_plans")
        if p["redo_h"] and not p["redo_v"]:
            k.add("redo_h_only")
        if p["redo_v"] and not p["redo_h"]:
            k.add("redo_v_only")
        if i > 0 and preds[i - 1]["redo"]:
            k.add("after_redo")
        out.append(k)
    return out
