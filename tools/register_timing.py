#!/usr/bin/env python3
"""Times the registration of depth into a second camera (adc_register_depth_device: two memsets, k_reg_scatter, k_reg_resolve, the
pinned read-back; adc_align_color_device: k_reg_align) on one MI355X at 1920x1080 into 1920x1080 and 3840x2160, prices its traffic and
checks that the plain figures did not move; writes profiles/register_timing.md.

    python tools/register_timing.py [--parent-lib DIR/libadcensus_hip.so --parent-commit HASH] [--out profiles/register_timing.md]

The driver starts one child process per step (this file with --child ..., or tools/products_timing.py --child plain / device for the
plain figures), each with its own time limit, and stops at the first step that fails.
  calls    per target size, map (noise: independent disparities, every neighbour at another depth; structured: two planes and a
           nearer rectangle) and form of the scatter (with the pre-test load, ADC_REG_PRETEST / every atomic issued, the default): N calls enqueued back to back on
           the handle's stream, one adc_wait, best of --reps.  The priced bytes stand next to the time: 8 Pt for the z-buffer memset,
           4 P for the map, 8 per candidate key, 16 Pt for the resolve; the candidate count is the definition's (tests/register_ref.py)
  kernels  the same configurations, one `rocprofv3 --kernel-trace --stats` run each (and nothing else in it): average time of
           k_reg_scatter, k_reg_resolve, k_reg_align, and candidates / scatter time = the achieved rate of 64-bit minimum atomics
  plain    adc_match_device + adc_wait (ms per pair) and adc_farm_submit (pairs/s) of the parent build and of this build, --reps
           repetitions each, alternating; the new median is judged against the min-max spread of the parent's own repetitions"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
N = W * H
CALIB = (0.8 * W, 0.16, W / 2 - 0.3, H / 2 + 0.2, 1.25)
TARGETS = ["1920x1080", "3840x2160"]
MAPS = ["noise", "structured"]
FORMS = ["pre-test load", "every atomic"]
TAG = "REGISTER_TIMING "


def source_map(name):
    rng = np.random.default_rng(1)
    if name == "noise":
        m = rng.uniform(4.0, 64.0, (H, W)).astype(np.float32)
    else:
        y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        m = np.where(y < H // 2, 20 + 0.01 * x + 0.005 * y, 30 + 0.004 * x + 0.02 * y).astype(np.float32)
        m[H // 4:(3 * H) // 5, W // 3:(2 * W) // 3] = 50
    m[rng.random((H, W)) < 0.03] = np.inf
    return m


def target_for(A, size):
    wt, ht = (int(v) for v in size.split("x"))
    sx, sy = wt / W, ht / H
    return A.RegTarget(width=wt, height=ht, fx=CALIB[0] * sx, fy=CALIB[0] * sy, cx=CALIB[2] * sx, cy=CALIB[3] * sy, t=[-1.5 * CALIB[1], 0, 0], k1=-0.05, k2=0.01)


def child(a):
    import adcensus_amd as A
    from tests import register_ref as R
    L = A.lib()
    out = {"version": L.adc_version().decode()}
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, A.ADCensusOption(max_disparity=16)), A.last_error()
    configs = [(t, m) for t in TARGETS for m in MAPS] if a.child == "calls" else [tuple(a.config.split(",")[:2])]
    for size, name in configs:
        target = target_for(A, size)
        nt = target.width * target.height
        st.set_register_target(target)
        bufs = [L.adc_device_malloc(s) for s in (4 * N, 4 * nt, 4 * nt, 3 * nt, 3 * N, N)]
        dm, dz, di, dt, do, dv = bufs
        tbgr = np.random.default_rng(2).integers(0, 256, (target.height, target.width, 3), dtype=np.uint8)
        m = source_map(name)
        assert L.adc_memcpy_h2d(dt, tbgr.ctypes.data, tbgr.nbytes) == 0 and L.adc_memcpy_h2d(dm, m.ctypes.data, m.nbytes) == 0
        if a.child == "kernels":  # (under the profiler: the launches and nothing else)
            flags = A.REG_PRETEST if a.config.split(",")[2] == FORMS[0] else 0
            for _ in range(a.batch):
                assert st.register_depth_device(dm, CALIB, A.REG_FROM_DISPARITY, flags, dz, di), A.last_error()
                assert st.align_color_device(dm, CALIB, dt, do, dv), A.last_error()
            assert st.wait(), A.last_error()
        else:
            want = R.register(m, R.FROM_DISPARITY, CALIB, target)[2]
            key = "%s %s " % (size, name)
            out[key + "candidates"], out[key + "filled"], out[key + "projected"] = want["candidates"], want["dst_filled"], want["src_projected"]
            for form, flags in ((FORMS[0], A.REG_PRETEST), (FORMS[1], 0)):
                best = 1e9
                for _ in range(a.reps + 1):
                    t0 = time.perf_counter()
                    for _ in range(a.batch):
                        assert st.register_depth_device(dm, CALIB, A.REG_FROM_DISPARITY, flags, dz, di), A.last_error()
                    assert st.wait(), A.last_error()
                    best = min(best, (time.perf_counter() - t0) * 1e3 / a.batch)
                rep = st.register_report()
                assert (rep.src_valid, rep.src_projected, rep.dst_filled) == (want["src_valid"], want["src_projected"], want["dst_filled"]), key
                out[key + form] = best
            best = 1e9
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                for _ in range(a.batch):
                    assert st.align_color_device(dm, CALIB, dt, do, dv), A.last_error()
                assert st.wait(), A.last_error()
                best = min(best, (time.perf_counter() - t0) * 1e3 / a.batch)
            out[key + "align"] = best
        for b in bufs:
            L.adc_device_free(b)
    st.Release()
    print(TAG + json.dumps(out), flush=True)


def run_child(script, args, lib, limit, tag, prefix=()):
    env = dict(os.environ, ADC_HIP_LIB=lib) if lib else dict(os.environ)
    cmd = list(prefix) + [sys.executable, script] + args
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith(tag)]
    if r.returncode != 0 or not lines:
        print("step %s failed (exit %d): %s" % (" ".join(args), r.returncode, (r.stdout + r.stderr)[-2000:]), flush=True)
        sys.exit(1)  # (nothing more is started on the GPU behind a step that failed)
    print("step %s ok" % " ".join(args), flush=True)
    return json.loads(lines[-1][len(tag):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--new-first", action="store_true", help="plain: each repetition runs this build before the parent's (default: the parent's first)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_timing.md"))
    ap.add_argument("--prof-dir", default="", help="where rocprofv3 writes (default: a temporary directory)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = os.path.abspath(__file__)
    prof_dir = a.prof_dir or tempfile.mkdtemp(prefix="register_prof_")
    md = ["# Registration into a second camera: timing on one MI355X, source 1920x1080", "",
          "`tools/register_timing.py`; %d calls enqueued back to back and one `adc_wait`, best of %d; kernel times from one `rocprofv3 --kernel-trace --stats` run per "
          "configuration (average over %d launches).  P = 2073600 source pixels, Pt target pixels; priced bytes = 8 Pt (z-buffer memset) + 4 P (map) + 8 per "
          "candidate key + 16 Pt (resolve: 8 read, 4 + 4 written); align: 4 P + 3 P gathered + 4 P written." % (a.batch, a.reps, a.batch), ""]
    calls = run_child(me, ["--child", "calls", "--batch", str(a.batch), "--reps", str(a.reps)], "", 900, TAG)
    md += ["## Whole calls (`adc_register_depth_device`, `adc_align_color_device`), ms per call", "",
           "| target | map | candidates | target pixels filled | priced MB | pre-test load | every atomic | priced bytes / time (every atomic) | align | align priced MB |", "|---|---|---|---|---|---|---|---|---|---|"]
    for size in TARGETS:
        wt, ht = (int(v) for v in size.split("x"))
        for name in MAPS:
            k = "%s %s " % (size, name)
            priced = 8 * wt * ht + 4 * N + 8 * calls[k + "candidates"] + 16 * wt * ht
            md.append("| %s | %s | %d | %d | %.1f | %.4f | %.4f | %.2f TB/s | %.4f | %.1f |" % (size, name, calls[k + "candidates"], calls[k + "filled"], priced / 1e6, calls[k + FORMS[0]],
                                                                                           calls[k + FORMS[1]], priced / calls[k + FORMS[1]] / 1e9, calls[k + "align"], 11 * N / 1e6))
    md += ["", "## Kernels alone (rocprofv3), ms per launch", "",
           "| target | map | form | k_reg_scatter | k_reg_resolve | k_reg_align | 64-bit minimum atomics issued at most | atomics / us at most |", "|---|---|---|---|---|---|---|---|"]
    for size in TARGETS:
        for name in MAPS:
            for form in FORMS:
                tag = "%s_%s_%s" % (size, name, form.split()[0])
                run_child(me, ["--child", "kernels", "--config", "%s,%s,%s" % (size, name, form), "--batch", str(a.batch)], "", 600, TAG,
                          prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", prof_dir, "-o", tag, "--output-format", "csv", "--"))
                avg = {}
                for path in glob.glob(os.path.join(prof_dir, "**", tag + "*kernel_stats.csv"), recursive=True):
                    for row in csv.DictReader(open(path)):
                        for kn in ("k_reg_scatter", "k_reg_resolve", "k_reg_align"):
                            if kn in row.get("Name", ""):
                                avg[kn] = float(row["AverageNs"]) / 1e6
                cand = calls["%s %s candidates" % (size, name)]
                if len(avg) == 3:
                    # (with the pre-test load only the keys that could still win are issued: the candidate count is an upper bound there)
                    md.append("| %s | %s | %s | %.4f | %.4f | %.4f | %d | %.0f |" % (size, name, form, avg["k_reg_scatter"], avg["k_reg_resolve"], avg["k_reg_align"], cand,
                                                                                 cand / (avg["k_reg_scatter"] * 1e3)))
                else:
                    md.append("| %s | %s | %s | not measured (no kernel_stats.csv rows) | | | %d | |" % (size, name, form, cand))
    md += ["", "## The plain figures against the parent (%s), %d alternating repetitions each" % (a.parent_commit, a.reps), ""]
    if a.parent_lib:
        new_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip.so")
        pt = os.path.join(ROOT, "tools", "products_timing.py")
        runs = {(s, t): [] for s in ("device", "plain") for t in ("parent", "new")}
        for _ in range(a.reps):
            for step in ("device", "plain"):
                for tag, lib in ((("new", new_lib), ("parent", a.parent_lib)) if a.new_first else (("parent", a.parent_lib), ("new", new_lib))):
                    runs[(step, tag)].append(run_child(pt, ["--child", step, "--seconds", str(a.seconds)], lib, 300, "PRODUCTS_TIMING "))
        md += ["1920x1080, D = 128, the benchmark's noise and structured pairs (`tools/products_timing.py --child device / plain`, windows of at least %.0f s after a "
               "warm-up; the library is selected with `ADC_HIP_LIB`; within a repetition %s runs first)." % (a.seconds, "this build" if a.new_first else "the parent"), "",
               "| figure | pair | parent repetitions | parent min - max | new repetitions | new median | inside the parent's spread |", "|---|---|---|---|---|---|---|"]
        for step, label, key, fmt in (("device", "`adc_match_device` + `adc_wait`, ms per pair", "%s plain", "%.3f"), ("plain", "`adc_farm_submit`, 3 pipelines, pairs/s", "%s", "%.1f")):
            for pair in ("noise", "structured"):
                p, n = [r[key % pair] for r in runs[(step, "parent")]], [r[key % pair] for r in runs[(step, "new")]]
                med = statistics.median(n)
                verdict = "yes" if min(p) <= med <= max(p) else ("outside: " + ("above" if med > max(p) else "below"))
                md.append(("| %s | %s | %s | " + fmt + " - " + fmt + " | %s | " + fmt + " | %s |") % (label, pair, " ".join(fmt % v for v in p), min(p), max(p),
                                                                                             " ".join(fmt % v for v in n), med, verdict))
    else:
        md.append("not measured (no parent library given)")
    text = "\n".join(md) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
