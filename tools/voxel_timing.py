#!/usr/bin/env python3
"""Times the voxel-grid filter of the cloud (adc_set_cloud_voxel_grid) on one MI355X at 1920x1080, D = 128, on the final maps of the
benchmark's noise and structured pairs, and writes profiles/voxel_timing.md.

    python tools/voxel_timing.py --parent-lib DIR/libadcensus_hip.so --parent-commit HASH --new-commit HASH [--out profiles/voxel_timing.md]

The driver starts one child process per step (this file with --child ...), each with its own time limit, and stops at the first step
that fails.  A child selects its library with ADC_HIP_LIB.  Every comparison alternates its sides inside one child, --reps times.
  reproject  cloud-only adc_reproject_device: plain, voxel at the small and at the large leaf; 20 calls enqueued back to back and one
             adc_wait, best of 5 per repetition
  kernel     the same calls under rocprofv3 --kernel-trace --stats, one run per map and leaf: average time of every kernel of the path
  farm       adc_farm_submit(_products), 3 pipelines, host delivery: no product, the cloud at capacity W*H, the voxel cloud (large leaf)
  bench      bench.py --gpus 1, the plain headline: the parent build against this build, alternating"""
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
W, H, D, PIPES = 1920, 1080, 128, 3
N = W * H
CALIB = (1050.0, 0.54, W / 2.0, H / 2.0, 0.0)  # Z = 567 / |d|: 4.4 at d = 128; a pixel's footprint Z / f is 0.004 there, 0.05 at d = 10
LEAVES = {"small": 0.02, "large": 0.2}
KERNELS = ["k_out_measure", "k_out_scan", "k_out_emit", "k_vox_insert", "k_vox_count", "k_vox_scan", "k_vox_emit"]


def pairs():
    from adcensus_amd import workloads
    return {"noise": workloads.noise_pair(W, H, 12345), "structured": workloads.structured_pair(W, H, D, 777)}


def device_maps(A, st):
    """the final map of each pair and its left image on the device"""
    L = A.lib()
    out = {}
    for name, (left, right) in pairs().items():
        disp = st.match(left, right)
        dd, dl = L.adc_device_malloc(4 * N), L.adc_device_malloc(3 * N)
        assert L.adc_memcpy_h2d(dd, disp.ctypes.data, 4 * N) == 0 and L.adc_memcpy_h2d(dl, np.ascontiguousarray(left).ctypes.data, 3 * N) == 0
        out[name] = (dd, dl)
    return out


def set_grid(st, which):
    if which == "plain":
        st.clear_cloud_voxel_grid()
    else:
        st.set_cloud_voxel_grid(LEAVES[which])


def farm_rate(farm, pair, slots, seconds):
    def round_():
        for disp, req in slots:
            farm.submit(pair[0], pair[1], disp, req)
    for _ in range(2):
        round_()
    farm.drain()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        round_()
        n += len(slots)
    farm.drain()
    return n / (time.perf_counter() - t0)


def child(a):
    import adcensus_amd as A
    L = A.lib()
    opt = A.ADCensusOption(max_disparity=D)
    out = {"version": L.adc_version().decode()}
    if a.child in ("reproject", "kernel"):
        st = A.ADCensusStereo(device=0)
        assert st.Initialize(W, H, opt), A.last_error()
        maps = device_maps(A, st)
        pc, pn = L.adc_device_malloc(16 * N), L.adc_device_malloc(16)

        def burst(dd, dl, calls=20):
            t0 = time.perf_counter()
            for _ in range(calls):
                assert st.reproject_device(dd, dl, CALIB, None, pc, N, pn, None), A.last_error()
            assert st.wait(), A.last_error()
            return (time.perf_counter() - t0) * 1e3 / calls

        if a.child == "kernel":  # (under the profiler: one map, one form)
            dd, dl = maps[a.map]
            set_grid(st, a.form)
            burst(dd, dl)
            out["count"] = st.cloud_count()
        else:
            for name, (dd, dl) in maps.items():
                for which in ("plain", "small", "large"):
                    set_grid(st, which)
                    burst(dd, dl)
                    out["%s %s count" % (name, which)] = st.cloud_count()
                    if which != "plain":
                        out["%s %s report" % (name, which)] = st.voxel_report()
                for rep in range(a.reps):
                    for which in ("plain", "small", "large"):
                        set_grid(st, which)
                        out.setdefault("%s %s" % (name, which), []).append(min(burst(dd, dl) for _ in range(5)))
        st.Release()
    elif a.child == "farm":
        farm = A.PairFarm(W, H, opt, device=0, pipelines=PIPES)
        for name, pair in pairs().items():
            for rep in range(a.reps):
                for which in ("none", "cloud", "voxel"):
                    farm.set_cloud_voxel_grid(LEAVES["large"] if which == "voxel" else None)
                    slots = [(np.zeros((H, W), np.float32), None if which == "none" else A.Products.from_arrays(calib=CALIB, cloud=np.zeros(N, A.POINT_DTYPE)))
                             for _ in range(PIPES)]
                    out.setdefault("%s %s" % (name, which), []).append(farm_rate(farm, pair, slots, a.seconds))
                    if which != "none":
                        out["%s %s count" % (name, which)] = int(slots[0][1].count[0])
        farm.close()
    print("VOXEL_TIMING " + json.dumps(out), flush=True)


def run(cmd, limit, lib=None, tag="VOXEL_TIMING "):
    env = dict(os.environ, ADC_HIP_LIB=lib) if lib else dict(os.environ)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith(tag)]
    if r.returncode != 0 or not lines:
        print("step %s failed (exit %d): %s" % (" ".join(cmd[-6:]), r.returncode, (r.stdout + r.stderr)[-2000:]), flush=True)
        sys.exit(1)  # (nothing more is started on the GPU behind a step that failed)
    print("step %s ok" % " ".join(cmd[-6:]), flush=True)
    return json.loads(lines[-1] if tag == "{" else lines[-1][len(tag):])  # (bench.py prints its JSON object bare)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--map", default="noise")
    ap.add_argument("--form", default="plain")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--new-commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_timing.md"))
    ap.add_argument("--prof-dir", default="", help="where rocprofv3 writes (default: a temporary directory)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    a.prof_dir = a.prof_dir or tempfile.mkdtemp(prefix="voxel_prof_")
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--seconds", str(a.seconds)]
    md = ["# Voxel-grid filter of the cloud: timing on one MI355X, 1920x1080, D = 128", "",
          "`tools/voxel_timing.py`; parent build %s, this build %s.  Maps: the final maps of the benchmark's noise and structured pairs; calibration "
          "f = %g px, B = %g, doffs = 0; leaves %g (near a pixel's footprint at the near end) and %g; every comparison alternates its sides, %d repetitions."
          % (a.parent_commit, a.new_commit, CALIB[0], CALIB[1], LEAVES["small"], LEAVES["large"], a.reps), ""]
    # ---- the whole call
    res = run(me + ["--child", "reproject"], 300)
    md += ["## Cloud-only `adc_reproject_device`, ms per call (20 calls back to back, one `adc_wait`, best of 5; one figure per repetition)", "",
           "| map | form | records | points kept | ms per call | median |", "|---|---|---|---|---|---|"]
    for name in ("noise", "structured"):
        for which in ("plain", "small", "large"):
            v = res["%s %s" % (name, which)]
            kept = res.get("%s %s report" % (name, which), {}).get("points_kept", "")
            md.append("| %s | %s | %d | %s | %s | %.4f |" % (name, "plain cloud" if which == "plain" else "voxel, leaf %g" % LEAVES[which], res["%s %s count" % (name, which)],
                                                        kept, " ".join("%.4f" % x for x in v), statistics.median(v)))
    # ---- kernels alone, under the profiler
    md += ["", "## Kernels alone (`rocprofv3 --kernel-trace --stats`, one run per row, average over 20 launches), ms per launch", "",
           "| map | form | " + " | ".join(KERNELS) + " | sum | run sets of atomics at most | atomics / ns at most |", "|---|---|" + "---|" * (len(KERNELS) + 3)]
    for name in ("noise", "structured"):
        for which in ("plain", "small", "large"):
            d = os.path.join(a.prof_dir, "%s_%s" % (name, which))
            run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "vox", "--output-format", "csv", "--"] + me + ["--child", "kernel", "--map", name, "--form", which], 300)
            avg = {}
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    for k in KERNELS:
                        if k in row.get("Name", ""):
                            avg[k] = float(row["AverageNs"]) / 1e6
            cells = ["%.4f" % avg[k] if k in avg else "" for k in KERNELS]
            kept = res.get("%s %s report" % (name, which), {}).get("points_kept")
            # at most one set of 8 atomics (1 compare-and-swap claim aside) per kept pixel; runs of equal keys inside a wave issue one set
            rate = "%.1f" % (8 * kept / (avg["k_vox_insert"] * 1e6)) if kept and "k_vox_insert" in avg else ""
            md.append("| %s | %s | %s | %.4f | %s | %s |" % (name, which, " | ".join(cells), sum(avg.values()), kept if kept else "", rate))
    # ---- the farm
    res = run(me + ["--child", "farm"], 600)
    md += ["", "## Farm, %d pipelines, host delivery (`adc_farm_submit_products`), pairs/s (windows of at least %.0f s)" % (PIPES, a.seconds), "",
           "| pair | request | records per pair | pairs/s per repetition | median |", "|---|---|---|---|---|"]
    for name in ("noise", "structured"):
        for which, label in (("none", "no product"), ("cloud", "cloud, capacity W*H"), ("voxel", "voxel cloud, leaf %g, capacity W*H" % LEAVES["large"])):
            v = res["%s %s" % (name, which)]
            md.append("| %s | %s | %s | %s | %.1f |" % (name, label, res.get("%s %s count" % (name, which), ""), " ".join("%.1f" % x for x in v), statistics.median(v)))
    # ---- the plain headline against the parent
    md += ["", "## Plain headline (`bench.py --gpus 1 --steps %d --warmup 5`), pairs/s, parent against this build, alternating" % a.bench_steps, ""]
    if a.parent_lib:
        new_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip.so")
        vals = {"parent": [], "new": []}
        for _ in range(a.reps):
            for tag, lib in (("parent", a.parent_lib), ("new", new_lib)):
                o = run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "5", "--no-cpu-baseline"], 300, lib=lib, tag="{")
                vals[tag].append(o["value"])
        p, n = vals["parent"], vals["new"]
        med = statistics.median(n)
        verdict = "yes" if min(p) <= med <= max(p) else ("above it" if med > max(p) else "NO, below it")
        md += ["| parent repetitions | parent min - max | new repetitions | new median | inside the parent's spread |", "|---|---|---|---|---|",
               "| %s | %.2f - %.2f | %s | %.2f | %s |" % (" ".join("%.2f" % v for v in p), min(p), max(p), " ".join("%.2f" % v for v in n), med, verdict)]
    else:
        md.append("not measured (no parent library given)")
    text = "\n".join(md) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
