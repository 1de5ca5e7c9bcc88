#!/usr/bin/env python3
"""Times the products paths (adc_farm_submit_products, adc_match_device_products, k_disp16) on one MI355X at 1920x1080, D = 128, on
the noise and the structured pair of the benchmark, 3 pipelines, and writes profiles/products_timing.md.

    python tools/products_timing.py --parent-lib DIR/libadcensus_hip.so --parent-commit HASH --new-commit HASH [--out profiles/products_timing.md]

The driver starts one child process per step (this file with --child ...), each with its own time limit, and stops at the first step
that fails.  A child selects its library with ADC_HIP_LIB, warms every shape up and times windows of at least --seconds of work.
  plain     adc_farm_submit throughput of the parent build and of this build, --reps repetitions each, alternating; the new median is
            judged against the min-max spread of the parent's own repetitions (there is no preset ratio)
  products  farm pairs/s with each product alone and with all of them, pageable and registered destinations, the cloud at capacity W*H
  device    adc_match_device_products + adc_wait against adc_match_device + adc_wait, ms per pair
  kernel    k_disp16 from a rocprofv3 --kernel-trace --stats run of its own, next to the copy kernel over the same 6 bytes per pixel"""
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
CALIB = (1050.0, 0.54, W / 2.0, H / 2.0, 0.0)
SETS = ["none", "provenance", "confidence", "depth", "cloud", "disp8", "disp16", "all"]


def pairs():
    from adcensus_amd import workloads
    return {"noise": workloads.noise_pair(W, H, 12345), "structured": workloads.structured_pair(W, H, D, 777)}


def arrays_for(A, which, registered):
    names = ["provenance", "confidence", "depth", "cloud", "disp8", "disp16"] if which == "all" else ([] if which == "none" else [which])
    dts = dict(provenance=np.uint8, confidence=np.float32, depth=np.float32, disp8=np.uint8, disp16=np.uint16)
    arr = {n: (np.zeros(N, A.POINT_DTYPE) if n == "cloud" else np.zeros((H, W), dts[n])) for n in names}
    disp = np.zeros((H, W), np.float32)
    if registered:
        for a in list(arr.values()) + [disp]:
            A.host_register(a)
    req = A.Products.from_arrays(calib=CALIB, disp16_scale=256.0, **arr) if names else None
    return disp, arr, req


def farm_rate(A, farm, pair, slots, seconds):
    """pairs/s of submit ... drain over a window of at least `seconds` (after a warm-up of two rounds)"""
    def round_():
        for disp, _, req in slots:
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
    P = pairs()
    if a.child == "plain":
        farm = A.PairFarm(W, H, opt, device=0, pipelines=PIPES)
        slots = [(np.zeros((H, W), np.float32), None, None) for _ in range(PIPES)]
        for name, pair in P.items():
            out[name] = farm_rate(A, farm, pair, slots, a.seconds)
        farm.close()
    elif a.child == "products":
        farm = A.PairFarm(W, H, opt, device=0, pipelines=PIPES)
        for name, pair in P.items():
            for which in SETS:
                for registered in ((False, True) if which in ("all", "cloud", "none") else (False,)):
                    slots = [arrays_for(A, which, registered) for _ in range(PIPES)]
                    out["%s %s %s" % (name, which, "registered" if registered else "pageable")] = farm_rate(A, farm, pair, slots, a.seconds)
                    for disp, arr, _ in slots:
                        for x in (list(arr.values()) + [disp]) if registered else []:
                            A.host_unregister(x)
        farm.close()
    elif a.child == "device":
        st = A.ADCensusStereo(device=0)
        assert st.Initialize(W, H, opt), A.last_error()
        sizes = dict(provenance=N, confidence=4 * N, depth=4 * N, cloud=16 * N, disp8=N, disp16=2 * N)
        p = {k: L.adc_device_malloc(v) for k, v in sizes.items()}
        dl, dr, dd, pn = (L.adc_device_malloc(s) for s in (3 * N, 3 * N, 4 * N, 16))
        req = A.Products.from_addresses(p["provenance"], p["confidence"], CALIB, p["depth"], p["cloud"], N, pn, p["disp8"], p["disp16"], 256.0)
        only16 = A.Products.from_addresses(disp16=p["disp16"], disp16_scale=256.0)
        for name, pair in P.items():
            for arr, ptr in ((pair[0], dl), (pair[1], dr)):
                assert L.adc_memcpy_h2d(ptr, np.ascontiguousarray(arr).ctypes.data, 3 * N) == 0
            for label, r in (("plain", None), ("disp16", only16), ("all", req)):
                call = (lambda: st.match_device(dl, dr, dd)) if r is None else (lambda: st.match_device_products(dl, dr, dd, r))
                for _ in range(3):
                    assert call() and st.wait(), A.last_error()
                n, t0 = 0, time.perf_counter()
                while time.perf_counter() - t0 < a.seconds:
                    assert call() and st.wait(), A.last_error()
                    n += 1
                out["%s %s" % (name, label)] = (time.perf_counter() - t0) * 1e3 / n
        st.Release()
    elif a.child == "kernel":  # (run under the profiler by the driver; the copy-kernel yardstick when --seconds is 0)
        st = A.ADCensusStereo(device=0)
        assert st.Initialize(W, H, opt), A.last_error()
        dd, po, ca, cb = (L.adc_device_malloc(s) for s in (4 * N, 2 * N, 16 * N, 16 * N))
        rng = np.random.default_rng(1)
        m = (rng.random((H, W), dtype=np.float32) * np.float32(128)).astype(np.float32)
        m[rng.random((H, W)) < 0.1] = np.inf
        assert L.adc_memcpy_h2d(dd, m.ctypes.data, 4 * N) == 0
        if a.seconds > 0:
            for _ in range(200):
                assert st.disp16_device(dd, 256.0, po)
            assert st.wait()
        else:
            out["copy_kernel_ms_same_bytes"] = L.adc_device_copy_kernel_ms(ca, cb, 6 * N // 2 // 16 * 16, 20)  # (3 bytes read + 3 written per pixel)
        st.Release()
    print("PRODUCTS_TIMING " + json.dumps(out), flush=True)


def run_child(step, lib, seconds, limit, prefix=()):
    env = dict(os.environ, ADC_HIP_LIB=lib) if lib else dict(os.environ)
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", step, "--seconds", str(seconds)]
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("PRODUCTS_TIMING ")]
    if r.returncode != 0 or not lines:
        print("step %s failed (exit %d): %s" % (step, r.returncode, (r.stdout + r.stderr)[-2000:]), flush=True)
        sys.exit(1)  # (nothing more is started on the GPU behind a step that failed)
    print("step %s %s ok" % (step, os.path.basename(os.path.dirname(lib)) if lib else ""), flush=True)
    return json.loads(lines[-1][len("PRODUCTS_TIMING "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--new-commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "products_timing.md"))
    ap.add_argument("--prof-dir", default="", help="where rocprofv3 writes (default: a temporary directory)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    a.prof_dir = a.prof_dir or tempfile.mkdtemp(prefix="products_prof_")
    new_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip.so")
    md = ["# Products: timing on one MI355X, 1920x1080, D = 128, %d pipelines" % PIPES, "",
          "`tools/products_timing.py`; windows of at least %.0f s after a warm-up; parent build %s, this build %s." % (a.seconds, a.parent_commit, a.new_commit), ""]
    # ---- plain farm: parent against this build, alternating
    md += ["## Plain farm (`adc_farm_submit`), pairs/s", ""]
    if a.parent_lib:
        runs = {"parent": [], "new": []}
        for _ in range(a.reps):
            for tag, lib in (("parent", a.parent_lib), ("new", new_lib)):
                runs[tag].append(run_child("plain", lib, a.seconds, 240))
        md += ["| pair | parent repetitions | parent min - max | new repetitions | new median | inside the parent's spread |", "|---|---|---|---|---|---|"]
        for pair in ("noise", "structured"):
            p, n = [r[pair] for r in runs["parent"]], [r[pair] for r in runs["new"]]
            med = statistics.median(n)
            verdict = "yes" if min(p) <= med <= max(p) else ("above it" if med > max(p) else "NO, below it")
            md.append("| %s | %s | %.1f - %.1f | %s | %.1f | %s |" % (pair, " ".join("%.1f" % v for v in p), min(p), max(p), " ".join("%.1f" % v for v in n), med, verdict))
    else:
        md.append("not measured (no parent library given)")
    # ---- product costs
    res = run_child("products", new_lib, a.seconds, 600)
    md += ["", "## Farm with products (`adc_farm_submit_products`), pairs/s", "", "The cloud has capacity W*H and is copied by adc_wait once the count is known "
           "(min(count, capacity) points, device to the caller's memory); a stream-ordered copy of the whole capacity through pinned staging was not measured.", "",
           "| products | destinations | noise | structured |", "|---|---|---|---|"]
    for which in SETS:
        for dest in ("pageable", "registered"):
            if "noise %s %s" % (which, dest) in res:
                md.append("| %s | %s | %.1f | %.1f |" % (which, dest, res["noise %s %s" % (which, dest)], res["structured %s %s" % (which, dest)]))
    dev = run_child("device", new_lib, a.seconds, 300)
    md += ["", "## Device-resident (`adc_match_device` / `adc_match_device_products` + `adc_wait`), ms per pair", "", "| request | noise | structured |", "|---|---|---|"]
    for label in ("plain", "disp16", "all"):
        md.append("| %s | %.3f | %.3f |" % (label, dev["noise " + label], dev["structured " + label]))
    # ---- the kernel alone, under the profiler (everything above ran without it)
    md += ["", "## k_disp16 alone", ""]
    copy = run_child("kernel", new_lib, 0, 300)["copy_kernel_ms_same_bytes"]
    run_child("kernel", new_lib, 1, 600, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", a.prof_dir, "-o", "disp16", "--output-format", "csv", "--"))
    avg = None
    for path in glob.glob(os.path.join(a.prof_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "k_disp16" in row.get("Name", ""):
                avg = float(row["AverageNs"]) / 1e6
    if avg is None:
        md.append("k_disp16 under rocprofv3: not measured (no kernel_stats.csv row); copy kernel over the same %d bytes: %.4f ms" % (6 * N, copy))
    else:
        md.append("k_disp16 (rocprofv3 --kernel-trace --stats, 200 launches): %.4f ms average for %d bytes (4 read + 2 written per pixel), %.2f TB/s; "
                  "`adc_device_copy_kernel_ms` over the same bytes: %.4f ms, ratio %.2f." % (avg, 6 * N, 6 * N / avg / 1e9, copy, avg / copy))
    text = "\n".join(md) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
