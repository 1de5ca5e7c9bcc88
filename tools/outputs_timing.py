#!/usr/bin/env python3
"""Cost of the outputs computed from the final map (depth + point cloud + 8-bit image, k_outputs.hip).

    python tools/outputs_timing.py [--parent-lib PATH] [--alternations 5] [--reps 10] [--sizes 1920x1080,1242x375]
                                   [--workloads noise,structured] [--out profiles/outputs_timing.txt]

Per size and workload, device-resident inputs and outputs, each Match timed on the host from enqueue to adc_wait:
  * `--alternations` rounds, each: a child process with the PARENT revision's library (--parent-lib, loaded through ADC_HIP_LIB)
    runs `--reps` plain adc_match_device, then a child with this tree's library runs `--reps` plain adc_match_device and `--reps`
    adc_match_device_out with all three outputs.  The figure is the median over rounds of (out - parent plain); this tree's plain
    Match next to the parent's shows that the plain path did not move.  Without --parent-lib only this tree's two forms are timed.
  * the three kernels alone: adc_reproject_device on the delivered map, all outputs and each output alone (host time of enqueue +
    adc_wait, which includes the launch latencies), next to the yardstick for the cloud: adc_device_copy_kernel_ms over the bytes
    the cloud moves, 4 P + 3 P read and 16 * count written.
One JSON line at the end.  Under `rocprofv3 --kernel-trace --stats -- python tools/outputs_timing.py --trace-only out|plain` one
process runs a few Matches of one form, so that the kernel table lists k_out_* (or, for `plain`, exactly the parent's kernels)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALIB = (1050.0, 0.54, 960.0, 540.0, 0.0)


def _setup(w, h, d, workload):
    import adcensus_amd as A
    from adcensus_amd import workloads
    L = A.lib()
    left, right = workloads.noise_pair(w, h, 12345) if workload == "noise" else workloads.structured_pair(w, h, d, seed=777)
    n = w * h
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, 4 * n, 16 * n, 16, n)]
    assert all(bufs), "adc_device_malloc failed"
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, A.ADCensusOption(max_disparity=d)), A.last_error()
    assert L.adc_memcpy_h2d(bufs[0], np.ascontiguousarray(left).ctypes.data, 3 * n) == 0
    assert L.adc_memcpy_h2d(bufs[1], np.ascontiguousarray(right).ctypes.data, 3 * n) == 0
    return A, L, st, bufs


def _timed(fn, st, A):
    t0 = time.perf_counter()
    ok = fn() and st.wait()
    t1 = time.perf_counter()
    assert ok, A.last_error()
    return (t1 - t0) * 1e3


def child(w, h, d, workload, reps, forms):
    """one process, one library: `reps` Matches of each form after a warm-up; prints a JSON line {form: median ms}"""
    A, L, st, bufs = _setup(w, h, d, workload)
    dl, dr, dd, pz, pc, pn, pg = bufs
    n = w * h
    run = {"plain": lambda: st.match_device(dl, dr, dd),
           "out": lambda: st.match_device_out(dl, dr, dd, CALIB, pz, pc, n, pn, pg)}
    res = {}
    for form in forms:
        for _ in range(5):
            _timed(run[form], st, A)
        res[form] = statistics.median(_timed(run[form], st, A) for _ in range(reps))
    if "out" in forms:  # the kernels alone, on the map the last Match delivered
        res["count"] = st.cloud_count()
        alone = {"all": (CALIB, pz, pc, pg), "depth": (CALIB, pz, None, None), "cloud": (CALIB, None, pc, None), "disp8": (None, None, None, pg)}
        for name, (cal, z, c, g) in alone.items():
            fn = lambda: st.reproject_device(dd, dl, cal, z, c, n, pn if c else None, g)  # noqa: E731
            for _ in range(5):
                _timed(fn, st, A)
            res["reproject_" + name] = statistics.median(_timed(fn, st, A) for _ in range(reps))
        moved = 7 * n + 16 * res["count"]
        half = moved // 2 & ~15  # (a copy of B bytes moves 2 B; the copy kernel wants multiples of 16)
        a, b = L.adc_device_malloc(half), L.adc_device_malloc(half)
        res["cloud_bytes"] = moved
        res["copy_kernel_ms"] = float(L.adc_device_copy_kernel_ms(a, b, half, 20))
        L.adc_device_free(a)
        L.adc_device_free(b)
    st.Release()
    for b in bufs:
        L.adc_device_free(b)
    print("CHILD " + json.dumps(res), flush=True)


def _spawn(args, lib=None):
    env = dict(os.environ)
    if lib:
        env["ADC_HIP_LIB"] = lib
    else:
        env.pop("ADC_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError("child failed (%d): %s" % (out.returncode, out.stdout[-1000:] + out.stderr[-2000:]))
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("CHILD ")][-1]
    return json.loads(line[6:])


def measure(w, h, d, workload, alternations, reps, parent_lib):
    base = ["--child", "%dx%d" % (w, h), "--disp", str(d), "--workloads", workload, "--reps", str(reps)]
    rounds = []
    for _ in range(alternations):
        parent = _spawn(base + ["--forms", "plain"], parent_lib)["plain"] if parent_lib else None
        rounds.append((parent, _spawn(base + ["--forms", "plain,out"])))
    last = rounds[-1][1]
    res = {"size": [w, h, d], "workload": workload, "parent_plain_ms": [None if p is None else round(p, 4) for p, _ in rounds],
           "plain_ms": [round(r["plain"], 4) for _, r in rounds], "out_ms": [round(r["out"], 4) for _, r in rounds],
           "out_minus_plain_ms_median": round(statistics.median(r["out"] - r["plain"] for _, r in rounds), 4),
           "count": last["count"], "cloud_bytes": last["cloud_bytes"]}
    if parent_lib:
        res["out_minus_parent_plain_ms_median"] = round(statistics.median(r["out"] - p for p, r in rounds), 4)
        res["plain_minus_parent_plain_ms_median"] = round(statistics.median(r["plain"] - p for p, r in rounds), 4)
    for key in ("reproject_all", "reproject_depth", "reproject_cloud", "reproject_disp8", "copy_kernel_ms"):
        res[key] = round(statistics.median(r[key] for _, r in rounds), 4)
    res["cloud_over_copy"] = round(res["reproject_cloud"] / res["copy_kernel_ms"], 2) if res["copy_kernel_ms"] > 0 else None
    return res


def trace_only(w, h, d, workload, form):
    A, L, st, bufs = _setup(w, h, d, workload)
    dl, dr, dd, pz, pc, pn, pg = bufs
    for _ in range(10):
        ok = st.match_device_out(dl, dr, dd, CALIB, pz, pc, w * h, pn, pg) if form == "out" else st.match_device(dl, dr, dd)
        assert ok and st.wait(), A.last_error()
    st.Release()
    for b in bufs:
        L.adc_device_free(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent-lib", default=None, help="libadcensus_hip.so built from the parent revision")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1920x1080,1242x375")
    ap.add_argument("--workloads", default="noise,structured")
    ap.add_argument("--disp", type=int, default=128)
    ap.add_argument("--out", default=None, help="also write the report lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--forms", default="plain,out", help=argparse.SUPPRESS)
    ap.add_argument("--trace-only", default=None, choices=["out", "plain"])
    a = ap.parse_args()
    if a.child:
        w, h = (int(v) for v in a.child.split("x"))
        return child(w, h, a.disp, a.workloads, a.reps, a.forms.split(","))
    lines, out = [], []
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for wl in a.workloads.split(","):
            if a.trace_only:
                trace_only(w, h, a.disp, wl, a.trace_only)
                continue
            r = measure(w, h, a.disp, wl, a.alternations, a.reps, a.parent_lib and os.path.abspath(a.parent_lib))
            out.append(r)
            lines.append("%dx%d D=%d %-10s parent plain %s ms | plain %s ms | out %s ms" % (w, h, a.disp, wl, r["parent_plain_ms"], r["plain_ms"], r["out_ms"]))
            lines.append("    out - plain %.3f ms, out - parent plain %s ms, plain - parent plain %s ms (medians of %d rounds)" % (
                r["out_minus_plain_ms_median"], r.get("out_minus_parent_plain_ms_median"), r.get("plain_minus_parent_plain_ms_median"), a.alternations))
            lines.append("    kernels alone (enqueue + wait): all %.3f ms, depth %.3f, cloud %.3f, disp8 %.3f | %d points, %d bytes moved, "
                         "copy kernel %.4f ms, cloud / copy %s" % (r["reproject_all"], r["reproject_depth"], r["reproject_cloud"], r["reproject_disp8"],
                                                                  r["count"], r["cloud_bytes"], r["copy_kernel_ms"], r["cloud_over_copy"]))
            print("\n".join(lines[-3:]), flush=True)
    if a.trace_only:
        return
    lines.append(json.dumps({"outputs_timing": out}))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
