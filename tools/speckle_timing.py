#!/usr/bin/env python3
"""Cost of the optional speckle filter (k_speckle.hip).

    python tools/speckle_timing.py [--alternations 5] [--reps 10] [--sizes 1920x1080,1242x375] [--workloads noise,structured]
                                   [--size 200] [--diff 1.0] [--out FILE]

Per size and workload, device-resident inputs and outputs, each Match timed on the host from enqueue to adc_wait, on ONE handle:
`--alternations` rounds of `--reps` plain adc_match_device, then `--reps` with the filter switched on; the figure is the median over
rounds of (filtered - plain).  Then the four kernels alone: adc_filter_speckles_device on the delivered unfiltered map (uploaded
again before every call, outside the timed region; host time of enqueue + adc_wait, which includes the launch latencies), next to
the yardstick adc_device_copy_kernel_ms over one map (4 P bytes read + 4 P written).  At the first size also the synthetic maps
of tests/speckle_patterns.py with the longest paths (serpentine, spiral, comb) and the most components (checkerboards).
What each kernel has to move at least, P = W * H: k_spk_runs reads 4 P (map), writes 8 P (parent, size); k_spk_merge reads 4 P (map;
the upper row comes from the cache) and touches the parents of the pixels it unites; k_spk_flatten reads 4 P (parent), writes up to
4 P (parent) and the sizes at the roots; k_spk_apply reads 8 P (map, parent) and the sizes at the roots, writes 4 P out of place.
One JSON line at the end.  Under `rocprofv3 --kernel-trace --stats -- python tools/speckle_timing.py --trace-only on|off` one process
runs a few Matches with the filter on (the table lists k_spk_*) or on a handle that never had it set (exactly the parent's kernels)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, st, A):
    t0 = time.perf_counter()
    ok = fn() and st.wait()
    t1 = time.perf_counter()
    assert ok, A.last_error()
    return (t1 - t0) * 1e3


def _setup(w, h, d, workload):
    import adcensus_amd as A
    from adcensus_amd import workloads
    L = A.lib()
    left, right = workloads.noise_pair(w, h, 12345) if workload == "noise" else workloads.structured_pair(w, h, d, seed=777)
    n = w * h
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, 4 * n)]
    assert all(bufs), "adc_device_malloc failed"
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, A.ADCensusOption(max_disparity=d)), A.last_error()
    assert L.adc_memcpy_h2d(bufs[0], np.ascontiguousarray(left).ctypes.data, 3 * n) == 0
    assert L.adc_memcpy_h2d(bufs[1], np.ascontiguousarray(right).ctypes.data, 3 * n) == 0
    return A, L, st, bufs


def _alone(A, L, st, pd, pl, disp, size, diff, reps):
    """median host ms of adc_filter_speckles_device + adc_wait on `disp` (uploaded before every call), and the stats"""
    d = np.ascontiguousarray(disp, np.float32)
    ts = []
    for r in range(reps + 3):
        assert L.adc_memcpy_h2d(pd, d.ctypes.data, d.nbytes) == 0
        t = _timed(lambda: st.filter_speckles_device(pd, size, diff, pl), st, A)
        if r >= 3:
            ts.append(t)
    return statistics.median(ts), st.speckle_stats()


def measure(w, h, d, workload, alternations, reps, size, diff, synthetic):
    A, L, st, bufs = _setup(w, h, d, workload)
    dl, dr, dd, pl = bufs
    n = w * h
    run = lambda: st.match_device(dl, dr, dd)  # noqa: E731
    rounds = []
    for _ in range(alternations):
        st.set_speckle_filter(0, 0.0)
        for _ in range(3):
            _timed(run, st, A)
        plain = statistics.median(_timed(run, st, A) for _ in range(reps))
        st.set_speckle_filter(size, diff)
        for _ in range(3):
            _timed(run, st, A)
        rounds.append((plain, statistics.median(_timed(run, st, A) for _ in range(reps))))
    stats = st.speckle_stats()
    st.set_speckle_filter(0, 0.0)
    _timed(run, st, A)
    disp = np.empty((h, w), np.float32)
    assert L.adc_memcpy_d2h(disp.ctypes.data, dd, 4 * n) == 0
    res = {"size": [w, h, d], "workload": workload, "params": [size, diff], "plain_ms": [round(p, 4) for p, _ in rounds],
           "filtered_ms": [round(f, 4) for _, f in rounds], "added_ms_median": round(statistics.median(f - p for p, f in rounds), 4),
           "stats": stats}
    res["alone_ms"], _ = _alone(A, L, st, dd, None, disp, size, diff, reps)
    res["alone_labels_ms"], _ = _alone(A, L, st, dd, pl, disp, size, diff, reps)
    a, b = L.adc_device_malloc(4 * n & ~15), L.adc_device_malloc(4 * n & ~15)
    res["copy_kernel_ms"] = float(L.adc_device_copy_kernel_ms(a, b, 4 * n & ~15, 20))
    L.adc_device_free(a)
    L.adc_device_free(b)
    res["synthetic"] = {}
    if synthetic:
        from tests.speckle_patterns import patterns
        pats = patterns(w, h)
        for name in ("serpentine", "spiral", "comb", "constant", "checker_valid_invalid", "checker_two_disparities"):
            m, s, df = pats[name]
            ms, sst = _alone(A, L, st, dd, None, m, s, df, reps)
            res["synthetic"][name] = {"alone_ms": round(ms, 4), "stats": sst}
    st.Release()
    for p in bufs:
        L.adc_device_free(p)
    for k in ("alone_ms", "alone_labels_ms", "copy_kernel_ms"):
        res[k] = round(res[k], 4)
    return res


def trace_only(w, h, d, workload, form, size, diff):
    A, L, st, bufs = _setup(w, h, d, workload)
    if form == "on":
        st.set_speckle_filter(size, diff)
    for _ in range(10):
        assert st.match_device(bufs[0], bufs[1], bufs[2]) and st.wait(), A.last_error()
    st.Release()
    for b in bufs:
        L.adc_device_free(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1920x1080,1242x375")
    ap.add_argument("--workloads", default="noise,structured")
    ap.add_argument("--disp", type=int, default=128)
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--diff", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the report lines to this file")
    ap.add_argument("--trace-only", default=None, choices=["on", "off"])
    a = ap.parse_args()
    lines, out = [], []
    first = True
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for wl in a.workloads.split(","):
            if a.trace_only:
                trace_only(w, h, a.disp, wl, a.trace_only, a.size, a.diff)
                continue
            r = measure(w, h, a.disp, wl, a.alternations, a.reps, a.size, a.diff, first)
            first = False
            out.append(r)
            lines.append("%dx%d D=%d %-10s (%d, %g): plain %s ms | filtered %s ms" % (w, h, a.disp, wl, a.size, a.diff, r["plain_ms"], r["filtered_ms"]))
            lines.append("    filtered - plain %.3f ms (median of %d rounds); components / removed components / removed pixels %s" % (
                r["added_ms_median"], a.alternations, r["stats"]))
            lines.append("    kernels alone (enqueue + wait): %.3f ms, with labels %.3f ms | copy kernel over one map (4 P read + 4 P written) %.4f ms" % (
                r["alone_ms"], r["alone_labels_ms"], r["copy_kernel_ms"]))
            for name, s in r["synthetic"].items():
                lines.append("    synthetic %-24s kernels alone %.3f ms, stats %s" % (name, s["alone_ms"], s["stats"]))
            print("\n".join(lines[-(3 + len(r["synthetic"])):]), flush=True)
    if a.trace_only:
        return
    lines.append(json.dumps({"speckle_timing": out}))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
