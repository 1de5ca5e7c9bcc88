#!/usr/bin/env python3
"""Cost of the optional per-pixel maps: adc_match_device against adc_match_device_ex (provenance + confidence), interleaved on
one handle -- `--alternations` rounds of `--reps` plain Matches then `--reps` Matches with both maps, each timed on the host from
enqueue to adc_wait (device-resident inputs and outputs).  Prints one line per pair and geometry: median ms of each form per
round, the median over rounds of (ex - plain), and one JSON line at the end.

    python tools/extras_timing.py [--alternations 5] [--reps 10] [--sizes 1920x1080,1242x375] [--workloads noise,structured]

Under `rocprofv3 --kernel-trace --stats -- python tools/extras_timing.py ...` the kernel table shows k_confidence / k_provenance
next to the pipeline's own kernels."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import adcensus_amd as A  # noqa: E402
from adcensus_amd import workloads  # noqa: E402


def run(w, h, d, workload, alternations, reps):
    L = A.lib()
    left, right = workloads.noise_pair(w, h, 12345) if workload == "noise" else workloads.structured_pair(w, h, d, seed=777)
    n = w * h
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, n, 4 * n)]
    assert all(bufs), "adc_device_malloc failed"
    dl, dr, dd, dp, dc = bufs
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, A.ADCensusOption(max_disparity=d)), A.last_error()
    try:
        assert L.adc_memcpy_h2d(dl, np.ascontiguousarray(left).ctypes.data, 3 * n) == 0
        assert L.adc_memcpy_h2d(dr, np.ascontiguousarray(right).ctypes.data, 3 * n) == 0

        def one(ex):
            t0 = time.perf_counter()
            ok = st.match_device_ex(dl, dr, dd, dp, dc) if ex else st.match_device(dl, dr, dd)
            ok = ok and st.wait()
            t1 = time.perf_counter()
            assert ok, A.last_error()
            return (t1 - t0) * 1e3

        for _ in range(5):  # warm-up: both forms, the handle's learned budgets settle
            one(False)
            one(True)
        rounds = []
        for _ in range(alternations):
            plain = statistics.median(one(False) for _ in range(reps))
            ex = statistics.median(one(True) for _ in range(reps))
            rounds.append((plain, ex))
        diffs = [e - p for p, e in rounds]
        res = {"size": [w, h, d], "workload": workload, "plain_ms": [round(p, 4) for p, _ in rounds],
               "ex_ms": [round(e, 4) for _, e in rounds], "ex_minus_plain_ms_median": round(statistics.median(diffs), 4)}
        print("%dx%d D=%d %-10s plain %s ms | ex %s ms | ex - plain (median of %d rounds) %.3f ms" % (
            w, h, d, workload, res["plain_ms"], res["ex_ms"], alternations, res["ex_minus_plain_ms_median"]), flush=True)
        return res
    finally:
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
    a = ap.parse_args()
    out = []
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for wl in a.workloads.split(","):
            out.append(run(w, h, a.disp, wl, a.alternations, a.reps))
    print(json.dumps({"extras_timing": out}), flush=True)


if __name__ == "__main__":
    main()
