#!/usr/bin/env python3
"""Break-even density of the sparse small-ring aggregation launches (GPU): 1080p noise pairs in which a growing share of the pixels
copies its left or its upper neighbour, each matched alternately with the dense form (ADC_AGG_SPARSE=0) and with the sparse form
forced (ADC_AGG_SPARSE_DENSITY=1) on one handle; the time is the aggregation stage's (HIP events).  The planted copies sit on every
third column / row only, so no arm outgrows the small ring.  Prints a markdown table; the committed threshold
(AGG_SPARSE_MAX_DENSITY, k_aggregate.hip) is half of the density at which the two forms take the same time.
    python tools/gpu_sparse_sweep.py [reps]
With `gather` as second argument the same pairs are matched alternately with the sparse march (ADC_AGG_GATHER=0) and with the gather
form of the sparse launches forced (ADC_AGG_GATHER_DENSITY=1), both with the sparse form forced: the table behind
AGG_GATHER_MAX_DENSITY (profiles/gather_agg_density_sweep.md).
    python tools/gpu_sparse_sweep.py [reps] gather
With `flat` the same pairs are matched alternately with the small-ring march as first launch (ADC_COST_FLAT=0) and with the
element-wise first launch forced (k_cost_agg_flat, ADC_COST_FLAT_DENSITY=1), sparse and gather forms forced for the other launches;
the time is the FIRST launch's, from the aggregation marks (debug counter 24): the table behind COST_FLAT_MAX_DENSITY
(profiles/flat_cost_density_sweep.md).
    python tools/gpu_sparse_sweep.py [reps] flat"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import adcensus_amd as A  # noqa: E402
from adcensus_amd import workloads  # noqa: E402


def planted(W, H, p, seed=12345):
    left, right = (a.copy() for a in workloads.noise_pair(W, H, seed=seed))
    rng = np.random.default_rng(seed + 7)
    src = left.copy()
    mh = rng.random((H, W)) < p
    mh[:, np.arange(W) % 3 != 1] = False
    mv = rng.random((H, W)) < p
    mv[np.arange(H) % 3 != 1, :] = False
    mv &= ~mh
    left[mh] = np.roll(src, 1, axis=1)[mh]
    left[mv] = np.roll(src, 1, axis=0)[mv]
    return np.ascontiguousarray(left), right


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    flat = len(sys.argv) > 2 and sys.argv[2] == "flat"
    gather = flat or (len(sys.argv) > 2 and sys.argv[2] == "gather")  # (flat: the pairs and the forced forms of the gather sweep)
    switch, counter = ("ADC_COST_FLAT", 22) if flat else ("ADC_AGG_GATHER", 20) if gather else ("ADC_AGG_SPARSE", 16)
    a, b = ("march", "flat") if flat else ("march", "gather") if gather else ("dense", "sparse")
    W, H, D = 1920, 1080, 128
    opt = A.ADCensusOption()
    opt.max_disparity = D
    rows = []
    print("| planted share p | density h | density v | %s ms (median, min) | %s ms (median, min) | %s - %s ms | %s launches per Match |" % (a, b, b, a, b))
    print("|---|---|---|---|---|---|---|")
    for p in ((0.0, 0.01, 0.03, 0.05, 0.08, 0.12, 0.15, 0.2, 0.25, 0.4, 0.55) if gather else (0.0, 0.03, 0.08, 0.15, 0.25, 0.4, 0.55, 0.7, 0.85, 1.0)):
        l, r = planted(W, H, p)
        st = A.ADCensusStereo(device=0)
        assert st.Initialize(W, H, opt)
        st.set_profiling(True)
        os.environ["ADC_AGG_SPARSE_DENSITY"] = os.environ["ADC_AGG_GATHER_DENSITY"] = "1.0"
        os.environ["ADC_AGG_SPARSE"] = "1" if gather else "0"
        os.environ["ADC_AGG_GATHER"] = "1" if flat else "0"
        os.environ["ADC_COST_FLAT_DENSITY"] = "1.0"
        os.environ["ADC_COST_FLAT"] = "0"
        st.match(l, r)  # (first Match of a handle: full ring)
        st.match(l, r)
        t = {"0": [], "1": []}
        launches = 0
        for _ in range(reps):
            for mode in ("0", "1"):
                os.environ[switch] = mode
                before = st.debug_counter(counter)
                st.match(l, r)
                t[mode].append(st.debug_counter(24) * 1e-6 if flat else st.stage_ms()["aggregate"])
                assert t[mode][-1] > 0
                ran = st.debug_counter(counter) - before
                assert (ran > 0) == (mode == "1"), (mode, ran, st.aggregate_kernel())
                launches = max(launches, ran)
        dh, dv = st.debug_counter(18) / float(W * H), st.debug_counter(19) / float(W * H)
        redos = st.debug_counter(2) + st.debug_counter(4)
        st.Release()
        md, ms = float(np.median(t["0"])), float(np.median(t["1"]))
        rows.append((max(dh, dv), ms - md))
        print("| %.2f | %.4f | %.4f | %.3f, %.3f | %.3f, %.3f | %+.3f | %d |%s" % (
            p, dh, dv, md, min(t["0"]), ms, min(t["1"]), ms - md, launches, " (redos: %d)" % redos if redos else ""), flush=True)
    be = None
    for (d0, y0), (d1, y1) in zip(rows, rows[1:]):
        if y0 < 0 <= y1:
            be = d0 + (d1 - d0) * (0 - y0) / (y1 - y0)
            break
    print("\nbreak-even density (linear interpolation, larger of the two directions): %s; half of it: %s" % (
        "%.3f" % be if be is not None else "not crossed", "%.3f" % (be / 2) if be is not None else "-"))


if __name__ == "__main__":
    main()
