#!/usr/bin/env python3
"""Times the ground-truth evaluation (adc_evaluate_device: memset of the report words, k_eval_measure, pinned read-back) on one
MI355X next to the copy-kernel yardstick over the same number of bytes.  Writes the lines it prints to --out.

    python tools/eval_timing.py [--sizes 1920x1080,1242x375] [--batch 50] [--reps 7] [--out profiles/eval_timing.txt]

Per size: N evaluations enqueued back to back on the handle's stream, one adc_wait, best of `reps` -- once with every input
(provenance, confidence) and both per-pixel outputs (19 bytes per pixel), once with the report only (d, g and the occlusion byte: 9
bytes per pixel), once with the report only but provenance and confidence read (14).  The rocprofv3 kernel table next to this file
(profiles/eval_kernel_stats.md) has the kernel alone."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adcensus_amd as A  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,1242x375")
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = A.lib()
    lines = ["# tools/eval_timing.py --sizes %s --batch %d --reps %d (one MI355X; %s)" % (a.sizes, a.batch, a.reps, L.adc_version().decode())]
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        n = w * h
        rng = np.random.default_rng(1)
        g = (rng.random((h, w)) * 100).astype(np.float32)
        g[rng.random((h, w)) < 0.05] = np.nan
        d = (np.nan_to_num(g) + rng.normal(0, 1.0, (h, w))).astype(np.float32)
        d[rng.random((h, w)) < 0.05] = np.inf
        prov = rng.choice(np.array([0, 0, 0, 0, 0, 0, 5, 6, 9, 10], np.uint8), (h, w))
        conf = rng.random((h, w)).astype(np.float32)
        st = A.ADCensusStereo(device=0)
        assert st.Initialize(w, h, A.ADCensusOption(max_disparity=16)), A.last_error()
        st.set_ground_truth(g, np.roll(g, -3, axis=1))
        bufs = [L.adc_device_malloc(s) for s in (4 * n, n, 4 * n, 4 * n, n, 16 * n, 16 * n)]
        dd, dp, dc, de, dk, ca, cb = bufs
        for arr, p in ((d, dd), (prov, dp), (conf, dc)):
            assert L.adc_memcpy_h2d(p, np.ascontiguousarray(arr).ctypes.data, arr.nbytes) == 0
        variants = (("all inputs, err + class", (dd, dp, dc, (1.0,), de, dk), 19), ("report only", (dd, None, None, (1.0,), None, None), 9),
                    ("report only, provenance + confidence", (dd, dp, dc, (1.0,), None, None), 14))
        lines.append("%dx%d" % (w, h))
        for name, args, bpp in variants:
            params = A.EvalParams(args[3])
            call = (args[0], args[1], args[2], params, args[4], args[5])
            best = 1e9
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                for _ in range(a.batch):
                    assert st.evaluate_device(*call), A.last_error()
                assert st.wait(), A.last_error()
                best = min(best, (time.perf_counter() - t0) * 1e3 / a.batch)
            one = 1e9
            for _ in range(a.reps):
                t0 = time.perf_counter()
                assert st.evaluate_device(*call) and st.wait()
                one = min(one, (time.perf_counter() - t0) * 1e3)
            traffic = bpp * n
            copy_ms = L.adc_device_copy_kernel_ms(ca, cb, traffic // 2 // 16 * 16, 20)  # (reads and writes: the same bytes moved in total)
            lines.append("    %-38s %.4f ms per evaluation back to back, %.4f ms enqueue + wait | %d bytes moved, %.2f TB/s | copy kernel over the same bytes %.4f ms, ratio %.2f"
                         % (name, best, one, traffic, traffic / best / 1e9, copy_ms, best / copy_ms))
        rep = st.eval_report()
        lines.append("    (known %d, invalid %d, bad > 1: %d)" % (rep.all.pixels, rep.all.invalid, rep.all.bad[0]))
        for b in bufs:
            L.adc_device_free(b)
        st.Release()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
