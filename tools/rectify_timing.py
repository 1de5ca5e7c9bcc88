#!/usr/bin/env python3
"""Cost of the optional rectification (k_rectify.hip).

    python tools/rectify_timing.py [--alternations 5] [--reps 10] [--sizes 1920x1080,1242x375] [--workloads structured,noise]
                                   [--disp 128] [--out FILE]

Per size:
  * k_rect_remap alone, per source format, on the example lens model (tests/rectify_ref.py: example_model, source = destination size
    + 128 x 72): HIP-event-free host timing would be dominated by the launch, so the remap is enqueued `--batch` times back to back
    (adc_rectify_device) and the wall time to adc_wait divided by the batch; bytes = records 8 P + output 3 P + the source image once;
    next to the yardstick adc_device_copy_kernel_ms over the same byte count (half read, half written) in the same process.
  * per workload, device-resident inputs and outputs, each Match timed on the host from enqueue to adc_wait on ONE handle:
    `--alternations` rounds of `--reps` plain adc_match_device on the rectified pair, then `--reps` with rectification on and the
    raw pair; the figure is the median over rounds of (on - off).  The same for the host entry point adc_match (pageable arrays).
One JSON line at the end.  Under `rocprofv3 --kernel-trace --stats -- python tools/rectify_timing.py --trace-only on|off` one process
runs a few Matches with rectification on (the table lists k_rect_*) or on a handle that never had a side set (the parent's kernels).
The clock state is not read."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMATS = ["BGR8", "RGB8", "GRAY8", "BGRA8"]


def _timed(fn, st, A):
    t0 = time.perf_counter()
    ok = fn() and st.wait()
    t1 = time.perf_counter()
    assert ok, A.last_error()
    return (t1 - t0) * 1e3


def _raws(A, RR, pair, w, h, fmts):
    """the pair warped into raw frames (w + 128) x (h + 72) under second_model, packed -> per side (bytes, RawFormat, model dict)"""
    ws, hs = w + 128, h + 72
    out = []
    for img, fmt in zip(pair, fmts):
        frame = RR.remap(img, w, h, w * 3, RR.BGR8, *RR.model_maps(RR.second_model(w, h, ws, hs), ws, hs))[0]
        raw = RR.pack_source(frame, fmt)
        out.append((raw, A.RawFormat(ws, hs, raw.shape[1], fmt), RR.example_model(ws, hs, w, h)))
    return out


def _pair(workloads, w, h, d, workload):
    return workloads.noise_pair(w, h, 12345) if workload == "noise" else workloads.structured_pair(w, h, d, seed=777)


def remap_alone(w, h, d, reps, batch):
    import adcensus_amd as A
    from adcensus_amd import workloads
    from tests import rectify_ref as RR
    L = A.lib()
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, A.ADCensusOption(max_disparity=d)), A.last_error()
    left, _ = _pair(workloads, w, h, d, "structured")
    res = {}
    for fmt, name in enumerate(FORMATS):
        raw, rf, model = _raws(A, RR, (left,), w, h, (fmt,))[0]
        st.set_rectify_model(A.SIDE_LEFT, rf, A.CameraModel(**model))
        valid = float(st.rectify_maps(A.SIDE_LEFT)[2].mean())
        pr, po = L.adc_device_malloc(raw.nbytes), L.adc_device_malloc(3 * w * h)
        assert pr and po and L.adc_memcpy_h2d(pr, raw.ctypes.data, raw.nbytes) == 0

        def run():
            ok = True
            for _ in range(batch):
                ok = ok and st.rectify_device(A.SIDE_LEFT, pr, po)
            return ok

        for _ in range(3):
            _timed(run, st, A)
        ts = sorted(_timed(run, st, A) / batch for _ in range(reps))
        single = sorted(_timed(lambda: st.rectify_device(A.SIDE_LEFT, pr, po), st, A) for _ in range(reps))
        nbytes = 8 * w * h + 3 * w * h + raw.nbytes
        cb = (nbytes // 2) & ~15
        a, b = L.adc_device_malloc(cb), L.adc_device_malloc(cb)
        copy_ms = float(L.adc_device_copy_kernel_ms(a, b, cb, 20))
        for p in (a, b, pr, po):
            L.adc_device_free(p)
        res[name] = {"us_median": round(1e3 * statistics.median(ts), 2), "us_min": round(1e3 * ts[0], 2), "single_call_us_median": round(1e3 * statistics.median(single), 2),
                     "bytes": nbytes, "tb_per_s": round(nbytes / (statistics.median(ts) * 1e-3) / 1e12, 3), "copy_kernel_us": round(1e3 * copy_ms, 2),
                     "copy_tb_per_s": round(2 * cb / (copy_ms * 1e-3) / 1e12, 3), "valid_fraction": round(valid, 4)}
    st.Release()
    return res


def match_on_off(w, h, d, workload, alternations, reps):
    import adcensus_amd as A
    from adcensus_amd import workloads
    from tests import rectify_ref as RR
    L = A.lib()
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, A.ADCensusOption(max_disparity=d)), A.last_error()
    pair = _pair(workloads, w, h, d, workload)
    raws = _raws(A, RR, pair, w, h, (RR.BGR8, RR.BGR8))

    def on():
        for side, (_, rf, model) in enumerate(raws):
            st.set_rectify_model(side, rf, A.CameraModel(**model))

    on()
    rect = [st.rectify(raws[s][0], s) for s in (0, 1)]
    n = w * h
    dev = [L.adc_device_malloc(a.nbytes) for a in (rect[0], rect[1], raws[0][0], raws[1][0])] + [L.adc_device_malloc(4 * n)]
    for p, a in zip(dev, (rect[0], rect[1], raws[0][0], raws[1][0])):
        assert p and L.adc_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
    out = np.empty((h, w), np.float32)
    forms = {"device": (lambda: st.match_device(dev[0], dev[1], dev[4]), lambda: st.match_device(dev[2], dev[3], dev[4])),
             "host": (lambda: st.Match(rect[0], rect[1], out), lambda: st.Match(raws[0][0], raws[1][0], out))}
    res = {"size": [w, h, d], "workload": workload}
    for name, (off_fn, on_fn) in forms.items():
        rounds = []
        for _ in range(alternations):
            st.clear_rectify()
            for _ in range(3):
                _timed(off_fn, st, A)
            t_off = statistics.median(_timed(off_fn, st, A) for _ in range(reps))
            on()
            for _ in range(3):
                _timed(on_fn, st, A)
            rounds.append((t_off, statistics.median(_timed(on_fn, st, A) for _ in range(reps))))
        res[name] = {"off_ms": [round(a, 4) for a, _ in rounds], "on_ms": [round(b, 4) for _, b in rounds],
                     "added_ms_median": round(statistics.median(b - a for a, b in rounds), 4)}
    st.Release()
    for p in dev:
        L.adc_device_free(p)
    return res


def trace_only(w, h, d, form):
    import adcensus_amd as A
    from adcensus_amd import workloads
    L = A.lib()
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, A.ADCensusOption(max_disparity=d)), A.last_error()
    pair = _pair(workloads, w, h, d, "structured")
    if form == "on":
        from tests import rectify_ref as RR
        raws = _raws(A, RR, pair, w, h, (RR.BGR8, RR.BGRA8))
        for side, (_, rf, model) in enumerate(raws):
            st.set_rectify_model(side, rf, A.CameraModel(**model))
        images = [r[0] for r in raws]
    else:
        images = [np.ascontiguousarray(p) for p in pair]
    bufs = [L.adc_device_malloc(a.nbytes) for a in images] + [L.adc_device_malloc(4 * w * h)]
    for p, a in zip(bufs, images):
        assert p and L.adc_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
    for _ in range(10):
        assert st.match_device(bufs[0], bufs[1], bufs[2]) and st.wait(), A.last_error()
    st.Release()
    for b in bufs:
        L.adc_device_free(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--sizes", default="1920x1080,1242x375")
    ap.add_argument("--workloads", default="structured,noise")
    ap.add_argument("--disp", type=int, default=128)
    ap.add_argument("--out", default=None, help="also write the report lines to this file")
    ap.add_argument("--trace-only", default=None, choices=["on", "off"])
    a = ap.parse_args()
    lines, out = [], {"remap": {}, "match": []}
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        if a.trace_only:
            trace_only(w, h, a.disp, a.trace_only)
            continue
        r = remap_alone(w, h, a.disp, a.reps, a.batch)
        out["remap"][size] = r
        for name, v in r.items():
            lines.append("%s k_rect_remap %-5s: %.1f us median (min %.1f; one call enqueue + wait %.1f us), %d bytes, %.2f TB/s | copy kernel over the same bytes "
                         "%.1f us, %.2f TB/s | valid %.2f %%" % (size, name, v["us_median"], v["us_min"], v["single_call_us_median"], v["bytes"], v["tb_per_s"],
                                                                 v["copy_kernel_us"], v["copy_tb_per_s"], 100 * v["valid_fraction"]))
        print("\n".join(lines[-len(r):]), flush=True)
        for wl in a.workloads.split(","):
            m = match_on_off(w, h, a.disp, wl, a.alternations, a.reps)
            out["match"].append(m)
            for form in ("device", "host"):
                lines.append("%s D=%d %-10s %-6s: off %s ms | on %s ms | on - off %.3f ms (median of %d rounds)" % (
                    size, a.disp, wl, form, m[form]["off_ms"], m[form]["on_ms"], m[form]["added_ms_median"], a.alternations))
            print("\n".join(lines[-2:]), flush=True)
    if a.trace_only:
        return
    lines.append(json.dumps({"rectify_timing": out}))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
