#!/usr/bin/env python3
"""Cost of the optional rectification (k_rectify.hip).

    python tools/rectify_timing.py [--alternations 5] [--reps 10] [--sizes 1920x1080,1242x375] [--workloads structured,noise]
                                   [--disp 128] [--out FILE]
    python tools/rectify_timing.py --rawfmt [--alternations 3] [--batch 20] [--out profiles/rawfmt_timing.md]

Per size:
  * k_rect_remap alone, per source format, on the example lens model (tests/rectify_ref.py: example_model, source = destination size
    + 128 x 72): HIP-event-free host timing would be dominated by the launch, so the remap is enqueued `--batch` times back to back
    (adc_rectify_device) and the wall time to adc_wait divided by the batch; bytes = records 8 P + output 3 P + the source image once;
    next to the yardstick adc_device_copy_kernel_ms over the same byte count (half read, half written) in the same process.
  * per workload, device-resident inputs and outputs, each Match timed on the host from enqueue to adc_wait on ONE handle:
    `--alternations` rounds of `--reps` plain adc_match_device on the rectified pair, then `--reps` with rectification on and the
    raw pair; the figure is the median over rounds of (on - off).  The same for the host entry point adc_match (pageable arrays).
`--rawfmt` (a run of its own): every source layout at 1920 x 1080 -> 1920 x 1080 -- the remap under the example lens model and the
conversion-only kernel (adc_set_input_format), each timed from HIP events on the handle's stream around `--batch` launches, in
`--alternations` (at least three) interleaved repetitions of the whole list in one process, next to the BGR8 remap (whose generated code
is the parent revision's) and the best adc_device_copy_kernel_ms; then adc_match host to host in pairs/s on the structured pair handed
over as BGR8 (plain), as BAYER_RGGB8 and as NV12 through adc_set_input_format, interleaved the same way.  Writes a markdown table with
the priced bytes per destination pixel (remap: 8 record + 1 valid + 3 out + the source footprint; conversion: source + 3) and the clock
state as far as it can be read to `--out` (default profiles/rawfmt_timing.md).
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


# layout name -> (format word, source bytes per pixel)
RAW_LAYOUTS = [("BGR8", 0, 3.0), ("RGB8", 1, 3.0), ("GRAY8", 2, 1.0), ("BGRA8", 3, 4.0), ("GRAY16/12", 0x10 | (12 << 8), 2.0),
               ("BAYER_RGGB8", 0x20, 1.0), ("BAYER_GRBG8", 0x21, 1.0), ("BAYER_GBRG8", 0x22, 1.0), ("BAYER_BGGR8", 0x23, 1.0),
               ("BAYER_RGGB16/12", 0x30 | (12 << 8), 2.0), ("BAYER_GRBG16/10", 0x31 | (10 << 8), 2.0), ("BAYER_GBRG16/12", 0x32 | (12 << 8), 2.0),
               ("BAYER_BGGR16/10", 0x33 | (10 << 8), 2.0), ("YUYV", 0x40, 2.0), ("UYVY", 0x41, 2.0), ("NV12", 0x42, 1.5)]


class _Events:
    """HIP events on a handle's stream (adc_get_stream), through the runtime library the product library is linked with"""

    def __init__(self, stream):
        import ctypes as C
        self.C, self.hip, self.stream = C, C.CDLL("libamdhip64.so"), C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def ms(self, fn):
        assert self.hip.hipEventRecord(self.a, self.stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, self.stream) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        t = self.C.c_float(0)
        assert self.hip.hipEventElapsedTime(self.C.byref(t), self.a, self.b) == 0
        return float(t.value)


def _clock_state():
    import subprocess
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=60)
        keep = [l.strip() for l in r.stdout.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l or "fclk" in l or "Performance" in l)]
        return keep or ["not readable (rocm-smi printed nothing for GPU[0])"]
    except Exception as exc:  # noqa: BLE001
        return ["not readable (%s)" % exc]


def rawfmt(alternations, batch, out_path):
    import ctypes as C
    import adcensus_amd as A
    from adcensus_amd import workloads
    from tests import rawfmt_ref as RF
    from tests import rectify_ref as RR
    L = A.lib()
    L.adc_get_stream.restype = C.c_void_p
    L.adc_get_stream.argtypes = [C.c_void_p]
    w, h, d = 1920, 1080, 128
    P = w * h
    alternations = max(3, alternations)
    clocks = [_clock_state()]
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, A.ADCensusOption(max_disparity=d)), A.last_error()
    ev = _Events(L.adc_get_stream(st._h))
    left, right = workloads.structured_pair(w, h, d, seed=777)
    model = A.CameraModel(**RR.example_model(w, h, w, h))
    po = L.adc_device_malloc(3 * P)
    frames = {}
    for name, word, _ in RAW_LAYOUTS:
        raw = RF.pack(left, word)
        p = L.adc_device_malloc(raw.nbytes)
        assert p and L.adc_memcpy_h2d(p, raw.ctypes.data, raw.nbytes) == 0
        frames[name] = (p, A.RawFormat(w, h, 0, word))
    cb = 16 << 20
    ca, cbuf = L.adc_device_malloc(cb), L.adc_device_malloc(cb)
    times = {name: {"remap": [], "convert": []} for name, _, _ in RAW_LAYOUTS}
    copies = []

    def launches(p):
        for _ in range(batch):
            assert st.rectify_device(A.SIDE_LEFT, p, po), A.last_error()

    for _ in range(alternations):
        for name, _, _ in RAW_LAYOUTS:
            p, rf = frames[name]
            for kind in ("remap", "convert"):
                if kind == "remap":
                    st.set_rectify_model(A.SIDE_LEFT, rf, model)
                else:
                    st.set_input_format(A.SIDE_LEFT, rf)
                launches(p)
                assert st.wait()
                times[name][kind].append(ev.ms(lambda: launches(p)) / batch)
                assert st.wait()
        copies.append(float(L.adc_device_copy_kernel_ms(ca, cbuf, cb, 20)))
    valid = None
    st.set_rectify_model(A.SIDE_LEFT, frames["BGR8"][1], model)
    valid = float(st.rectify_maps(A.SIDE_LEFT)[2].mean())
    st.clear_rectify()
    # ---- the upload effect: adc_match host to host, the same frames as BGR8 (plain), BAYER_RGGB8 and NV12
    pairs = {"BGR8 (plain)": (None, np.ascontiguousarray(left), np.ascontiguousarray(right))}
    for name, word in (("BAYER_RGGB8", 0x20), ("NV12", 0x42)):
        pairs[name] = (A.RawFormat(w, h, 0, word), RF.pack(left, word), RF.pack(right, word))
    out = np.empty((h, w), np.float32)
    rates = {name: [] for name in pairs}
    reps = 10
    for _ in range(alternations):
        for name, (rf, l, r) in pairs.items():
            st.clear_rectify()
            if rf is not None:
                st.set_input_format(0, rf)
                st.set_input_format(1, rf)
            for _ in range(3):
                assert st.Match(l, r, out), A.last_error()
            t0 = time.perf_counter()
            for _ in range(reps):
                assert st.Match(l, r, out), A.last_error()
            rates[name].append(reps / (time.perf_counter() - t0))
    st.Release()
    for p in [po, ca, cbuf] + [f[0] for f in frames.values()]:
        L.adc_device_free(p)
    clocks.append(_clock_state())
    # ---- the report
    copy_ms = min(copies)
    copy_tbs = 2 * cb / (copy_ms * 1e-3) / 1e12
    base = min(times["BGR8"]["remap"])
    lines = ["# Camera layouts: remap and conversion-only kernels, 1920 x 1080 -> 1920 x 1080", "",
             "`python tools/rectify_timing.py --rawfmt --alternations %d --batch %d`: HIP events on the handle's stream around %d launches, "
             "%d interleaved repetitions of the whole list in one process on one box; the figure is the best repetition, the spread is max / min - 1 "
             "over the repetitions.  Example lens model, %.2f %% of the destination valid.  Priced bytes per destination pixel: remap 8 (record) + 1 (valid) + 3 (out) + source, "
             "conversion source + 3.  The BGR8 remap is the parent revision's kernel (identical generated code)." % (alternations, batch, batch, alternations, 100 * valid), "",
             "Best device copy (adc_device_copy_kernel_ms, %d MiB): %.1f us, %.2f TB/s (read + written)." % (cb >> 20, 1e3 * copy_ms, copy_tbs), "",
             "Clock state before: " + "; ".join(clocks[0]), "", "Clock state after: " + "; ".join(clocks[1]), "",
             "| layout | remap us | spread | priced B/px | priced TB/s | vs BGR8 remap | convert us | spread | priced B/px | priced TB/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    table, slow = {}, []
    for name, _, src in RAW_LAYOUTS:
        r, c = times[name]["remap"], times[name]["convert"]
        rb, cbp = 12.0 + src, src + 3.0
        table[name] = {"remap_us": [round(1e3 * t, 2) for t in r], "convert_us": [round(1e3 * t, 2) for t in c], "remap_bytes_per_px": rb, "convert_bytes_per_px": cbp}
        rate = base / min(r)
        if rate < 0.5:
            slow.append(name)
        lines.append("| %s | %.1f | %.0f %% | %.1f | %.2f | %.2f x | %.1f | %.0f %% | %.1f | %.2f |" % (
            name, 1e3 * min(r), 100 * (max(r) / min(r) - 1), rb, rb * P / (min(r) * 1e-3) / 1e12, rate, 1e3 * min(c), 100 * (max(c) / min(c) - 1), cbp,
            cbp * P / (min(c) * 1e-3) / 1e12))
    lines += ["", "Layouts below half of the BGR8 remap's rate (pixels per second): " + (", ".join(slow) if slow else "none") + ".", "",
              "## adc_match host to host, structured 1080p pair, D = 128 (pairs/s, %d Matches per figure)" % reps, "",
              "| input | uploaded bytes per pair | pairs/s per repetition | best |", "|---|---|---|---|"]
    for name, (rf, l, r) in pairs.items():
        lines.append("| %s | %d | %s | %.1f |" % (name, l.nbytes + r.nbytes, ", ".join("%.1f" % v for v in rates[name]), max(rates[name])))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    print(json.dumps({"rawfmt_timing": {"kernels": table, "copy_us": [round(1e3 * c, 2) for c in copies], "match_pairs_per_s": rates, "clocks": clocks}}), flush=True)


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
    ap.add_argument("--rawfmt", action="store_true", help="the camera layouts at 1920x1080 (a run of its own)")
    a = ap.parse_args()
    if a.rawfmt:
        rawfmt(a.alternations if a.alternations != 5 else 3, a.batch if a.batch != 50 else 20, a.out or os.path.join(ROOT, "profiles", "rawfmt_timing.md"))
        return
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
