#!/usr/bin/env python3
"""Times frame-to-model tracking (adc_track_device: the cleared state, `iterations` pairs of k_track_reduce / k_track_solve, the
read-back of the record) on one MI355X, separates the reduce pass, the solve and a surplus no-op pair, prices the reduce pass against
the copy kernel on the bytes it reads and checks that the benchmark's headline did not move; writes profiles/tsdf_track_timing.md.

    python tools/tsdf_track_timing.py [--parent-lib DIR/libadcensus_hip.so --parent-commit HASH] [--out FILE]

In the manner of tools/tsdf_raycast_timing.py (whose driver functions it shares through tools/tsdf_timing.py): one child process per
step, each with its own time limit, and nothing more is started behind a step that fails.
  calls     the analytic room corner of tests/tsdf_track_cases.py (four planes) at 640x480 and 1920x1080: the model maps rendered at a
            pose A, the frame at a pose 1.6 degrees / 2.7 cm away, tracked from the guess A with eps_rot = eps_trans = 0, so that every
            one of the `iterations` solves runs.  The whole call between two HIP events on the handle's stream, the median of --reps
            after a warm-up, at stride 1, 2 and 16 and with 10 and 2 iterations.
            one pair        = (t(10 iterations) - t(2 iterations)) / 8: a reduce pass and a solve, with their two launches;
            solve           ~ the pair at stride 16, where the reduce pass has 1 / 256 of the pixels (an upper bound for the solve);
            reduce          = the pair at that stride - the pair at stride 16;
            surplus pair    = (t(10) - t(2)) / 8 on a frame without depth, which is LOST in the first solve: eight pairs of no-ops.
            The copy kernel (adc_device_copy_kernel_ms) on the bytes the reduce pass asks for: 24 per participating pixel (the map
            value, the model's depth and its normal).
  headline  bench.py --gpus 1 of the parent build and of this build, --reps repetitions each, alternating (tools/tsdf_timing.py)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import tsdf_timing as TT  # noqa: E402

SIZES = [(640, 480), (1920, 1080)]
STRIDES = (1, 2, 16)
TAG = "TSDF_TRACK_TIMING "
ANALYSIS_HEADING = "## What bounds the reduce pass"


def child(a):
    import adcensus_amd as A
    from tests import tsdf_track_cases as KC
    from tests import tsdf_track_ref as TR
    L = A.lib()
    hip = C.CDLL("libamdhip64.so")
    L.adc_get_stream.restype = C.c_void_p
    L.adc_get_stream.argtypes = [C.c_void_p]
    out = {"version": L.adc_version().decode()}
    ca, cb = L.adc_device_malloc(1 << 28), L.adc_device_malloc(1 << 28)
    for W, H in SIZES:
        st = A.ADCensusStereo(device=0)
        assert st.Initialize(W, H, A.ADCensusOption(max_disparity=64)), A.last_error()
        stream = C.c_void_p(L.adc_get_stream(st._h))
        ev0, ev1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
        c = KC.scene(W, H, KC.A_POSE, KC.SMALL, planes=KC.CORNER4)
        m = c["model"]
        frame = A.TsdfFrame(c["frame"]["calib"], c["frame"]["R"], c["frame"]["t"], c["frame"]["kind"])
        view = A.TsdfRaycastParams(m["width"], m["height"], m["focal_px"], m["cx"], m["cy"], m["R"], m["t"], 0.05, 10.0, 0.025, 0.05, 1, 4096)
        bufs = {}
        for k, arr in (("map", c["map"]), ("empty", np.zeros_like(c["map"])), ("mdepth", c["mdepth"]), ("mnormals", c["mnormals"])):
            arr = np.ascontiguousarray(arr, np.float32)
            bufs[k] = L.adc_device_malloc(arr.nbytes)
            assert L.adc_memcpy_h2d(bufs[k], arr.ctypes.data, arr.nbytes) == 0

        def timed(which, stride, iterations):
            p = A.TrackParams(iterations=iterations, stride=stride, eps_rot=0.0, eps_trans=0.0)
            ms_all = []
            for k in range(a.reps + 1):  # (the first one warms up)
                assert hip.hipEventRecord(ev0, stream) == 0
                assert st.track_device(bufs[which], frame, view, bufs["mdepth"], bufs["mnormals"], p), A.last_error()
                assert hip.hipEventRecord(ev1, stream) == 0
                assert st.wait(), A.last_error()
                ms = C.c_float(0)
                assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
                if k:
                    ms_all.append(float(ms.value))
            return statistics.median(ms_all), st.track_result()

        for stride in STRIDES:
            t10, res = timed("map", stride, 10)
            assert res.status == TR.MAX_ITERATIONS and res.solves == 10, (res.status, res.solves)
            t2, _ = timed("map", stride, 2)
            l10, lost = timed("empty", stride, 10)
            assert lost.status == TR.LOST and lost.solves == 1
            l2, _ = timed("empty", stride, 2)
            asked = 24 * res.pixels
            copy = float(L.adc_device_copy_kernel_ms(cb, ca, max(asked // 32 * 16, 16), 5))
            key = "%dx%d %d" % (W, H, stride)
            out[key] = dict(t10=t10, t2=t2, l10=l10, l2=l2, pixels=res.pixels, used=res.used, asked=asked, copy=copy, rms=res.iteration[9].rms)
            print(key, out[key], flush=True)
        for b in bufs.values():
            L.adc_device_free(b)
        hip.hipEventDestroy(ev0)
        hip.hipEventDestroy(ev1)
        st.Release()
    L.adc_device_free(ca)
    L.adc_device_free(cb)
    print(TAG + json.dumps(out), flush=True)


def tables(calls):
    md = ["## The whole call, 10 iterations that all run", "",
          "| frame | stride | participating pixels | used in the last pass | ms per call, 10 iterations | 2 iterations | LOST in the first solve, 10 enqueued | 2 enqueued |",
          "|---|---|---|---|---|---|---|---|"]
    for W, H in SIZES:
        for s in STRIDES:
            c = calls["%dx%d %d" % (W, H, s)]
            md.append("| %dx%d | %d | %d | %d | %.4f | %.4f | %.4f | %.4f |" % (W, H, s, c["pixels"], c["used"], c["t10"], c["t2"], c["l10"], c["l2"]))
    md += ["", "## One pair, its parts, a surplus pair, and the copy kernel", "",
           "| frame | stride | one pair (reduce + solve), us | solve (the pair at stride 16), us | reduce, us | surplus no-op pair, us | MB the reduce pass asks for | "
           "copy kernel, same bytes, us | reduce / copy |", "|---|---|---|---|---|---|---|---|---|"]
    for W, H in SIZES:
        solve = (calls["%dx%d 16" % (W, H)]["t10"] - calls["%dx%d 16" % (W, H)]["t2"]) / 8 * 1e3
        for s in STRIDES[:-1]:
            c = calls["%dx%d %d" % (W, H, s)]
            pair = (c["t10"] - c["t2"]) / 8 * 1e3
            noop = (c["l10"] - c["l2"]) / 8 * 1e3
            red = pair - solve
            md.append("| %dx%d | %d | %.1f | %.1f | %.1f | %.1f | %.2f | %.1f | %.1f |" % (W, H, s, pair, solve, red, noop, c["asked"] / 1e6, c["copy"] * 1e3,
                                                                                         red / (c["copy"] * 1e3) if c["copy"] > 0 else float("nan")))
    return md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_track_timing.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = os.path.abspath(__file__)
    md = ["# Frame-to-model tracking: timing on one MI355X", "",
          "`tools/tsdf_track_timing.py`; the analytic room corner of tests/tsdf_track_cases.py (four planes), the model maps rendered at a pose A, the frame "
          "1.6 degrees / 2.7 cm away, tracked from the guess A with eps_rot = eps_trans = 0, so that all `iterations` solves run; max_dist 0.1, no frame "
          "normals.  The whole call (the cleared state, the pairs of launches, the read-back of the record) between two HIP events on the handle's stream, the "
          "median of %d after a warm-up.  One pair = (t(10) - t(2)) / 8.  The solve is read off the pair at stride 16 (1 / 256 of the pixels: an upper bound), "
          "the reduce pass is the pair less that.  A surplus pair is (t(10) - t(2)) / 8 on a frame without depth, which is LOST in the first solve.  Copy "
          "kernel: `adc_device_copy_kernel_ms` moving the bytes the reduce pass asks for, 24 per participating pixel (a copy of half of them, read + write)." % a.reps, ""]
    calls = TT.run_child([sys.executable, me, "--child", "calls", "--reps", str(a.reps)], "", 600, TAG)
    md += tables(calls)
    md += ["", "## The benchmark's headline against the parent (%s), %d alternating repetitions each" % (a.parent_commit, a.reps), ""]
    md += TT.headline(a)
    text = "\n".join(md) + "\n"
    if os.path.exists(a.out):
        old = open(a.out).read()
        at = old.find(ANALYSIS_HEADING)
        if at >= 0:
            text += "\n" + old[at:]
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
