#!/usr/bin/env python3
"""Times the ray cast of the TSDF volume (adc_tsdf_raycast_device: the cleared report words, k_tsdf_raycast, the pinned read-back) on
one MI355X, explains the time with the number of samples, prices the bytes written against the copy kernel and checks that the
benchmark's headline did not move; writes profiles/tsdf_raycast_timing.md.

    python tools/tsdf_raycast_timing.py [--parent-lib DIR/libadcensus_hip.so --parent-commit HASH] [--out FILE]

In the manner of tools/tsdf_timing.py (whose driver functions it uses): one child process per step, each with its own time limit, and
nothing more is started behind a step that fails.
  calls     the volumes of profiles/tsdf_timing.md (the final map of the benchmark's structured pair, D = 128, fused once from the
            identity pose into cubes of 256^3 and 512^3 voxels around the map's median depth, truncation 4 voxels, a colour volume), seen
            from a pose a little off the fusing one, in views of 1920x1080 and 640x480 (the same field of view); depth alone and all four
            outputs; skip = step and skip = trunc / 2 (step = voxel / 2).  The whole call between two HIP events on the handle's stream,
            the median of --reps after a warm-up.  Samples per ray and per nanosecond from the report; the copy kernel
            (adc_device_copy_kernel_ms) on the bytes the call writes.
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

W, H, D, CALIB = TT.W, TT.H, TT.D, TT.CALIB
SIDES = TT.SIDES
VIEWS = [(1920, 1080), (640, 480)]
TAG = "TSDF_RAYCAST_TIMING "
ANALYSIS_HEADING = "## What bounds the kernel"


def child(a):
    import adcensus_amd as A
    from adcensus_amd import workloads
    L = A.lib()
    hip = C.CDLL("libamdhip64.so")
    L.adc_get_stream.restype = C.c_void_p
    L.adc_get_stream.argtypes = [C.c_void_p]
    out = {"version": L.adc_version().decode()}
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, A.ADCensusOption(max_disparity=D)), A.last_error()
    stream = C.c_void_p(L.adc_get_stream(st._h))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    N = W * H
    dm, di = (L.adc_device_malloc(s) for s in (4 * N, 3 * N))
    outs = [L.adc_device_malloc(s * N) for s in (4, 16, 3, 1)]
    ca, cb = L.adc_device_malloc(1 << 28), L.adc_device_malloc(1 << 28)
    frame = A.TsdfFrame(CALIB)

    def timed(call):
        ms_all = []
        for k in range(a.reps + 1):  # (the first one warms up)
            assert hip.hipEventRecord(ev0, stream) == 0
            assert call(), A.last_error()
            assert hip.hipEventRecord(ev1, stream) == 0
            assert st.wait(), A.last_error()
            ms = C.c_float(0)
            assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
            if k:
                ms_all.append(float(ms.value))
        return statistics.median(ms_all)

    left, right = workloads.structured_pair(W, H, D, seed=777)
    disp = st.match(left, right)
    assert L.adc_memcpy_h2d(dm, disp.ctypes.data, disp.nbytes) == 0 and L.adc_memcpy_h2d(di, left.ctypes.data, left.nbytes) == 0
    a_ = np.abs(disp)
    ok = np.isfinite(a_) & (a_ + CALIB[4] > 0)
    zmed = float(np.median(CALIB[0] * CALIB[1] / (a_[ok] + CALIB[4])))
    extent = 1.25 * zmed
    ang = np.radians(2.0)
    R = (np.cos(ang), 0.0, np.sin(ang), 0.0, 1.0, 0.0, -np.sin(ang), 0.0, np.cos(ang))  # two degrees about y, a little off the fusing pose
    t = (0.02 * zmed, -0.01 * zmed, 0.0)
    for side in SIDES:
        voxel = extent / side
        p = A.TsdfParams(side, side, side, voxel, (-extent / 2, -extent / 2, zmed - extent / 2), 4 * voxel, max_weight=64, flags=A.TSDF_COLOR)
        assert st.tsdf_create(p), A.last_error()
        assert st.tsdf_integrate_device(dm, frame, di) and st.wait(), A.last_error()
        for vw, vh in VIEWS:
            scale = vw / W
            for skip_name, skip in (("skip = step", voxel / 2), ("skip = trunc / 2", 2 * voxel)):
                view = A.TsdfRaycastParams(vw, vh, CALIB[0] * scale, vw / 2 - 0.3, vh / 2 + 0.2, R, t, voxel, 100.0 * zmed, voxel / 2, skip, 1, 16384)
                for what, ptrs in (("depth", (outs[0], None, None, None)), ("all", tuple(outs))):
                    ms = timed(lambda: st.tsdf_raycast_device(view, *ptrs))
                    rep = st.tsdf_raycast_report()
                    written = vw * vh * (4 if what == "depth" else 24)
                    copy = float(L.adc_device_copy_kernel_ms(cb, ca, max(written // 32 * 16, 16), 5))
                    key = "%d %dx%d %s %s" % (side, vw, vh, skip_name, what)
                    out[key] = dict(ms=ms, rays=rep.rays, hit=rep.hit, miss=rep.miss, no_surface=rep.no_surface, behind=rep.behind, exhausted=rep.exhausted,
                                    samples=rep.samples, written=written, copy=copy)
                    print(key, out[key], flush=True)
    assert st.tsdf_destroy()
    for b in [dm, di, ca, cb] + outs:
        L.adc_device_free(b)
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.Release()
    print(TAG + json.dumps(out), flush=True)


def rows(calls, views):
    md = []
    for side in SIDES:
        for vw, vh in views:
            for skip_name in ("skip = step", "skip = trunc / 2"):
                for what in ("depth", "all"):
                    c = calls["%d %dx%d %s %s" % (side, vw, vh, skip_name, what)]
                    md.append("| %d^3 | %dx%d | %s | %s | %.4f | %d | %.1f | %.2f | %.2f | %.4f | %.1f |" % (
                        side, vw, vh, skip_name, "depth alone" if what == "depth" else "all four", c["ms"], c["hit"], c["samples"] / c["rays"], c["samples"] / c["ms"] / 1e6,
                        c["written"] / 1e6, c["copy"], c["ms"] / c["copy"] if c["copy"] > 0 else float("nan")))
    return md


HEAD = ["| volume | view | skip | outputs | ms per call | rays that hit | samples per ray | samples per ns | MB written | copy kernel, same bytes, ms | call / copy |",
        "|---|---|---|---|---|---|---|---|---|---|---|"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_raycast_timing.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = os.path.abspath(__file__)
    md = ["# Ray cast of the TSDF volume: timing on one MI355X", "",
          "`tools/tsdf_raycast_timing.py`; the volumes of profiles/tsdf_timing.md (the final map of the benchmark's structured pair, D = 128, fused once from the "
          "identity pose; cubes of 256^3 and 512^3 voxels around the map's median depth, truncation 4 voxels, a colour volume), seen from a pose two degrees and "
          "a few centimetres off the fusing one.  step = voxel / 2, min_weight 1, max_steps 16384.  The whole call (the cleared report words, the kernel, the "
          "read-back of the report) between two HIP events on the handle's stream, the median of %d after a warm-up.  Samples from the call's report.  Copy kernel: "
          "`adc_device_copy_kernel_ms` moving the bytes the call writes (a copy of half of them, read + write)." % a.reps, ""]
    calls = TT.run_child([sys.executable, me, "--child", "calls", "--reps", str(a.reps)], "", 600, TAG)
    md += HEAD + rows(calls, VIEWS)
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
