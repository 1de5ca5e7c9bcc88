#!/usr/bin/env python3
"""Times the stereo-aware TSDF fusion (adc_tsdf_weights_device: the cleared report words, k_tsdf_obs_weight, the pinned read-back;
adc_tsdf_fuse_device: the cleared words, k_tsdf_fuse, the read-back) on one MI355X with 1920x1080 maps into 256^3 and 512^3 voxels,
next to adc_tsdf_integrate_device in the same process, prices the weight pass against the copy kernel on its bytes and checks that the
benchmark's headline did not move; writes profiles/tsdf_fuse_timing.md.

    python tools/tsdf_fuse_timing.py [--parent-lib DIR/libadcensus_hip.so --parent-commit HASH] [--out FILE]

In the manner of tools/tsdf_timing.py (whose driver functions and scene it shares): one child process per step, each with its own time
limit, and nothing more is started behind a step that fails.
  calls     the final map, provenance and confidence a Match delivers for the benchmark's structured pair (D = 128); the volume of
            tools/tsdf_timing.py (a cube around the map's median depth, truncation 4 voxels, no colour) that already holds the frame.
            The whole call between two HIP events on the handle's stream, the median of --reps after a warm-up, of
              integrate          adc_tsdf_integrate_device, unchanged: the baseline
              fuse plain         adc_tsdf_fuse_device without a weight map and without the flag
              fuse weights       with the weight map of the default adc_tsdf_weight_params (z_ref = the median depth)
              fuse bilinear      without a weight map, ADC_TSDF_FUSE_BILINEAR, interp_gap 1 disparity
              fuse both
            and of adc_tsdf_weights_device with the map alone and with provenance and confidence, next to the copy kernel
            (adc_device_copy_kernel_ms) on the bytes the pass moves: 5 per pixel, 10 with both maps.
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

W, H, D, N, CALIB = TT.W, TT.H, TT.D, TT.N, TT.CALIB
SIDES = [256, 512]
VARIANTS = ("integrate", "fuse plain", "fuse weights", "fuse bilinear", "fuse both")
TAG = "TSDF_FUSE_TIMING "
ANALYSIS_HEADING = "## What bounds the kernels"


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
    dm, dp, dc, dw = (L.adc_device_malloc(s) for s in (4 * N, N, 4 * N, N))
    ca, cb = L.adc_device_malloc(1 << 26), L.adc_device_malloc(1 << 26)
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
    disp, prov, conf = st.match_ex(left, right)
    for d, arr in ((dm, disp), (dp, prov), (dc, conf)):
        arr = np.ascontiguousarray(arr)
        assert L.adc_memcpy_h2d(d, arr.ctypes.data, arr.nbytes) == 0
    a_ = np.abs(disp)
    ok = np.isfinite(a_) & (a_ + CALIB[4] > 0)
    zmed = float(np.median(CALIB[0] * CALIB[1] / (a_[ok] + CALIB[4])))
    extent = 1.25 * zmed
    wp = A.TsdfWeightParams(z_ref=zmed)
    out["weights map only"] = dict(ms=timed(lambda: st.tsdf_weights_device(dm, frame, dw, wp)), bytes=5 * N, copy=float(L.adc_device_copy_kernel_ms(cb, ca, 5 * N // 32 * 16, 5)))
    out["weights with provenance and confidence"] = dict(ms=timed(lambda: st.tsdf_weights_device(dm, frame, dw, wp, dp, dc)), bytes=10 * N,
                                                         copy=float(L.adc_device_copy_kernel_ms(cb, ca, 10 * N // 32 * 16, 5)))
    wrep = st.tsdf_fuse_report()[1]
    out["weight_report"] = [wrep.valid, wrep.nonzero, wrep.below_confidence, wrep.saturated]
    print(out, flush=True)
    bil = A.TsdfFuseParams(A.TSDF_FUSE_BILINEAR, 1.0)
    for side in SIDES:
        voxel = extent / side
        p = A.TsdfParams(side, side, side, voxel, (-extent / 2, -extent / 2, zmed - extent / 2), 4 * voxel, max_weight=64)
        assert st.tsdf_create(p), A.last_error()
        assert st.tsdf_integrate_device(dm, frame) and st.wait(), A.last_error()  # (the volume holds the frame: every variant loads and stores the same groups)
        calls = {"integrate": lambda: st.tsdf_integrate_device(dm, frame), "fuse plain": lambda: st.tsdf_fuse_device(dm, frame),
                 "fuse weights": lambda: st.tsdf_fuse_device(dm, frame, dw), "fuse bilinear": lambda: st.tsdf_fuse_device(dm, frame, None, bil),
                 "fuse both": lambda: st.tsdf_fuse_device(dm, frame, dw, bil)}
        for name in VARIANTS:
            ms = timed(calls[name])
            rep = st.tsdf_report()[0] if name == "integrate" else st.tsdf_fuse_report()[0]
            out["%d %s" % (side, name)] = dict(ms=ms, updated=rep.updated, unweighted=getattr(rep, "unweighted", 0), interpolated=getattr(rep, "interpolated", 0))
            print(side, name, out["%d %s" % (side, name)], flush=True)
    assert st.tsdf_destroy()
    for b in (dm, dp, dc, dw, ca, cb):
        L.adc_device_free(b)
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.Release()
    print(TAG + json.dumps(out), flush=True)


def tables(calls):
    md = ["## One frame into a volume that holds it", "", "| volume | call | ms | to the baseline | voxels updated | unweighted | interpolated |", "|---|---|---|---|---|---|---|"]
    for side in SIDES:
        base = calls["%d integrate" % side]["ms"]
        for name in VARIANTS:
            c = calls["%d %s" % (side, name)]
            md.append("| %d^3 | %s | %.4f | %.2f | %d | %d | %d |" % (side, name, c["ms"], c["ms"] / base, c["updated"], c["unweighted"], c["interpolated"]))
    md += ["", "## The weight pass", "", "| inputs | ms | MB moved | copy kernel, same bytes, ms | pass / copy |", "|---|---|---|---|---|"]
    for key in ("weights map only", "weights with provenance and confidence"):
        c = calls[key]
        md.append("| %s | %.4f | %.2f | %.4f | %.2f |" % (key[len("weights "):], c["ms"], c["bytes"] / 1e6, c["copy"], c["ms"] / c["copy"] if c["copy"] > 0 else float("nan")))
    md += ["", "Weight report of the second call (valid, nonzero, below_confidence, saturated): %s." % ", ".join(str(v) for v in calls["weight_report"])]
    return md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_fuse_timing.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = os.path.abspath(__file__)
    md = ["# Stereo-aware TSDF fusion: timing on one MI355X", "",
          "`tools/tsdf_fuse_timing.py`; the final map, provenance and confidence of a Match of the benchmark's structured pair (1920x1080, D = 128), the cube of "
          "`tools/tsdf_timing.py` around the map's median depth (truncation 4 voxels, no colour), which already holds the frame.  The whole call (the cleared "
          "report words, the kernel, the read-back) between two HIP events on the handle's stream, the median of %d after a warm-up, all in one process.  Weights: "
          "the default `adc_tsdf_weight_params` with z_ref = the median depth; bilinear: interp_gap 1 disparity.  Copy kernel: `adc_device_copy_kernel_ms` moving "
          "the bytes the weight pass moves (a copy of half of them, read + write)." % a.reps, ""]
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
