#!/usr/bin/env python3
"""Times the moving TSDF volume (adc_tsdf_shift_device: the cleared report words, k_tsdf_leave_measure, k_tsdf_scan, k_tsdf_leave_emit,
k_tsdf_shift, the pinned read-back) on one MI355X with volumes of 256^3 and 512^3 voxels fused from a 1920x1080 frame, with and without
colour, next to the copy kernel on the bytes a shift moves, to adc_tsdf_download + adc_tsdf_upload (what the call replaces) and to
adc_tsdf_extract_device on the same volume, and checks that the benchmark's headline did not move; writes profiles/tsdf_shift_timing.md.

    python tools/tsdf_shift_timing.py [--parent-lib DIR/libadcensus_hip.so --parent-commit HASH] [--out FILE]

In the manner of tools/tsdf_timing.py (whose driver functions and scene it shares): one child process per step, each with its own time
limit, and nothing more is started behind a step that fails.
  calls     the final map of a Match of the benchmark's structured pair (D = 128) fused once into the cube of tools/tsdf_timing.py around
            the map's median depth (truncation 4 voxels).  The whole call between two HIP events on the handle's stream, the median of
            --reps after a warm-up.  In front of every repetition (outside the events) the volume is emptied and the frame fused again,
            and the repetitions alternate between the shift and its opposite, so that the window swings between two places and every
            repetition of one sign sees the same words.  Per shift:
              with the list      d_points with room for every record, d_count
              without            d_points NULL: no emit launch
            and per volume: adc_tsdf_extract_device with the list and counting only; adc_tsdf_download + adc_tsdf_upload (wall clock,
            pageable host memory); the copy kernel (adc_device_copy_kernel_ms) on 2 * 4 * N bytes, 2 * 8 * N with colour.
  headline  bench.py --gpus 1 of the parent build and of this build, --reps repetitions each, alternating (tools/tsdf_timing.py)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import tsdf_timing as TT  # noqa: E402

W, H, D, N, CALIB = TT.W, TT.H, TT.D, TT.N, TT.CALIB
SIDES = [256, 512]
SHIFTS = [(0, 0, 8), (8, 0, 0), (5, 3, -8)]
TAG = "TSDF_SHIFT_TIMING "
ANALYSIS_HEADING = "## What bounds the call"


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
    dm, di, dc = (L.adc_device_malloc(s) for s in (4 * N, 3 * N, 16))
    ca, cb = L.adc_device_malloc(1 << 30), L.adc_device_malloc(1 << 30)
    frame = A.TsdfFrame(CALIB)

    def timed(call, before=None):
        ms_all = []
        for k in range(a.reps + 1):  # (the first one warms up)
            if before is not None:
                assert before() and st.wait(), A.last_error()
            assert hip.hipEventRecord(ev0, stream) == 0
            assert call(k), A.last_error()
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
    for side in SIDES:
        voxel = extent / side
        vox = side ** 3
        for colour in (False, True):
            key = "%d %s" % (side, "colour" if colour else "plain")
            p = A.TsdfParams(side, side, side, voxel, (-extent / 2, -extent / 2, zmed - extent / 2), 4 * voxel, max_weight=64, flags=A.TSDF_COLOR if colour else 0)
            assert st.tsdf_create(p), A.last_error()
            img = di if colour else None

            def refill():
                return st.tsdf_reset() and st.tsdf_integrate_device(dm, frame, img)

            assert refill() and st.wait(), A.last_error()
            cap = 3 * vox // 8
            dp = L.adc_device_malloc(16 * cap)
            o = dict(voxel=voxel, shifts={})
            o["extract"] = timed(lambda k: st.tsdf_extract_device(dp, cap, None, dc))
            xrep = st.tsdf_report()[1]
            assert xrep.points <= cap
            o["extract_count"] = timed(lambda k: st.tsdf_extract_device(None, 0))
            o["seen"], o["points"] = xrep.voxels_seen, xrep.points
            for s in SHIFTS:
                neg = tuple(-v for v in s)
                # the window swings: an even repetition shifts by s from the place of creation, an odd one back
                place = [0]

                def call(k, pts, c):
                    back = place[0] % 2 == 1
                    place[0] += 1
                    return st.tsdf_shift_device(neg if back else s, pts, c, d_count=dc if pts else None)

                with_list = timed(lambda k: call(k, dp, cap), refill)
                rep = st.tsdf_shift_report()
                assert rep.points <= cap
                if place[0] % 2 == 1:  # (back to the place of creation for the next series)
                    assert refill() and st.tsdf_shift_device(neg) and st.wait(), A.last_error()
                    place[0] += 1
                without = timed(lambda k: call(k, None, 0), refill)
                if place[0] % 2 == 1:
                    assert refill() and st.tsdf_shift_device(neg) and st.wait(), A.last_error()
                    place[0] += 1
                assert st.tsdf_offset()[0] == (0, 0, 0)
                o["shifts"]["%d,%d,%d" % s] = dict(with_list=with_list, without=without, report=[rep.moved_nonempty, rep.left_nonempty, rep.left_seen, rep.points])
            bytes_moved = 2 * 4 * vox * (2 if colour else 1)
            o["bytes"] = bytes_moved
            o["copy"] = float(L.adc_device_copy_kernel_ms(cb, ca, min(bytes_moved // 2, 1 << 30), 5)) * (bytes_moved // 2 / min(bytes_moved // 2, 1 << 30))
            assert refill() and st.wait(), A.last_error()
            t0 = time.perf_counter()
            host = st.tsdf_download()
            t1 = time.perf_counter()
            st.tsdf_upload(*host)
            t2 = time.perf_counter()
            del host
            o["download_ms"], o["upload_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
            L.adc_device_free(dp)
            out[key] = o
            print(key, o, flush=True)
    assert st.tsdf_destroy()
    for b in (dm, di, dc, ca, cb):
        L.adc_device_free(b)
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.Release()
    print(TAG + json.dumps(out), flush=True)


def child_trace(a):
    """for a kernel trace taken in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/tsdf_shift_timing.py --child trace):
    the 512^3 volume without colour, a few z shifts there and back, each behind a fused frame, and as many extractions"""
    import adcensus_amd as A
    from adcensus_amd import workloads
    L = A.lib()
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, A.ADCensusOption(max_disparity=D)), A.last_error()
    left, right = workloads.structured_pair(W, H, D, seed=777)
    disp = st.match(left, right)
    dm, dc = L.adc_device_malloc(4 * N), L.adc_device_malloc(16)
    assert L.adc_memcpy_h2d(dm, disp.ctypes.data, disp.nbytes) == 0
    a_ = np.abs(disp)
    ok = np.isfinite(a_) & (a_ + CALIB[4] > 0)
    zmed = float(np.median(CALIB[0] * CALIB[1] / (a_[ok] + CALIB[4])))
    extent, side = 1.25 * zmed, 512
    voxel = extent / side
    frame = A.TsdfFrame(CALIB)
    assert st.tsdf_create(A.TsdfParams(side, side, side, voxel, (-extent / 2, -extent / 2, zmed - extent / 2), 4 * voxel, max_weight=64)), A.last_error()
    cap = 3 * side ** 3 // 8
    dp = L.adc_device_malloc(16 * cap)
    for k in range(2 * a.reps):
        assert st.tsdf_reset() and st.tsdf_integrate_device(dm, frame), A.last_error()
        assert st.tsdf_shift_device((0, 0, 8 if k % 2 == 0 else -8), dp, cap, d_count=dc) and st.wait(), A.last_error()
        assert st.tsdf_extract_device(dp, cap, None, dc) and st.wait(), A.last_error()
    for b in (dm, dc, dp):
        L.adc_device_free(b)
    st.Release()


def tables(calls):
    md = ["## The shift call", "",
          "| volume | colour | shift | call with the list, ms | without a list, ms | MB moved | copy kernel, same bytes, ms | call / copy | download + upload, ms | leaving points | moved / left non-empty voxels |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for side in SIDES:
        for colour in ("plain", "colour"):
            c = calls["%d %s" % (side, colour)]
            for s in SHIFTS:
                r = c["shifts"]["%d,%d,%d" % s]
                md.append("| %d^3 | %s | %d,%d,%d | %.4f | %.4f | %.0f | %.4f | %.2f | %.0f | %d | %d / %d |" % (
                    (side, colour) + s + (r["with_list"], r["without"], c["bytes"] / 1e6, c["copy"], r["with_list"] / c["copy"] if c["copy"] > 0 else float("nan"),
                                          c["download_ms"] + c["upload_ms"], r["report"][3], r["report"][0], r["report"][1])))
    md += ["", "## The leaving list against a full extraction", "",
           "The z shift touches 8 of the volume's layers (plus the layer in front of them); the x shift cuts every row, so no tile can leave early.  The scan of the "
           "tile counts is `k_tsdf_scan` in all of them.", "",
           "| volume | colour | adc_tsdf_extract_device, ms | counting only (measure + scan), ms | points | z shift with the list, ms | x shift with the list, ms | x - z, ms |",
           "|---|---|---|---|---|---|---|---|"]
    for side in SIDES:
        for colour in ("plain", "colour"):
            c = calls["%d %s" % (side, colour)]
            z, x = c["shifts"]["0,0,8"]["with_list"], c["shifts"]["8,0,0"]["with_list"]
            md.append("| %d^3 | %s | %.4f | %.4f | %d | %.4f | %.4f | %.4f |" % (side, colour, c["extract"], c["extract_count"], c["points"], z, x, x - z))
    return md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_shift_timing.md"))
    a = ap.parse_args()
    if a.child:
        return child_trace(a) if a.child == "trace" else child(a)
    me = os.path.abspath(__file__)
    md = ["# Moving TSDF volume: timing on one MI355X", "",
          "`tools/tsdf_shift_timing.py`; the final map of a Match of the benchmark's structured pair (1920x1080, D = 128) fused once into the cube of "
          "`tools/tsdf_timing.py` around the map's median depth (truncation 4 voxels).  The whole call (the cleared report words, the leaving list's measure, scan and "
          "emit, the shift kernel, the read-back) between two HIP events on the handle's stream, the median of %d after a warm-up, all in one process; in front of "
          "every repetition the volume is emptied and the frame fused again, and the repetitions alternate between the shift and its opposite.  Copy kernel: "
          "`adc_device_copy_kernel_ms` on the bytes a shift moves (2 * 4 * N, 2 * 8 * N with colour: a copy of half of them, read + write).  Download + upload: "
          "`adc_tsdf_download` and `adc_tsdf_upload` of the same volume, wall clock, pageable host memory -- without the host's re-packing between them." % a.reps, ""]
    calls = TT.run_child([sys.executable, me, "--child", "calls", "--reps", str(a.reps)], "", 900, TAG)
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
