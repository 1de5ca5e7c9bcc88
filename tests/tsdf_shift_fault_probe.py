"""Runs inside a subprocess of tests/test_gpu_tsdf_shift_faults.py (and, with the argument `calls`, of tests/test_gpu_tsdf_shift.py) with
ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the background).

Without an argument: every HIP call of the moving volume fails once -- a device scenario (adc_tsdf_shift_device with a point list and a
count word, adc_wait) and a host scenario (adc_tsdf_shift), each on a volume whose first shift it is, so that the allocation of the
second planes, the report words and the tile counts is among the calls, and on a volume that has shifted before.  The failures are
injected return codes; no kernel is made to fault.  The failing call must report it with code 2; the volume, its origin and its offset
must be what they were; the same shift afterwards must deliver the list, the report, the volume, the offset and the origin of
tests/tsdf_shift_ref.py byte for byte; a Match must still be exact; and no device memory may stay behind (hipMemGetInfo and
adc_test_live_buffers).

With `calls`: the numbers of hooked HIP calls the existing entry points make on a handle that never shifts and on one that has, and
those of the shift itself.  Prints one JSON object; the tests assert on it."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import adcensus_amd as A  # noqa: E402
from adcensus_amd import workloads  # noqa: E402
from tests import tsdf_ref as T  # noqa: E402
from tests import tsdf_shift_cases as SC  # noqa: E402
from tests import tsdf_shift_ref as SR  # noqa: E402
from tests.test_tsdf_api import c_frame, c_params  # noqa: E402

W, H, D = 64, 48, 16
VOL = "v12x7x9"
FIRST, SECOND = (3, -2, 1), (-4, 1, 0)  # (both variants of the shift kernel)
F = np.float32


def free_bytes(hip):
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


class Failed(Exception):
    pass


def library():
    L = A.lib()
    assert hasattr(L, "adc_test_fail_at"), "not the fault-injection build"
    L.adc_test_fail_at.argtypes = [C.c_long]
    L.adc_test_fail_at.restype = None
    L.adc_test_hip_calls.restype = C.c_long
    L.adc_test_live_buffers.restype = C.c_long
    return L


def state(st):
    """everything a failed shift must leave alone"""
    tsdf, color = st.tsdf_download()
    off, org0 = st.tsdf_offset()
    return tsdf.tobytes() + color.tobytes() + np.array(off, np.int32).tobytes() + np.array(org0 + tuple(st.tsdf_volume_device()[2].origin), F).tobytes()


def expected(new, q, off, p, pts, rep):
    return (pts.tobytes() + np.array(SR.report_words(rep) + [0] * 4, np.uint32).tobytes() + new[0].tobytes() + new[1].tobytes() + np.array(off, np.int32).tobytes() +
            np.array(tuple(p["origin"]) + tuple(q["origin"]), F).tobytes())


def faults():
    L = library()
    hip = C.CDLL("libamdhip64.so")
    p, old = SC.params(VOL, True), SC.volume(VOL, True)
    params = c_params(p)
    v1, q1, o1, pts1, rep1 = SR.shift(old, p, SR.shift_params(FIRST))
    v2, q2, o2, pts2, rep2 = SR.shift(v1, q1, SR.shift_params(SECOND), o1, p["origin"])
    want1, want2 = expected(v1, q1, o1, p, pts1, rep1), expected(v2, q2, o2, p, pts2, rep2)
    left, right = workloads.structured_pair(W, H, D, seed=31)
    opt = A.ADCensusOption(max_disparity=D, do_filling=0)
    cap = max(len(pts1), len(pts2)) + 3
    out = dict(points=[len(pts1), len(pts2)])
    codes = set()

    def must(rc):
        if rc is True or rc == 0:
            return
        if rc is not False:
            codes.add(int(rc))
        raise Failed(A.last_error())

    live0 = int(L.adc_test_live_buffers())
    d_pts, d_cnt = L.adc_device_malloc(16 * cap), L.adc_device_malloc(16)

    def device_shift(st, s):
        sp = A.TsdfShiftParams(s)
        must(L.adc_tsdf_shift_device(st._h, C.byref(sp), d_pts, cap, d_cnt))
        must(L.adc_wait(st._h))
        rep = st.tsdf_shift_report()
        got = np.empty(16 * rep.points, np.uint8)
        cnt = np.empty(1, np.uint32)
        assert got.nbytes == 0 or L.adc_memcpy_d2h(got.ctypes.data, d_pts, got.nbytes) == 0
        assert L.adc_memcpy_d2h(cnt.ctypes.data, d_cnt, 4) == 0 and int(cnt[0]) == rep.points
        return got.tobytes() + bytes(rep)

    def host_shift(st, s):
        sp, rep = A.TsdfShiftParams(s), A.TsdfShiftReport()
        pts = np.zeros(cap, A.POINT_DTYPE)
        must(L.adc_tsdf_shift(st._h, C.byref(sp), pts.ctypes.data, cap, C.byref(rep)))
        return pts[:rep.points].tobytes() + bytes(rep)

    def open_volume(shifted):
        """a fresh handle with the case's volume; shifted: FIRST has been applied (everything of the shift is allocated)"""
        L.adc_test_fail_at(0)
        st = A.ADCensusStereo(device=0)
        assert st.Initialize(W, H, opt)
        assert st.tsdf_create(params), A.last_error()
        st.tsdf_upload(*old)
        if shifted:
            assert st.tsdf_shift_device(FIRST) and st.wait(), A.last_error()
        return st

    want_d = None
    base = None
    for name, call, shifted, s, want in (("device_first", device_shift, False, FIRST, want1), ("device_later", device_shift, True, SECOND, want2),
                                         ("host_first", host_shift, False, FIRST, want1), ("host_later", host_shift, True, SECOND, want2)):
        st = open_volume(shifted)
        if want_d is None:
            want_d = st.match(left, right)
        L.adc_test_fail_at(0)
        assert call(st, s) + state(st) == want, name
        st.Release()
        if base is None:
            L.adc_device_synchronize()
            base = free_bytes(hip)  # (after one handle has come and gone: the runtime's own pools exist)
        # the calls of the shift alone
        st = open_volume(shifted)
        L.adc_test_fail_at(0)
        call(st, s)
        calls = int(L.adc_test_hip_calls())
        st.Release()
        not_failed, changed, wrong_after, live, waits = [], [], [], [], []
        for k in range(1, calls + 1):
            st = open_volume(shifted)
            before = state(st)
            L.adc_test_fail_at(k)
            in_wait = False
            try:
                call(st, s)
                not_failed.append(k)
            except Failed as exc:
                if "adc_" not in str(exc):
                    not_failed.append(-k)
                in_wait = call is device_shift and "adc_tsdf_shift" not in str(exc)
            L.adc_test_fail_at(0)
            if in_wait:
                # the device form had returned 0 and the shift was on the stream: it was adc_wait that failed, behind a shift that is
                # complete (its report is lost); the volume is the shifted one, whole
                waits.append(k)
                if state(st) != want[-len(before):]:
                    changed.append(k)
            else:
                if state(st) != before:
                    changed.append(k)
                if call(st, s) + state(st) != want:
                    wrong_after.append(k)
            if k % 6 == 0 and not np.array_equal(st.match(left, right).view(np.uint32), want_d.view(np.uint32)):
                wrong_after.append(-1000 - k)
            st.Release()
            if int(L.adc_test_live_buffers()) != live0:
                live.append(k)
        out[name] = dict(calls=calls, not_failed=not_failed, changed=changed, wrong_after=wrong_after, live_after=live, failed_in_wait=waits)
    L.adc_device_free(d_pts)
    L.adc_device_free(d_cnt)
    L.adc_device_synchronize()
    out["final_leak_bytes"] = base - free_bytes(hip)
    out["final_live"] = int(L.adc_test_live_buffers()) - live0
    out["codes"] = sorted(codes)
    print("FAULT_PROBE " + json.dumps(out))
    return 0


def calls():
    L = library()
    p, old = SC.params(VOL, True), SC.volume(VOL, True)
    params = c_params(p)
    left, right = workloads.structured_pair(W, H, D, seed=31)
    opt = A.ADCensusOption(max_disparity=D, do_filling=0)
    rng = np.random.default_rng(3)
    depth = (2.2 + 0.05 * rng.standard_normal((H, W))).astype(F)
    frame = c_frame(T.frame((60.0, 0.16, 50.0, 24.0, 0.0), kind=T.FROM_DEPTH))
    live0 = int(L.adc_test_live_buffers())
    d_map, d_pts, d_cnt = L.adc_device_malloc(depth.nbytes), L.adc_device_malloc(16 * 4096), L.adc_device_malloc(16)
    assert L.adc_memcpy_h2d(d_map, depth.ctypes.data, depth.nbytes) == 0

    def count(fn):
        L.adc_test_fail_at(0)
        assert fn(), A.last_error()
        n = int(L.adc_test_hip_calls())
        assert L.adc_wait(st._h) == 0, A.last_error()
        return n

    def match():
        return st.match_device(dl, dr, dd)

    out = {}
    for name in ("plain", "shifted"):
        st = A.ADCensusStereo(device=0)
        L.adc_test_fail_at(0)
        assert st.Initialize(W, H, opt)
        dl, dr, dd = L.adc_device_malloc(left.nbytes), L.adc_device_malloc(right.nbytes), L.adc_device_malloc(W * H * 4)
        assert L.adc_memcpy_h2d(dl, left.ctypes.data, left.nbytes) == 0 and L.adc_memcpy_h2d(dr, right.ctypes.data, right.nbytes) == 0
        o = {}
        count(match)  # (the first Match of a handle learns; the second is the steady state)
        o["match_before_volume"] = count(match)
        o["create"] = count(lambda: st.tsdf_create(params))
        st.tsdf_upload(*old)
        if name == "shifted":
            out["shift_first"] = count(lambda: st.tsdf_shift_device(FIRST, d_pts, 4096, d_count=d_cnt))
            out["shift"] = count(lambda: st.tsdf_shift_device(SECOND, d_pts, 4096, d_count=d_cnt))
            out["shift_zero"] = count(lambda: st.tsdf_shift_device((0, 0, 0), d_pts, 4096, d_count=d_cnt))
            out["shift_all"] = count(lambda: st.tsdf_shift_device((0, 0, -9), d_pts, 4096, d_count=d_cnt))
            st.tsdf_upload(*old)
        o["integrate"] = count(lambda: st.tsdf_integrate_device(d_map, frame))
        o["extract_first" if name == "plain" else "extract"] = count(lambda: st.tsdf_extract_device(d_pts, 4096))
        o["extract"] = count(lambda: st.tsdf_extract_device(d_pts, 4096))
        o["match"] = count(match)
        o["create_again"] = count(lambda: st.tsdf_create(params))
        out[name] = o
        st.Release()
        for b in (dl, dr, dd):
            L.adc_device_free(b)
    for b in (d_map, d_pts, d_cnt):
        L.adc_device_free(b)
    out["live"] = int(L.adc_test_live_buffers()) - live0
    print("CALLS_PROBE " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(calls() if sys.argv[1:] == ["calls"] else faults())
