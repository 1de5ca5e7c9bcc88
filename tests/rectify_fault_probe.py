"""Runs inside a subprocess of tests/test_gpu_rectify.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the
background): every HIP call of switching the rectification on (first use: the allocations, the map kernels) plus a rectified adc_match,
of a rectified adc_match_device + adc_wait, of an adc_rectify_device + adc_wait and of adc_get_rectify_maps fails once.  The call (or
its adc_wait) must report it, clean calls on the SAME handle afterwards must deliver the undisturbed results, and no device memory may
stay behind.  Prints one JSON object; the test asserts on it.  `--plain-only`: just the number of hooked HIP calls of adc_create, of a
plain adc_match and of a plain adc_match_device + adc_wait on a handle that never had a side set (works with a library that predates
the rectification)."""
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


def free_bytes(hip):
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def main():
    L = A.lib()
    assert hasattr(L, "adc_test_fail_at"), "not the fault-injection build"
    L.adc_test_fail_at.argtypes = [C.c_long]
    L.adc_test_fail_at.restype = None
    L.adc_test_hip_calls.restype = C.c_long
    hip = C.CDLL("libamdhip64.so")
    W, H, D = 256, 144, 64
    n = W * H
    left, right = workloads.structured_pair(W, H, D, seed=31)
    opt = A.ADCensusOption(max_disparity=D, do_filling=0)
    out = {}

    def same(a, b):
        return a.tobytes() == b.tobytes()

    # ---- a handle that never had a side set: the hooked HIP calls of adc_create and of a plain Match (the parent's numbers)
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)  # (the first handle of the process: the shared lane, the probe of the XCD mapping)
    st.Release()
    st = A.ADCensusStereo(device=0)
    L.adc_test_fail_at(0)
    assert st.Initialize(W, H, opt)
    out["create_calls"] = int(L.adc_test_hip_calls())
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, 3 * n)]
    dl, dr, dd, dout = bufs
    assert L.adc_memcpy_h2d(dl, np.ascontiguousarray(left).ctypes.data, 3 * n) == 0
    assert L.adc_memcpy_h2d(dr, np.ascontiguousarray(right).ctypes.data, 3 * n) == 0
    st.match(left, right)
    L.adc_test_fail_at(0)
    st.match(left, right)
    out["plain_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert st.match_device(dl, dr, dd) and st.wait()
    out["device_plain_calls"] = int(L.adc_test_hip_calls())
    if "--plain-only" in sys.argv:
        st.Release()
        for b in bufs:
            L.adc_device_free(b)
        print("FAULT_PROBE " + json.dumps(out))
        return 0

    # ---- the raw pair: the same images as BGRA with a padded pitch (left) and as RGB (right), under a lens model
    from tests import rectify_ref as RR
    raws = [RR.pack_source(left, RR.BGRA8, W * 4 + 8), RR.pack_source(right, RR.RGB8, W * 3)]
    fmts = [A.RawFormat(W, H, W * 4 + 8, A.PIX_BGRA8), A.RawFormat(W, H, W * 3, A.PIX_RGB8)]
    model = A.CameraModel(**RR.example_model(W, H, W, H))
    mx, my = RR.model_maps(RR.second_model(W, H, W, H), W, H)  # (the right side through caller's maps)

    def set_both(s):
        return (L.adc_set_rectify_model(s._h, 0, C.byref(fmts[0]), C.byref(model)) == 0 and
                L.adc_set_rectify_maps(s._h, 1, C.byref(fmts[1]), mx.ctypes.data, my.ctypes.data) == 0)

    def set_both_checked(s):
        assert set_both(s), A.last_error()
        s._rect.set(0, fmts[0])
        s._rect.set(1, fmts[1])

    # ---- undisturbed rectified results and the number of HIP calls of each form
    L.adc_test_fail_at(0)
    assert L.adc_set_rectify_model(st._h, 0, C.byref(fmts[0]), C.byref(model)) == 0
    out["set_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert L.adc_set_rectify_maps(st._h, 1, C.byref(fmts[1]), mx.ctypes.data, my.ctypes.data) == 0
    out["set_maps_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert L.adc_set_rectify_model(st._h, 0, C.byref(fmts[0]), C.byref(model)) == 0
    out["set_second_calls"] = int(L.adc_test_hip_calls())
    set_both_checked(st)
    want_maps = st.rectify_maps(1)
    rect_l, rect_r = st.rectify(raws[0], 0), st.rectify(raws[1], 1)
    assert np.array_equal(rect_l, RR.remap(raws[0], W, H, W * 4 + 8, RR.BGRA8, *RR.model_maps(RR.example_model(W, H, W, H), W, H))[0])
    want_r = st.match(raws[0], raws[1])
    L.adc_test_fail_at(0)
    st.match(raws[0], raws[1])
    out["rect_calls"] = int(L.adc_test_hip_calls())
    st.clear_rectify()
    assert same(st.match(rect_l, rect_r), want_r)  # (a plain Match on the rectified images)
    st.Release()
    L.adc_device_synchronize()
    base = free_bytes(hip)  # (after handles have come and gone: the runtime's own pools exist)

    # ---- both set calls' first use + a rectified adc_match on a FRESH handle: every call fails once
    first = out["set_first_calls"] + out["set_maps_calls"] + out["rect_calls"]
    not_failed, wrong_after = [], []
    for k in range(1, first + 1):
        st = A.ADCensusStereo(device=0)
        L.adc_test_fail_at(0)
        assert st.Initialize(W, H, opt)
        L.adc_test_fail_at(k)
        d = np.empty((H, W), np.float32)
        ok = set_both(st) and L.adc_match(st._h, raws[0].ctypes.data, raws[1].ctypes.data, d.ctypes.data) == 0
        L.adc_test_fail_at(0)
        if ok or not A.last_error():
            not_failed.append(k)
        set_both_checked(st)
        if not same(st.match(raws[0], raws[1]), want_r) or not same(st.match(raws[0], raws[1]), want_r):
            wrong_after.append(k)
        st.clear_rectify()
        if not same(st.match(rect_l, rect_r), want_r):
            wrong_after.append(-k)
        st.Release()
    out["host_not_failed"], out["host_wrong_after"] = not_failed, wrong_after
    L.adc_device_synchronize()
    out["host_leak_bytes"] = base - free_bytes(hip)

    # ---- a rectified adc_match_device + adc_wait, adc_rectify_device + adc_wait and adc_get_rectify_maps on one handle
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    set_both_checked(st)
    raw_bufs = [L.adc_device_malloc(r.nbytes) for r in raws]
    for p, r in zip(raw_bufs, raws):
        assert L.adc_memcpy_h2d(p, r.ctypes.data, r.nbytes) == 0

    def fetch():
        d = np.empty((H, W), np.float32)
        assert L.adc_memcpy_d2h(d.ctypes.data, dd, d.nbytes) == 0
        return d

    def fetch_img():
        d = np.empty((H, W, 3), np.uint8)
        assert L.adc_memcpy_d2h(d.ctypes.data, dout, d.nbytes) == 0
        return d

    def device_call():
        return st.match_device(raw_bufs[0], raw_bufs[1], dd) and st.wait()

    def remap_call():
        assert L.adc_memcpy_h2d(dout, np.zeros(3 * n, np.uint8).ctypes.data, 3 * n) == 0
        return st.rectify_device(1, raw_bufs[1], dout) and st.wait()

    def getmaps_call():
        a, b, v = np.empty((H, W), np.float32), np.empty((H, W), np.float32), np.empty((H, W), np.uint8)
        ok = L.adc_get_rectify_maps(st._h, 1, a.ctypes.data, b.ctypes.data, v.ctypes.data) == 0
        return ok and all(same(x, y) for x, y in zip((a, b, v), want_maps))

    def all_good():
        return device_call() and same(fetch(), want_r) and remap_call() and np.array_equal(fetch_img(), rect_r) and getmaps_call()

    assert all_good()
    for name, call in (("device", device_call), ("remap", remap_call), ("getmaps", getmaps_call)):
        L.adc_test_fail_at(0)
        assert call()
        calls = int(L.adc_test_hip_calls())
        not_failed, wrong_after = [], []
        for k in range(1, calls + 1):
            L.adc_test_fail_at(k)
            ok = call()
            L.adc_test_fail_at(0)
            if ok or not A.last_error():
                not_failed.append(k)
            if not all_good():
                wrong_after.append(k)
        out[name + "_calls"], out[name + "_not_failed"], out[name + "_wrong_after"] = calls, not_failed, wrong_after
    st.Release()
    for b in bufs + raw_bufs:
        L.adc_device_free(b)
    L.adc_device_synchronize()
    out["final_leak_bytes"] = base - free_bytes(hip)
    print("FAULT_PROBE " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
