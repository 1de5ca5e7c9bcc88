"""Runs inside a subprocess of tests/test_gpu_speckle.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the
background): every HIP call of switching the speckle filter on (first use: the scratch allocations) plus a filtered adc_match, of a
filtered adc_match_device + adc_wait and of an adc_filter_speckles_device + adc_wait fails once.  The call (or its adc_wait) must
report it, clean calls on the SAME handle afterwards must deliver the undisturbed results, and no device memory may stay behind.
Prints one JSON object; the test asserts on it.  `--plain-only`: just the number of hooked HIP calls of a plain adc_match and of
a plain adc_match_device + adc_wait on a handle that never had the filter set (works with a library that predates the filter)."""
import ctypes as C
import json
import sys

import numpy as np

import adcensus_amd as A
from adcensus_amd import workloads

SIZE, DIFF = 10, 0.0625  # (on this map: 1229 components, 1190 of them removed, the largest of 18372 pixels kept)


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

    # ---- a handle that never had the filter set: the hooked HIP calls of a plain Match (the parent's number)
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, 4 * n)]
    dl, dr, dd, pl = bufs
    assert L.adc_memcpy_h2d(dl, np.ascontiguousarray(left).ctypes.data, 3 * n) == 0
    assert L.adc_memcpy_h2d(dr, np.ascontiguousarray(right).ctypes.data, 3 * n) == 0
    want = st.match(left, right)
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

    # ---- undisturbed filtered results and the number of HIP calls of each form
    L.adc_test_fail_at(0)
    st.set_speckle_filter(SIZE, DIFF)
    out["setter_first_calls"] = int(L.adc_test_hip_calls())
    want_f = st.match(left, right)
    want_stats = st.speckle_stats()
    L.adc_test_fail_at(0)
    st.match(left, right)
    out["filtered_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    st.set_speckle_filter(SIZE, DIFF)
    out["setter_again_calls"] = int(L.adc_test_hip_calls())
    st.set_speckle_filter(0, 0.0)
    assert same(st.match(left, right), want)
    out["removed_pixels"] = want_stats[2]
    assert want_stats[2] > 0 and not same(want, want_f)
    st.Release()
    L.adc_device_synchronize()
    base = free_bytes(hip)  # (after one handle has come and gone: the runtime's own pools exist)

    # ---- the setter's first use + a filtered adc_match on a FRESH handle: every call fails once
    first = out["setter_first_calls"] + out["filtered_calls"]
    not_failed, wrong_after = [], []
    for k in range(1, first + 1):
        st = A.ADCensusStereo(device=0)
        L.adc_test_fail_at(0)
        assert st.Initialize(W, H, opt)
        L.adc_test_fail_at(k)
        d = np.empty((H, W), np.float32)
        ok = L.adc_set_speckle_filter(st._h, SIZE, DIFF) == 0 and st.Match(left, right, d)
        L.adc_test_fail_at(0)
        if ok or not A.last_error():
            not_failed.append(k)
        st.set_speckle_filter(SIZE, DIFF)
        if not same(st.match(left, right), want_f) or not same(st.match(left, right), want_f) or st.speckle_stats() != want_stats:
            wrong_after.append(k)
        st.set_speckle_filter(0, 0.0)
        if not same(st.match(left, right), want):
            wrong_after.append(-k)
        st.Release()
    out["host_not_failed"], out["host_wrong_after"] = not_failed, wrong_after
    L.adc_device_synchronize()
    out["host_leak_bytes"] = base - free_bytes(hip)

    # ---- a filtered adc_match_device + adc_wait, and adc_filter_speckles_device + adc_wait, on one handle
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    st.set_speckle_filter(SIZE, DIFF)

    def fetch(p=dd):
        d = np.empty((H, W), np.float32)
        assert L.adc_memcpy_d2h(d.ctypes.data, p, d.nbytes) == 0
        return d

    def device_call():
        return st.match_device(dl, dr, dd) and st.wait()

    def filter_call():
        assert L.adc_memcpy_h2d(dd, want.ctypes.data, 4 * n) == 0
        return st.filter_speckles_device(dd, SIZE, DIFF, pl) and st.wait()

    for name, call in (("device", device_call), ("filter", filter_call)):
        assert call() and same(fetch(), want_f) and st.speckle_stats() == want_stats, name
        L.adc_test_fail_at(0)
        call()
        calls = int(L.adc_test_hip_calls())
        not_failed, wrong_after = [], []
        for k in range(1, calls + 1):
            L.adc_test_fail_at(k)
            ok = call()
            L.adc_test_fail_at(0)
            if ok or not A.last_error():
                not_failed.append(k)
            if not (device_call() and same(fetch(), want_f) and call() and same(fetch(), want_f) and st.speckle_stats() == want_stats):
                wrong_after.append(k)
        out[name + "_calls"], out[name + "_not_failed"], out[name + "_wrong_after"] = calls, not_failed, wrong_after
    st.Release()
    for b in bufs:
        L.adc_device_free(b)
    L.adc_device_synchronize()
    out["final_leak_bytes"] = base - free_bytes(hip)
    print("FAULT_PROBE " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
