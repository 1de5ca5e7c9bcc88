"""Runs inside a subprocess of tests/test_gpu_outputs.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the
background): every HIP call of an adc_match_out with all three outputs, of an adc_match_device_out and of an adc_reproject_device
fails once.  The call (or its adc_wait) must report it, a clean call on the SAME handle afterwards must deliver the undisturbed
outputs, and no device memory may stay behind.  Prints one JSON object; the test asserts on it."""
import ctypes as C
import json
import sys

import numpy as np

import adcensus_amd as A
from adcensus_amd import workloads

CALIB = (3740.0, 0.16, 128.0, 72.0, 0.0)


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
        return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))

    def host_call(st):
        return st.match_out(left, right, CALIB, depth=True, cloud=True, disp8=True)

    # ---- undisturbed results and the number of HIP calls of each form (second call: the scratch exists)
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    L.adc_test_fail_at(0)
    want = host_call(st)
    first_calls = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    host_call(st)
    host_calls = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    st.match(left, right)
    plain_calls = int(L.adc_test_hip_calls())
    st.Release()
    out["first_calls"], out["host_calls"], out["plain_calls"] = first_calls, host_calls, plain_calls
    L.adc_device_synchronize()
    base = free_bytes(hip)  # (after one handle has come and gone: the runtime's own pools exist)

    # ---- adc_match_out on a FRESH handle (its first call allocates the scratch): every call fails once
    not_failed, wrong_after = [], []
    for k in range(1, first_calls + 1):
        st = A.ADCensusStereo(device=0)
        L.adc_test_fail_at(0)
        assert st.Initialize(W, H, opt)
        L.adc_test_fail_at(k)
        d, z, g = np.empty((H, W), np.float32), np.empty((H, W), np.float32), np.empty((H, W), np.uint8)
        pts = np.empty(n, A.POINT_DTYPE)
        ok = st.MatchOut(left, right, d, CALIB, z, pts, g)
        L.adc_test_fail_at(0)
        if ok:
            not_failed.append(k)
        if not same(host_call(st), want) or not same(host_call(st), want):
            wrong_after.append(k)
        if not np.array_equal(st.match(left, right).view(np.uint32), want[0].view(np.uint32)):
            wrong_after.append(-k)
        st.Release()
    out["host_not_failed"], out["host_wrong_after"] = not_failed, wrong_after
    L.adc_device_synchronize()
    out["host_leak_bytes"] = base - free_bytes(hip)

    # ---- adc_match_device_out + adc_wait, and adc_reproject_device + adc_wait, on one handle
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, 4 * n, 16 * n, 16, n)]
    dl, dr, dd, pz, pc, pn, pg = bufs
    assert L.adc_memcpy_h2d(dl, np.ascontiguousarray(left).ctypes.data, 3 * n) == 0
    assert L.adc_memcpy_h2d(dr, np.ascontiguousarray(right).ctypes.data, 3 * n) == 0

    def fetch():
        d, z, g = np.empty((H, W), np.float32), np.empty((H, W), np.float32), np.empty((H, W), np.uint8)
        pts = np.empty(st.cloud_count(), A.POINT_DTYPE)
        for arr, p in ((d, dd), (z, pz), (g, pg), (pts, pc)):
            assert L.adc_memcpy_d2h(arr.ctypes.data, p, arr.nbytes) == 0
        return d, z, pts, g

    def device_call():
        return st.match_device_out(dl, dr, dd, CALIB, pz, pc, n, pn, pg) and st.wait()

    def reproject_call():
        return st.reproject_device(dd, dl, CALIB, pz, pc, n, pn, pg) and st.wait()

    for name, call in (("device", device_call), ("reproject", reproject_call)):
        L.adc_test_fail_at(0)
        assert st.match_device(dl, dr, dd) and st.wait()
        out["device_plain_calls"] = int(L.adc_test_hip_calls())
        assert device_call() and call() and same(fetch(), want), name
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
            if not (device_call() and call() and same(fetch(), want)):
                wrong_after.append(k)
        out[name + "_calls"], out[name + "_not_failed"], out[name + "_wrong_after"] = calls, not_failed, wrong_after
    st.Release()
    for b in bufs:
        L.adc_device_free(b)
    L.adc_device_synchronize()
    out["final_leak_bytes"] = base - free_bytes(hip)
    print("FAULT_PROBE " + json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
