"""Runs inside a subprocess of tests/test_gpu_products.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the
background).  First the hooked-call counts: adc_match, adc_match_async + adc_wait and adc_farm_submit + drain against the products
entry points with a NULL and with an empty request, in the same run.  Then every HIP call of an adc_match_async_products + adc_wait
with every product (on a fresh handle: the first-use allocations included) and of an adc_farm_submit_products + drain fails once -- a
host-side injected return code.  The call or its wait must report it, the next call on the SAME handle / farm must be exact, and no
device or pinned memory may stay behind.  Prints one JSON object; the test asserts on it."""
import ctypes as C
import json
import sys

import numpy as np

import adcensus_amd as A
from adcensus_amd import workloads

CALIB = (3740.0, 0.16, 64.0, 40.0, 0.5)
W, H, D = 128, 80, 32
N = W * H


def free_bytes(hip):
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def request():
    """(map, every product array, the adc_products) -- fresh arrays"""
    d = np.zeros((H, W), np.float32)
    arrays = dict(provenance=np.zeros((H, W), np.uint8), confidence=np.zeros((H, W), np.float32), depth=np.zeros((H, W), np.float32),
                  cloud=np.zeros(N, A.POINT_DTYPE), disp8=np.zeros((H, W), np.uint8), disp16=np.zeros((H, W), np.uint16))
    return d, arrays, A.Products.from_arrays(calib=CALIB, disp16_scale=256.0, **arrays)


def snapshot(d, arrays, req):
    n = int(req.count[0])
    return [d.tobytes()] + [arrays[k].tobytes() for k in ("provenance", "confidence", "depth", "disp8", "disp16")] + [n, arrays["cloud"][:n].tobytes()]


def main():
    L = A.lib()
    assert hasattr(L, "adc_test_fail_at"), "not the fault-injection build"
    L.adc_test_fail_at.argtypes = [C.c_long]
    L.adc_test_fail_at.restype = None
    L.adc_test_hip_calls.restype = C.c_long
    hip = C.CDLL("libamdhip64.so")
    left, right = workloads.structured_pair(W, H, D, seed=31)
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    lp, rp = left.ctypes.data, right.ctypes.data
    opt = A.ADCensusOption(max_disparity=D, do_filling=0)
    out = {}
    empty = A.Products.from_arrays()

    def calls_of(fn):
        L.adc_test_fail_at(0)
        assert fn(), A.last_error()
        return int(L.adc_test_hip_calls())

    def async_all(st):
        d, arrays, req = request()
        ok = st.match_async_products(left, right, d, req) and st.wait()
        return ok, snapshot(d, arrays, req)

    # ---- the plain paths: a NULL request and an empty one make the HIP calls of the plain entry points
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    d = np.zeros((H, W), np.float32)
    dp = d.ctypes.data
    for _ in range(2):
        assert st.Match(left, right, d)
    plain_map = d.copy()
    out["sync_plain_calls"] = calls_of(lambda: L.adc_match(st._h, lp, rp, dp) == 0)
    out["sync_null_calls"] = calls_of(lambda: L.adc_match_products(st._h, lp, rp, dp, None) == 0)
    out["sync_empty_calls"] = calls_of(lambda: L.adc_match_products(st._h, lp, rp, dp, C.byref(empty)) == 0)
    out["async_plain_calls"] = calls_of(lambda: L.adc_match_async(st._h, lp, rp, dp) == 0 and L.adc_wait(st._h) == 0)
    out["async_null_calls"] = calls_of(lambda: L.adc_match_async_products(st._h, lp, rp, dp, None) == 0 and L.adc_wait(st._h) == 0)
    out["async_empty_calls"] = calls_of(lambda: L.adc_match_async_products(st._h, lp, rp, dp, C.byref(empty)) == 0 and L.adc_wait(st._h) == 0)
    assert d.tobytes() == plain_map.tobytes()
    # ... and the numbers of an asynchronous products Match: the first one allocates, the second one does not
    L.adc_test_fail_at(0)
    ok, want = async_all(st)
    assert ok, A.last_error()
    out["async_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    ok, again = async_all(st)
    assert ok and again == want
    out["async_calls"] = int(L.adc_test_hip_calls())
    st.Release()
    farm = A.PairFarm(W, H, opt, device=0, pipelines=2)
    t = C.c_uint64(0)
    for _ in range(4):
        farm.submit(left, right, d)
    farm.drain()
    out["farm_plain_calls"] = calls_of(lambda: L.adc_farm_submit(farm._f, lp, rp, dp, C.byref(t)) == 0 and L.adc_farm_drain(farm._f) >= 0)
    out["farm_null_calls"] = calls_of(lambda: L.adc_farm_submit_products(farm._f, lp, rp, dp, None, C.byref(t)) == 0 and L.adc_farm_drain(farm._f) >= 0)
    out["farm_empty_calls"] = calls_of(lambda: L.adc_farm_submit_products(farm._f, lp, rp, dp, C.byref(empty), C.byref(t)) == 0 and L.adc_farm_drain(farm._f) >= 0)
    farm.close()
    L.adc_device_synchronize()
    base = free_bytes(hip)  # (after a handle and a farm have come and gone: the runtime's own pools exist)

    # ---- adc_match_async_products + adc_wait on a FRESH handle (its first call allocates scratch and staging): every call fails once
    not_failed, wrong_after = [], []
    for k in range(1, out["async_first_calls"] + 1):
        st = A.ADCensusStereo(device=0)
        L.adc_test_fail_at(0)
        assert st.Initialize(W, H, opt)
        L.adc_test_fail_at(k)
        ok, _ = async_all(st)
        L.adc_test_fail_at(0)
        if ok or not A.last_error():
            not_failed.append(k)
        if async_all(st) != (True, want) or async_all(st) != (True, want):
            wrong_after.append(k)
        if not (st.Match(left, right, d) and d.tobytes() == plain_map.tobytes()):
            wrong_after.append(-k)
        st.Release()
    out["async_not_failed"], out["async_wrong_after"] = not_failed, wrong_after
    L.adc_device_synchronize()
    out["async_leak_bytes"] = base - free_bytes(hip)

    # ---- adc_farm_submit_products + drain on one farm: every call fails once
    farm = A.PairFarm(W, H, opt, device=0, pipelines=2)

    def farm_all():
        d2, arrays, req = request()
        try:
            farm.submit(left, right, d2, req)
            farm.drain()
        except RuntimeError:
            return False, None
        return True, snapshot(d2, arrays, req)

    for _ in range(3):
        assert farm_all() == (True, want)
    L.adc_test_fail_at(0)
    assert farm_all() == (True, want)
    out["farm_calls"] = int(L.adc_test_hip_calls())
    not_failed, wrong_after = [], []
    for k in range(1, out["farm_calls"] + 1):
        L.adc_test_fail_at(k)
        ok, _ = farm_all()
        L.adc_test_fail_at(0)
        if ok:
            not_failed.append(k)
        try:
            farm.drain()  # (whatever the failed attempt left in flight)
        except RuntimeError:
            pass
        if farm_all() != (True, want) or farm_all() != (True, want):
            wrong_after.append(k)
    out["farm_not_failed"], out["farm_wrong_after"] = not_failed, wrong_after
    farm.close()
    L.adc_device_synchronize()
    out["final_leak_bytes"] = base - free_bytes(hip)
    print("FAULT_PROBE " + json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
