"""Runs inside a subprocess of tests/test_gpu_rawfmt.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the
background): every HIP call of switching the conversion on (adc_set_input_format on both sides, first use) plus a converting adc_match,
of a converting adc_match_device + adc_wait and of an adc_rectify_device + adc_wait on such a side fails once.  The call (or its
adc_wait) must report it, clean calls on the SAME handle afterwards must deliver the undisturbed results, and no device memory may stay
behind.  Prints one JSON object; the test asserts on it."""
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
from tests import rawfmt_ref as RF  # noqa: E402


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

    # the pair as camera frames: Bayer with a padded pitch (left), NV12 (right)
    fmts = [A.RawFormat(W, H, W + 8, A.PIX_BAYER_GBRG8), A.RawFormat(W, H, W, A.PIX_NV12)]
    raws = [RF.pack(left, RF.BAYER_GBRG8, W + 8), RF.pack(right, RF.NV12, W)]
    dec = [RF.decode(r, W, H, f.pitch_bytes, f.format).astype(np.uint8) for r, f in zip(raws, fmts)]

    def set_both(s):
        return L.adc_set_input_format(s._h, 0, C.byref(fmts[0])) == 0 and L.adc_set_input_format(s._h, 1, C.byref(fmts[1])) == 0

    def set_both_checked(s):
        assert set_both(s), A.last_error()
        s._rect.set(0, fmts[0])
        s._rect.set(1, fmts[1])

    # ---- the number of hooked HIP calls of each form, and the undisturbed results
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    st.match(left, right)
    L.adc_test_fail_at(0)
    want = st.match(dec[0], dec[1])
    out["plain_calls"] = int(L.adc_test_hip_calls())
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, 3 * n)]
    dl, dr, dd, dout = bufs
    assert L.adc_memcpy_h2d(dl, dec[0].ctypes.data, 3 * n) == 0 and L.adc_memcpy_h2d(dr, dec[1].ctypes.data, 3 * n) == 0
    L.adc_test_fail_at(0)
    assert st.match_device(dl, dr, dd) and st.wait()
    out["device_plain_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert L.adc_set_input_format(st._h, 0, C.byref(fmts[0])) == 0
    out["set_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert L.adc_set_input_format(st._h, 1, C.byref(fmts[1])) == 0
    out["set_other_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert L.adc_set_input_format(st._h, 0, C.byref(fmts[0])) == 0
    out["set_again_calls"] = int(L.adc_test_hip_calls())
    set_both_checked(st)
    assert np.array_equal(st.rectify(raws[0], 0), dec[0]) and np.array_equal(st.rectify(raws[1], 1), dec[1])
    assert same(st.match(raws[0], raws[1]), want)
    L.adc_test_fail_at(0)
    st.match(raws[0], raws[1])
    out["conv_calls"] = int(L.adc_test_hip_calls())
    st.Release()
    L.adc_device_synchronize()
    base = free_bytes(hip)  # (after handles have come and gone: the runtime's own pools exist)

    # ---- both set calls' first use + a converting adc_match on a FRESH handle: every call fails once
    first = out["set_first_calls"] + out["set_other_calls"] + out["conv_calls"]
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
        if not same(st.match(raws[0], raws[1]), want) or not same(st.match(raws[0], raws[1]), want):
            wrong_after.append(k)
        st.clear_rectify()
        if not same(st.match(dec[0], dec[1]), want):
            wrong_after.append(-k)
        st.Release()
    out["host_not_failed"], out["host_wrong_after"] = not_failed, wrong_after
    L.adc_device_synchronize()
    out["host_leak_bytes"] = base - free_bytes(hip)

    # ---- a converting adc_match_device + adc_wait and adc_rectify_device + adc_wait on one handle
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    set_both_checked(st)
    raw_bufs = [L.adc_device_malloc(r.nbytes) for r in raws]
    for p, r in zip(raw_bufs, raws):
        assert L.adc_memcpy_h2d(p, r.ctypes.data, r.nbytes) == 0

    def fetch(p, shape, dtype):
        d = np.empty(shape, dtype)
        assert L.adc_memcpy_d2h(d.ctypes.data, p, d.nbytes) == 0
        return d

    def device_call():
        return st.match_device(raw_bufs[0], raw_bufs[1], dd) and st.wait()

    def convert_call():
        assert L.adc_memcpy_h2d(dout, np.zeros(3 * n, np.uint8).ctypes.data, 3 * n) == 0
        return st.rectify_device(1, raw_bufs[1], dout) and st.wait()

    def all_good():
        return (device_call() and same(fetch(dd, (H, W), np.float32), want) and convert_call() and
                np.array_equal(fetch(dout, (H, W, 3), np.uint8), dec[1]))

    assert all_good()
    for name, call in (("device", device_call), ("convert", convert_call)):
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
