"""Runs inside a subprocess of tests/test_gpu_register.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the
background): every HIP call of an adc_set_register_target (first use: the allocations), of an adc_register_depth and an adc_align_color
(first use: their scratch) and of adc_register_depth_device / adc_align_color_device + adc_wait fails once.  The failures are injected
return codes; no kernel is made to fault.  The call (or its adc_wait) must report it with code 2, clean calls on the SAME handle
afterwards must deliver the undisturbed maps and report, a Match must still be exact, and no device memory may stay behind.  Prints
one JSON object; the test asserts on it.
`--counts-only`: just the number of hooked HIP calls of adc_create, and -- on a handle that has a target set but does not use it -- of
a plain adc_match and of a plain adc_match_device + adc_wait."""
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
from tests import register_cases as RC  # noqa: E402


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
    Wt, Ht = 300, 170
    n, nt = W * H, Wt * Ht
    left, right = workloads.structured_pair(W, H, D, seed=31)
    opt = A.ADCensusOption(max_disparity=D, do_filling=0)
    calib = A.Calib(*RC.calib_for(W, H))
    target = RC.target("rot5", W, H, Wt, Ht)
    small = RC.target("shift", W, H, 64, 40)
    tbgr = np.random.default_rng(3).integers(1, 256, (Ht, Wt, 3), dtype=np.uint8)
    out = {}

    st = A.ADCensusStereo(device=0)
    L.adc_test_fail_at(0)
    assert st.Initialize(W, H, opt)
    out["create_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    st.set_register_target(small)
    out["set_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    st.set_register_target(target)  # (a larger target: the z-buffer regrows)
    out["set_grow_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    st.set_register_target(target)
    out["set_calls"] = int(L.adc_test_hip_calls())
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, 4 * nt, 4 * nt, 3 * nt, 3 * n, n)]
    dl, dr, dd, dz, di, dt, do, dv = bufs
    assert L.adc_memcpy_h2d(dl, np.ascontiguousarray(left).ctypes.data, 3 * n) == 0
    assert L.adc_memcpy_h2d(dr, np.ascontiguousarray(right).ctypes.data, 3 * n) == 0
    assert L.adc_memcpy_h2d(dt, tbgr.ctypes.data, 3 * nt) == 0
    want_d = st.match(left, right)
    L.adc_test_fail_at(0)
    st.match(left, right)
    out["plain_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert st.match_device(dl, dr, dd) and st.wait()
    out["device_plain_calls"] = int(L.adc_test_hip_calls())
    if "--counts-only" in sys.argv:
        st.Release()
        for b in bufs:
            L.adc_device_free(b)
        print("FAULT_PROBE " + json.dumps(out))
        return 0

    # ---- undisturbed results
    def host_reg(s):
        depth, index, rep = s.register_depth(want_d, calib)
        return depth.tobytes() + index.tobytes() + bytes(rep)

    def host_align(s):
        img, valid = s.align_color(want_d, calib, tbgr)
        return img.tobytes() + valid.tobytes()

    L.adc_test_fail_at(0)
    want_reg = host_reg(st)
    out["reg_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert host_reg(st) == want_reg
    out["reg_calls"] = int(L.adc_test_hip_calls())
    out["filled"] = int(st.register_report().dst_filled)
    st.Release()
    st = A.ADCensusStereo(device=0)  # (a fresh handle: adc_align_color allocates its own scratch, the map's included)
    assert st.Initialize(W, H, opt)
    st.set_register_target(target)
    L.adc_test_fail_at(0)
    want_align = host_align(st)
    out["align_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert host_align(st) == want_align
    out["align_calls"] = int(L.adc_test_hip_calls())
    st.Release()
    L.adc_device_synchronize()
    base = free_bytes(hip)  # (after one handle has come and gone: the runtime's own pools exist)

    # ---- the set call and the two host calls on FRESH handles (first use: the allocations): every call fails once
    for name, calls in (("set", out["set_first_calls"]), ("reg", out["reg_first_calls"]), ("align", out["align_first_calls"])):
        not_failed, wrong_after = [], []
        for k in range(1, calls + 1):
            s = A.ADCensusStereo(device=0)
            L.adc_test_fail_at(0)
            assert s.Initialize(W, H, opt)
            if name != "set":
                s.set_register_target(target)
            L.adc_test_fail_at(k)
            try:
                s.set_register_target(target) if name == "set" else (host_reg(s) if name == "reg" else host_align(s))
                not_failed.append(k)
            except RuntimeError:
                if not A.last_error():
                    not_failed.append(-k)
            L.adc_test_fail_at(0)
            if name == "set":  # a failed set call leaves the target unset: a registration is refused, not wrong
                if s.register_depth_device(dd, calib, d_depth=dz) or "no target set" not in A.last_error():
                    wrong_after.append(-k)
                s.set_register_target(target)
            if host_reg(s) != want_reg or host_align(s) != want_align or host_reg(s) != want_reg:
                wrong_after.append(k)
            if not np.array_equal(s.match(left, right).view(np.uint32), want_d.view(np.uint32)):
                wrong_after.append(-1000 - k)
            s.Release()
        out[name + "_not_failed"], out[name + "_wrong_after"] = not_failed, wrong_after
        L.adc_device_synchronize()
        out[name + "_leak_bytes"] = base - free_bytes(hip)

    # ---- the device forms + adc_wait on one handle
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    st.set_register_target(target)
    assert L.adc_memcpy_h2d(dd, np.ascontiguousarray(want_d).ctypes.data, 4 * n) == 0

    def device_call():
        return st.register_depth_device(dd, calib, d_depth=dz, d_index=di) and st.align_color_device(dd, calib, dt, do, dv) and st.wait()

    def fetch():
        parts = []
        for p, size in ((dz, 4 * nt), (di, 4 * nt), (do, 3 * n), (dv, n)):
            a = np.empty(size, np.uint8)
            assert L.adc_memcpy_d2h(a.ctypes.data, p, size) == 0
            parts.append(a.tobytes())
        return parts[0] + parts[1] + bytes(st.register_report()), parts[2] + parts[3]

    assert device_call() and fetch() == (want_reg, want_align)
    L.adc_test_fail_at(0)
    device_call()
    calls = int(L.adc_test_hip_calls())
    not_failed, wrong_after = [], []
    for k in range(1, calls + 1):
        L.adc_test_fail_at(k)
        ok = device_call()
        L.adc_test_fail_at(0)
        if ok or not A.last_error():
            not_failed.append(k)
        if not (device_call() and fetch() == (want_reg, want_align)):
            wrong_after.append(k)
    out["device_calls"], out["device_not_failed"], out["device_wrong_after"] = calls, not_failed, wrong_after
    if not np.array_equal(st.match(left, right).view(np.uint32), want_d.view(np.uint32)):
        out["device_wrong_after"].append(-1000)
    st.Release()
    L.adc_device_synchronize()
    out["final_leak_bytes"] = base - free_bytes(hip)  # (`base` was taken with the probe's own buffers allocated: they are freed behind this)
    for b in bufs:
        L.adc_device_free(b)
    print("FAULT_PROBE " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
