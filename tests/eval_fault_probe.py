"""Runs inside a subprocess of tests/test_gpu_eval.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the
background): every HIP call of an adc_set_ground_truth (first use: the allocations), of an adc_evaluate with every input and output
(first use: its scratch) and of an adc_evaluate_device + adc_wait fails once.  The failures are injected return codes; no kernel is
made to fault.  The call (or its adc_wait) must report it, clean calls on the SAME handle afterwards must deliver the undisturbed
report and maps, a Match must still be exact, and no device memory may stay behind.  Prints one JSON object; the test asserts on it.
`--counts-only`: just the number of hooked HIP calls of adc_create, and -- after adc_set_ground_truth followed by
adc_clear_ground_truth -- of a plain adc_match and of a plain adc_match_device + adc_wait."""
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

THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


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
    rng = np.random.default_rng(77)
    gl = rng.integers(0, 4 * D, (H, W)).astype(np.uint8)
    gl[rng.random((H, W)) < 0.05] = 0
    gr = np.roll(gl, -9, axis=1)
    out = {}

    def set_gt(st):
        st.set_ground_truth(gl, gr, scale=4.0)

    st = A.ADCensusStereo(device=0)
    L.adc_test_fail_at(0)
    assert st.Initialize(W, H, opt)
    out["create_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    set_gt(st)
    out["set_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    set_gt(st)
    out["set_calls"] = int(L.adc_test_hip_calls())
    st.clear_ground_truth()
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, n, 4 * n, 4 * n, n)]
    dl, dr, dd, dp, dc, de, dk = bufs
    assert L.adc_memcpy_h2d(dl, np.ascontiguousarray(left).ctypes.data, 3 * n) == 0
    assert L.adc_memcpy_h2d(dr, np.ascontiguousarray(right).ctypes.data, 3 * n) == 0
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
    d, prov, conf = st.match_ex(left, right)
    assert np.array_equal(d.view(np.uint32), want_d.view(np.uint32))
    set_gt(st)

    def host_eval(s):
        rep, err, cls = s.evaluate(d, prov, conf, THRESHOLDS)
        return rep.words().tobytes() + bytes(rep)[A.EvalReport.thresholds.offset:] + err.tobytes() + cls.tobytes()

    L.adc_test_fail_at(0)
    want = host_eval(st)
    out["eval_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert host_eval(st) == want
    out["eval_calls"] = int(L.adc_test_hip_calls())
    out["known"] = int(st.eval_report().all.pixels)
    st.Release()
    L.adc_device_synchronize()
    base = free_bytes(hip)  # (after one handle has come and gone: the runtime's own pools exist)

    # ---- adc_set_ground_truth and adc_evaluate on FRESH handles (first use: the allocations): every call fails once
    for name, calls in (("set", out["set_first_calls"]), ("eval", out["eval_first_calls"])):
        not_failed, wrong_after = [], []
        for k in range(1, calls + 1):
            s = A.ADCensusStereo(device=0)
            L.adc_test_fail_at(0)
            assert s.Initialize(W, H, opt)
            if name == "eval":
                set_gt(s)
            L.adc_test_fail_at(k)
            try:
                set_gt(s) if name == "set" else host_eval(s)
                not_failed.append(k)
            except RuntimeError:
                if not A.last_error():
                    not_failed.append(-k)
            L.adc_test_fail_at(0)
            if name == "set":  # a failed set call leaves ground truth unset: an evaluation is refused, not wrong
                if s.evaluate_device(dd) or "no ground truth" not in A.last_error():
                    wrong_after.append(-k)
                set_gt(s)
            if host_eval(s) != want or host_eval(s) != want:
                wrong_after.append(k)
            if not np.array_equal(s.match(left, right).view(np.uint32), want_d.view(np.uint32)):
                wrong_after.append(-1000 - k)
            s.Release()
        out[name + "_not_failed"], out[name + "_wrong_after"] = not_failed, wrong_after
        L.adc_device_synchronize()
        out[name + "_leak_bytes"] = base - free_bytes(hip)

    # ---- adc_evaluate_device + adc_wait on one handle
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    set_gt(st)
    for arr, p in ((d, dd), (prov, dp), (conf, dc)):
        assert L.adc_memcpy_h2d(p, np.ascontiguousarray(arr).ctypes.data, arr.nbytes) == 0

    def device_call():
        return st.evaluate_device(dd, dp, dc, THRESHOLDS, de, dk) and st.wait()

    def fetch():
        err, cls = np.empty((H, W), np.float32), np.empty((H, W), np.uint8)
        assert L.adc_memcpy_d2h(err.ctypes.data, de, err.nbytes) == 0 and L.adc_memcpy_d2h(cls.ctypes.data, dk, cls.nbytes) == 0
        rep = st.eval_report()
        return rep.words().tobytes() + bytes(rep)[A.EvalReport.thresholds.offset:] + err.tobytes() + cls.tobytes()

    assert device_call() and fetch() == want
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
        if not (device_call() and fetch() == want):
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
