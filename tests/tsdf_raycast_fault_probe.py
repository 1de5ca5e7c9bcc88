"""Runs inside a subprocess of tests/test_gpu_tsdf_raycast_faults.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so
(tests/fault_probe.py has the background): every HIP call of the TSDF ray cast paths fails once -- a host scenario (adc_tsdf_create,
adc_tsdf_upload, adc_tsdf_raycast with all four outputs) and a device scenario (adc_tsdf_create, adc_tsdf_upload,
adc_tsdf_raycast_device for the depth alone and for all four outputs, each with adc_wait), on fresh handles, so that every first-use
allocation is among them, and the device scenario on a handle that has done it all before.  The failures are injected return codes;
no kernel is made to fault.  The failing call must report it with code 2, the same scenario on the SAME handle afterwards must
deliver the maps of tests/tsdf_raycast_ref.py, a Match must still be exact, and no device memory may stay behind (hipMemGetInfo and
adc_test_live_buffers).  Prints one JSON object; the test asserts on it."""
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
from tests import tsdf_raycast_cases as RC  # noqa: E402
from tests import tsdf_raycast_ref as RR  # noqa: E402
from tests import tsdf_ref as T  # noqa: E402
from tests.test_tsdf_api import c_params  # noqa: E402
from tests.test_tsdf_raycast_api import c_view  # noqa: E402


def free_bytes(hip):
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


class Failed(Exception):
    pass


def main():
    L = A.lib()
    assert hasattr(L, "adc_test_fail_at"), "not the fault-injection build"
    L.adc_test_fail_at.argtypes = [C.c_long]
    L.adc_test_fail_at.restype = None
    L.adc_test_hip_calls.restype = C.c_long
    L.adc_test_live_buffers.restype = C.c_long
    hip = C.CDLL("libamdhip64.so")
    W, H, D = 128, 96, 32
    left, right = workloads.structured_pair(W, H, D, seed=31)
    opt = A.ADCensusOption(max_disparity=D, do_filling=0)
    case = RC.case("rotated")
    params, view = c_params(case["params"]), c_view(case["view"])
    ref = RC.reference("rotated")
    P = case["view"]["width"] * case["view"]["height"]
    want = b"".join(ref[k].tobytes() for k in ("depth", "normals", "bgr", "status")) + bytes(np.array(RR.report_words(ref["report"]) + [0] * 8, np.uint32))
    out = dict(hits=ref["report"]["hit"])
    codes = set()  # every return code other than 0 the entry points gave

    def must(rc):
        """rc: a C return code, or the bool of the Python mirror (False = a failure whose code the mirror hid: adc_tsdf_create)"""
        if rc is True or rc == 0:
            return
        if rc is not False:
            codes.add(int(rc))
        raise Failed(A.last_error())

    live0 = int(L.adc_test_live_buffers())
    st = A.ADCensusStereo(device=0)
    L.adc_test_fail_at(0)
    assert st.Initialize(W, H, opt)
    bufs = [L.adc_device_malloc(s) for s in (4 * P, 16 * P, 3 * P, P)]
    dd, dn, dc, ds = bufs
    want_d = st.match(left, right)

    def upload(s):
        try:
            s.tsdf_upload(*case["volume"])
        except RuntimeError as exc:
            raise Failed(str(exc))

    def host_scenario(s):
        must(L.adc_tsdf_create(s._h, C.byref(params)))
        upload(s)
        d, n, c, t, rep = np.zeros(P, np.float32), np.zeros(4 * P, np.float32), np.zeros(3 * P, np.uint8), np.zeros(P, np.uint8), A.TsdfRaycastReport()
        must(L.adc_tsdf_raycast(s._h, C.byref(view), d.ctypes.data, n.ctypes.data, c.ctypes.data, t.ctypes.data, C.byref(rep)))
        return d.tobytes() + n.tobytes() + c.tobytes() + t.tobytes() + bytes(rep)

    def device_scenario(s):
        must(L.adc_tsdf_create(s._h, C.byref(params)))
        upload(s)
        must(L.adc_tsdf_raycast_device(s._h, C.byref(view), dd, None, None, None))  # (the depth alone)
        must(L.adc_wait(s._h))
        must(L.adc_tsdf_raycast_device(s._h, C.byref(view), dd, dn, dc, ds))
        must(L.adc_wait(s._h))
        rep = s.tsdf_raycast_report()
        got = [np.empty(n, np.uint8) for n in (4 * P, 16 * P, 3 * P, P)]
        for a, p in zip(got, bufs):
            assert L.adc_memcpy_d2h(a.ctypes.data, p, a.nbytes) == 0
        return b"".join(a.tobytes() for a in got) + bytes(rep)

    L.adc_test_fail_at(0)
    assert device_scenario(st) == want
    L.adc_test_fail_at(0)
    assert device_scenario(st) == want
    out["device_calls"] = int(L.adc_test_hip_calls())
    # the handle that has done it all before: every call of the device scenario fails once
    not_failed, wrong_after = [], []
    for k in range(1, out["device_calls"] + 1):
        L.adc_test_fail_at(k)
        try:
            device_scenario(st)
            not_failed.append(k)
        except Failed as exc:
            if "adc_" not in str(exc):
                not_failed.append(-k)
        L.adc_test_fail_at(0)
        if device_scenario(st) != want:
            wrong_after.append(k)
    if not np.array_equal(st.match(left, right).view(np.uint32), want_d.view(np.uint32)):
        wrong_after.append(-1000)
    if st.tsdf_extract()[0].tobytes() != T.extract(case["volume"], case["params"], 1)[0].tobytes():  # (the volume was only read)
        wrong_after.append(-2000)
    out["device_not_failed"], out["device_wrong_after"] = not_failed, wrong_after
    st.Release()
    L.adc_device_synchronize()
    base = free_bytes(hip)  # (after one handle has come and gone: the runtime's own pools exist)
    out["live_after_release"] = int(L.adc_test_live_buffers()) - live0

    # ---- FRESH handles (first use: the allocations): every call of either scenario fails once
    for name, scenario in (("host", host_scenario), ("fresh_device", device_scenario)):
        L.adc_test_fail_at(0)
        s = A.ADCensusStereo(device=0)
        assert s.Initialize(W, H, opt)
        L.adc_test_fail_at(0)
        assert scenario(s) == want
        calls = int(L.adc_test_hip_calls())
        s.Release()
        not_failed, wrong_after, live = [], [], []
        for k in range(1, calls + 1):
            s = A.ADCensusStereo(device=0)
            L.adc_test_fail_at(0)
            assert s.Initialize(W, H, opt)
            L.adc_test_fail_at(k)
            try:
                scenario(s)
                not_failed.append(k)
            except Failed as exc:
                if "adc_" not in str(exc):
                    not_failed.append(-k)
            L.adc_test_fail_at(0)
            if scenario(s) != want:
                wrong_after.append(k)
            if k % 8 == 0 and not np.array_equal(s.match(left, right).view(np.uint32), want_d.view(np.uint32)):
                wrong_after.append(-1000 - k)
            s.Release()
            if int(L.adc_test_live_buffers()) != live0:
                live.append(k)
        out[name + "_first_calls"] = calls
        out[name + "_not_failed"], out[name + "_wrong_after"], out[name + "_live_after"] = not_failed, wrong_after, live
    L.adc_device_synchronize()
    out["final_leak_bytes"] = base - free_bytes(hip)  # (`base` was taken with the probe's own buffers allocated: they are freed behind this)
    out["final_live"] = int(L.adc_test_live_buffers()) - live0
    out["codes"] = sorted(codes)
    for b in bufs:
        L.adc_device_free(b)
    print("FAULT_PROBE " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
