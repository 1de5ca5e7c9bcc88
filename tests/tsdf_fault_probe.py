"""Runs inside a subprocess of tests/test_gpu_tsdf_faults.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has
the background): every HIP call of the TSDF paths fails once -- a host scenario (adc_tsdf_create, adc_tsdf_integrate, adc_tsdf_extract
counting and with records, adc_tsdf_download) on fresh handles, so that every first-use allocation is among them, and a device scenario
(adc_tsdf_create, adc_tsdf_upload, adc_tsdf_reset, adc_tsdf_integrate_device, adc_tsdf_extract_device, each with adc_wait,
adc_tsdf_download) on fresh handles and on a handle that has done it all before.  The failures are injected return codes; no kernel is
made to fault.  The failing call must report it with code 2, the same scenario on the SAME handle afterwards (it begins with
adc_tsdf_create, which replaces the volume) must deliver the undisturbed volume, points and reports, a Match must still be exact, and
no device memory may stay behind (hipMemGetInfo and adc_test_live_buffers).  Prints one JSON object; the test asserts on it.
`--counts-only`: just the number of hooked HIP calls of adc_create, of a plain adc_match and of a plain adc_match_device + adc_wait,
on a handle that has never had a volume and again ("after_" keys) while it has one that frames were fused into."""
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


class Failed(Exception):
    pass


def must(ok):
    if not ok:
        raise Failed(A.last_error())


def main():
    L = A.lib()
    assert hasattr(L, "adc_test_fail_at"), "not the fault-injection build"
    L.adc_test_fail_at.argtypes = [C.c_long]
    L.adc_test_fail_at.restype = None
    L.adc_test_hip_calls.restype = C.c_long
    L.adc_test_live_buffers.restype = C.c_long
    hip = C.CDLL("libamdhip64.so")
    W, H, D = 256, 144, 64
    n = W * H
    left, right = workloads.structured_pair(W, H, D, seed=31)
    opt = A.ADCensusOption(max_disparity=D, do_filling=0)
    frame = A.TsdfFrame((900.0, 0.16, W / 2 - 0.3, H / 2 + 0.2, 0.75))
    params = A.TsdfParams(64, 36, 64, 0.04, (-1.28, -0.72, 4.0), 0.12, max_weight=8, flags=A.TSDF_COLOR)  # around the scene's median depth
    out = {}

    live0 = int(L.adc_test_live_buffers())
    st = A.ADCensusStereo(device=0)
    L.adc_test_fail_at(0)
    assert st.Initialize(W, H, opt)
    out["create_calls"] = int(L.adc_test_hip_calls())
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, 16 * 3 * 64 * 36 * 64, 4)]
    dl, dr, dd, dp, dc = bufs
    assert L.adc_memcpy_h2d(dl, np.ascontiguousarray(left).ctypes.data, 3 * n) == 0
    assert L.adc_memcpy_h2d(dr, np.ascontiguousarray(right).ctypes.data, 3 * n) == 0
    want_d = st.match(left, right)

    def plain_counts(prefix):
        L.adc_test_fail_at(0)
        st.match(left, right)
        out[prefix + "plain_calls"] = int(L.adc_test_hip_calls())
        L.adc_test_fail_at(0)
        assert st.match_device(dl, dr, dd) and st.wait()
        out[prefix + "device_plain_calls"] = int(L.adc_test_hip_calls())

    plain_counts("")

    def volume_bytes(s):
        t, c = s.tsdf_download()
        return t.tobytes() + c.tobytes()

    def host_scenario(s):
        try:
            must(s.tsdf_create(params))
            r1 = s.tsdf_integrate(want_d, frame, left)
            r2 = s.tsdf_integrate(want_d, frame, None)
            pts, xrep = s.tsdf_extract()
            return bytes(r1) + bytes(r2) + pts.tobytes() + bytes(xrep) + volume_bytes(s)
        except RuntimeError as exc:
            raise Failed(str(exc))

    L.adc_test_fail_at(0)
    want = host_scenario(st)
    out["host_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert host_scenario(st) == want
    out["host_calls"] = int(L.adc_test_hip_calls())
    irep, xrep = st.tsdf_report()
    out["updated"], out["points"] = int(irep.updated), int(xrep.points)
    assert L.adc_memcpy_h2d(dd, np.ascontiguousarray(want_d).ctypes.data, 4 * n) == 0
    cap = int(xrep.points)

    def device_scenario(s):
        try:
            must(s.tsdf_create(params))
            t0 = np.full((64, 36, 64), 0x00050123, np.uint32)
            s.tsdf_upload(t0, t0)
            must(s.tsdf_reset())
            must(s.wait())
            must(s.tsdf_integrate_device(dd, frame, dl))
            must(s.wait())
            r1 = s.tsdf_report()[0]
            must(s.tsdf_integrate_device(dd, frame, None))
            must(s.wait())
            r2 = s.tsdf_report()[0]
            must(s.tsdf_extract_device(dp, cap, None, dc))
            must(s.wait())
            x = s.tsdf_report()[1]
            cnt = np.empty(1, np.uint32)
            assert L.adc_memcpy_d2h(cnt.ctypes.data, dc, 4) == 0 and int(cnt[0]) == x.points == cap
            pts = np.empty(16 * cap, np.uint8)
            assert L.adc_memcpy_d2h(pts.ctypes.data, dp, 16 * cap) == 0
            return bytes(r1) + bytes(r2) + pts.tobytes() + bytes(x) + volume_bytes(s)
        except RuntimeError as exc:
            raise Failed(str(exc))

    L.adc_test_fail_at(0)
    assert device_scenario(st) == want
    out["device_calls"] = int(L.adc_test_hip_calls())
    plain_counts("after_")
    if "--counts-only" in sys.argv:
        st.Release()
        for b in bufs:
            L.adc_device_free(b)
        print("FAULT_PROBE " + json.dumps(out))
        return 0
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
            if k % 4 == 0 and not np.array_equal(s.match(left, right).view(np.uint32), want_d.view(np.uint32)):
                wrong_after.append(-1000 - k)
            s.Release()
            if int(L.adc_test_live_buffers()) != live0:
                live.append(k)
        out[name + "_first_calls"] = calls
        out[name + "_not_failed"], out[name + "_wrong_after"], out[name + "_live_after"] = not_failed, wrong_after, live
    L.adc_device_synchronize()
    out["final_leak_bytes"] = base - free_bytes(hip)  # (`base` was taken with the probe's own buffers allocated: they are freed behind this)
    out["final_live"] = int(L.adc_test_live_buffers()) - live0
    for b in bufs:
        L.adc_device_free(b)
    print("FAULT_PROBE " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
