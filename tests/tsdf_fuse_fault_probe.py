"""Runs inside a subprocess of tests/test_gpu_tsdf_fuse_faults.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py
has the background): every HIP call of the stereo-aware fusion fails once -- a device scenario (adc_tsdf_create,
adc_tsdf_weights_device, adc_tsdf_fuse_device, each with adc_wait, adc_tsdf_download) and a host scenario (adc_tsdf_create,
adc_tsdf_weights, adc_tsdf_fuse, adc_tsdf_download), on fresh handles, so that every first-use allocation is among them, and the device
scenario on a handle that has done it all before.  The failures are injected return codes; no kernel is made to fault.  The failing
call must report it with code 2, the same scenario on the SAME handle afterwards (it begins with adc_tsdf_create, which replaces the
volume) must deliver the weight map, the volume and the reports of tests/tsdf_fuse_ref.py byte for byte, a Match must still be exact,
and no device memory may stay behind (hipMemGetInfo and adc_test_live_buffers).  Prints one JSON object; the test asserts on it."""
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
from tests import tsdf_fuse_cases as FC  # noqa: E402
from tests.test_tsdf_api import c_frame, c_params  # noqa: E402
from tests.test_tsdf_fuse_api import c_fuse_params, c_weight_params, fuse_words, weight_words  # noqa: E402


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
    c, r = FC.case("long_row"), FC.reference("long_row")  # one frame: provenance, confidence, computed weights, bilinear; the colour stays out
    W, H = c["size"]
    D = 16
    f = c["frames"][0]
    left, right = workloads.structured_pair(W, H, D, seed=31)
    opt = A.ADCensusOption(max_disparity=D, do_filling=0)
    p = dict(c["params"], flags=0)
    params, frame, wp, fp = c_params(p), c_frame(f["frame"]), c_weight_params(f["wparams"]), c_fuse_params(f["fp"])
    wmap, tsdf = r["wmaps"][0], r["final"][0]
    want = (wmap.tobytes() + np.array(weight_words(r["wreports"][0]), np.uint32).tobytes() + np.array(fuse_words(r["reports"][0]), np.uint32).tobytes() + tsdf.tobytes())
    out = dict(updated=r["reports"][0]["updated"], interpolated=r["reports"][0]["interpolated"], nonzero=r["wreports"][0]["nonzero"])
    codes = set()  # every return code other than 0 the entry points gave

    def must(rc):
        if rc is True or rc == 0:
            return
        if rc is not False:
            codes.add(int(rc))
        raise Failed(A.last_error())

    live0 = int(L.adc_test_live_buffers())
    st = A.ADCensusStereo(device=0)
    L.adc_test_fail_at(0)
    assert st.Initialize(W, H, opt)
    arrays = [np.ascontiguousarray(f["map"], np.float32), np.ascontiguousarray(f["prov"], np.uint8), np.ascontiguousarray(f["conf"], np.float32)]
    bufs = [L.adc_device_malloc(a.nbytes) for a in arrays] + [L.adc_device_malloc(W * H)]
    for a, b in zip(arrays, bufs):
        assert L.adc_memcpy_h2d(b, a.ctypes.data, a.nbytes) == 0
    dm, dp, dc, dw = bufs
    want_d = st.match(left, right)

    def volume(s):
        try:
            return s.tsdf_download()[0].tobytes()
        except RuntimeError as exc:
            raise Failed(str(exc))

    def device_scenario(s):
        must(L.adc_tsdf_create(s._h, C.byref(params)))
        must(L.adc_tsdf_weights_device(s._h, dm, dp, dc, C.byref(frame), C.byref(wp), dw))
        must(L.adc_wait(s._h))
        wrep = s.tsdf_fuse_report()[1]
        must(L.adc_tsdf_fuse_device(s._h, dm, None, dw, C.byref(frame), C.byref(fp)))
        must(L.adc_wait(s._h))
        frep = s.tsdf_fuse_report()[0]
        got = np.empty(W * H, np.uint8)
        assert L.adc_memcpy_d2h(got.ctypes.data, dw, W * H) == 0
        return got.tobytes() + bytes(wrep) + bytes(frep) + volume(s)

    def host_scenario(s):
        must(L.adc_tsdf_create(s._h, C.byref(params)))
        w, wrep, frep = np.zeros((H, W), np.uint8), A.TsdfWeightReport(), A.TsdfFuseReport()
        must(L.adc_tsdf_weights(s._h, arrays[0].ctypes.data, arrays[1].ctypes.data, arrays[2].ctypes.data, C.byref(frame), C.byref(wp), w.ctypes.data, C.byref(wrep)))
        must(L.adc_tsdf_fuse(s._h, arrays[0].ctypes.data, None, w.ctypes.data, C.byref(frame), C.byref(fp), C.byref(frep)))
        return w.tobytes() + bytes(wrep) + bytes(frep) + volume(s)

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
