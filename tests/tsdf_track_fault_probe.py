"""Runs inside a subprocess of tests/test_gpu_tsdf_track_faults.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py
has the background): every HIP call of the tracking paths fails once -- a device scenario (adc_track_device with a device record,
adc_wait) and a host scenario (adc_tsdf_create, adc_tsdf_upload, adc_tsdf_track), on fresh handles, so that every first-use allocation
is among them, and the device scenario on a handle that has done it all before.  The failures are injected return codes; no kernel is
made to fault.  The failing call must report it with code 2, the same scenario on the SAME handle afterwards must deliver the record of
tests/tsdf_track_ref.py byte for byte, a Match must still be exact, and no device memory may stay behind (hipMemGetInfo and
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
from tests import tsdf_raycast_ref as RR  # noqa: E402
from tests import tsdf_track_cases as KC  # noqa: E402
from tests import tsdf_track_checks as K  # noqa: E402
from tests import tsdf_track_ref as TR  # noqa: E402
from tests.test_tsdf_api import c_frame, c_params  # noqa: E402
from tests.test_tsdf_track_api import c_model, c_track_params  # noqa: E402

ITERATIONS = 3


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
    W, H, D = 64, 48, 16
    left, right = workloads.structured_pair(W, H, D, seed=31)
    opt = A.ADCensusOption(max_disparity=D, do_filling=0)
    # the device scenario: analytic model maps; the host scenario: the volume of the chain check, cast by the call itself
    c = KC.scene(W, H, KC.A_POSE, KC.SMALL, planes=K.DIAGONAL3, iterations=ITERATIONS)
    frame, model, tp = c_frame(c["frame"]), c_model(c["model"]), c_track_params(c["params"])
    want_dev = TR.result_bytes(TR.track(c["map"], None, c["frame"], c["model"], c["mdepth"], c["mnormals"], c["params"]))
    big = K.chain_case()
    vp, vol = big["volume_params"], big["volume"]
    focal, _, cx, cy, _ = c["frame"]["calib"]
    cast = RR.raycast(vol, vp, dict(big["view"], width=W, height=H, focal_px=focal, cx=cx, cy=cy))
    ref_host = TR.track(c["map"], None, c["frame"], TR.model(W, H, focal, cx, cy, *KC.A_POSE), cast["depth"], cast["normals"], c["params"])
    want_host = TR.result_bytes(ref_host)
    params = c_params(vp)
    out = dict(used=ref_host["counts"]["used"], solves=ref_host["solves"])
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
    arrays = [np.ascontiguousarray(c[k], np.float32) for k in ("map", "mdepth", "mnormals")]
    bufs = [L.adc_device_malloc(a.nbytes) for a in arrays] + [L.adc_device_malloc(960)]
    for a, b in zip(arrays, bufs):
        assert L.adc_memcpy_h2d(b, a.ctypes.data, a.nbytes) == 0
    dm, dd, dn, dr = bufs
    want_d = st.match(left, right)
    host_map = arrays[0]

    def device_scenario(s):
        must(L.adc_track_device(s._h, dm, None, C.byref(frame), C.byref(model), dd, dn, C.byref(tp), dr))
        must(L.adc_wait(s._h))
        got = np.empty(960, np.uint8)
        assert L.adc_memcpy_d2h(got.ctypes.data, dr, 960) == 0
        res = s.track_result()
        return got.tobytes() + (b"" if res is None else bytes(res))

    def host_scenario(s):
        must(L.adc_tsdf_create(s._h, C.byref(params)))
        try:
            s.tsdf_upload(*vol)
        except RuntimeError as exc:
            raise Failed(str(exc))
        res = A.TrackResult()
        must(L.adc_tsdf_track(s._h, host_map.ctypes.data, C.byref(frame), C.byref(tp), C.byref(res)))
        return bytes(res)

    L.adc_test_fail_at(0)
    assert device_scenario(st) == want_dev + want_dev
    L.adc_test_fail_at(0)
    assert device_scenario(st) == want_dev + want_dev
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
        if device_scenario(st) != want_dev + want_dev:
            wrong_after.append(k)
    if not np.array_equal(st.match(left, right).view(np.uint32), want_d.view(np.uint32)):
        wrong_after.append(-1000)
    out["device_not_failed"], out["device_wrong_after"] = not_failed, wrong_after
    st.Release()
    L.adc_device_synchronize()
    base = free_bytes(hip)  # (after one handle has come and gone: the runtime's own pools exist)
    out["live_after_release"] = int(L.adc_test_live_buffers()) - live0

    # ---- FRESH handles (first use: the allocations): every call of either scenario fails once
    for name, scenario, want in (("host", host_scenario, want_host), ("fresh_device", device_scenario, want_dev + want_dev)):
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
