"""Runs inside a subprocess of tests/test_gpu_mesh.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the
background): every HIP call of an adc_mesh (first use: its scratch and the handle's block of words) and of adc_mesh_device + adc_wait fails
once.  The failures are injected return codes; no kernel is made to fault.  The call (or its adc_wait) must report it with code 2,
clean calls on the SAME handle afterwards must deliver the undisturbed mesh and report, a Match must still be exact, and no device
memory may stay behind (hipMemGetInfo and adc_test_live_buffers).  Prints one JSON object; the test asserts on it.
`--counts-only`: just the number of hooked HIP calls of adc_create, of a plain adc_match and of a plain adc_match_device + adc_wait,
on a handle that has never computed a mesh and again ("after_" keys) once it has, through both entry points."""
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
    calib = A.Calib(900.0, 0.16, W / 2 - 0.3, H / 2 + 0.2, 0.75)
    params = A.MeshParams(1.0, 2)
    wl, hl = (W - 1) // 2 + 1, (H - 1) // 2 + 1
    vcap, tcap = wl * hl, 2 * (wl - 1) * (hl - 1)
    out = {}

    live0 = int(L.adc_test_live_buffers())
    st = A.ADCensusStereo(device=0)
    L.adc_test_fail_at(0)
    assert st.Initialize(W, H, opt)
    out["create_calls"] = int(L.adc_test_hip_calls())
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, 16 * vcap, 4 * vcap, 12 * tcap, 8)]
    dl, dr, dd, dv, dvi, dt, dc = bufs
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

    def host_mesh(s):
        v, vi, t, rep = s.mesh(want_d, calib, params, left)
        return v.tobytes() + vi.tobytes() + t.tobytes() + bytes(rep)

    L.adc_test_fail_at(0)
    want = host_mesh(st)
    out["mesh_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert host_mesh(st) == want
    out["mesh_calls"] = int(L.adc_test_hip_calls())
    out["triangles"] = int(st.mesh_report().triangles)
    assert L.adc_memcpy_h2d(dd, np.ascontiguousarray(want_d).ctypes.data, 4 * n) == 0

    def device_call(s):
        return s.mesh_device(dd, calib, params, dl, dv, vcap, dvi, dt, tcap, dc) and s.wait()

    def fetch(s):
        rep = s.mesh_report()
        cnt = np.empty(2, np.uint32)
        assert L.adc_memcpy_d2h(cnt.ctypes.data, dc, 8) == 0 and cnt.tolist() == [rep.vertices, rep.triangles]
        parts = []
        for p, size in ((dv, 16 * rep.vertices), (dvi, 4 * rep.vertices), (dt, 12 * rep.triangles)):
            a = np.empty(max(size, 1), np.uint8)
            assert size == 0 or L.adc_memcpy_d2h(a.ctypes.data, p, size) == 0
            parts.append(a[:size].tobytes())
        return b"".join(parts) + bytes(rep)

    assert device_call(st) and fetch(st) == want
    plain_counts("after_")
    if "--counts-only" in sys.argv:
        st.Release()
        for b in bufs:
            L.adc_device_free(b)
        print("FAULT_PROBE " + json.dumps(out))
        return 0
    st.Release()
    L.adc_device_synchronize()
    base = free_bytes(hip)  # (after one handle has come and gone: the runtime's own pools exist)
    out["live_after_release"] = int(L.adc_test_live_buffers()) - live0

    # ---- the host call on FRESH handles (first use: the allocations): every call fails once
    not_failed, wrong_after, live = [], [], []
    for k in range(1, out["mesh_first_calls"] + 1):
        s = A.ADCensusStereo(device=0)
        L.adc_test_fail_at(0)
        assert s.Initialize(W, H, opt)
        L.adc_test_fail_at(k)
        try:
            host_mesh(s)
            not_failed.append(k)
        except RuntimeError as exc:
            if not A.last_error() or "adc_mesh" not in str(exc):
                not_failed.append(-k)
        L.adc_test_fail_at(0)
        if host_mesh(s) != want or host_mesh(s) != want:
            wrong_after.append(k)
        if not np.array_equal(s.match(left, right).view(np.uint32), want_d.view(np.uint32)):
            wrong_after.append(-1000 - k)
        s.Release()
        if int(L.adc_test_live_buffers()) != live0:
            live.append(k)
    out["host_not_failed"], out["host_wrong_after"], out["host_live_after"] = not_failed, wrong_after, live
    L.adc_device_synchronize()
    out["host_leak_bytes"] = base - free_bytes(hip)

    # ---- the device form + adc_wait: on a fresh handle (the block of words is allocated by the call), then on the same one
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    L.adc_test_fail_at(0)
    assert device_call(st) and fetch(st) == want
    out["device_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    device_call(st)
    calls = int(L.adc_test_hip_calls())
    not_failed, wrong_after = [], []
    for k in range(1, calls + 1):
        L.adc_test_fail_at(k)
        ok = device_call(st)
        L.adc_test_fail_at(0)
        if ok or not A.last_error():
            not_failed.append(k)
        if not (device_call(st) and fetch(st) == want):
            wrong_after.append(k)
    st.Release()
    for k in range(1, out["device_first_calls"] + 1):  # (first use)
        s = A.ADCensusStereo(device=0)
        L.adc_test_fail_at(0)
        assert s.Initialize(W, H, opt)
        L.adc_test_fail_at(k)
        ok = device_call(s)
        L.adc_test_fail_at(0)
        if ok or not A.last_error():
            not_failed.append(100 + k)
        if not (device_call(s) and fetch(s) == want):
            wrong_after.append(100 + k)
        if not np.array_equal(s.match(left, right).view(np.uint32), want_d.view(np.uint32)):
            wrong_after.append(-1000 - k)
        s.Release()
    out["device_calls"], out["device_not_failed"], out["device_wrong_after"] = calls, not_failed, wrong_after
    L.adc_device_synchronize()
    out["final_leak_bytes"] = base - free_bytes(hip)  # (`base` was taken with the probe's own buffers allocated: they are freed behind this)
    out["final_live"] = int(L.adc_test_live_buffers()) - live0
    for b in bufs:
        L.adc_device_free(b)
    print("FAULT_PROBE " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
