"""Runs inside a subprocess of tests/test_gpu_voxel_faults.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the
background): every HIP call of switching the voxel grid on (first use: the scratch allocations) plus an adc_reproject_device + adc_wait
with a cloud, and of an adc_match_async_products + adc_wait with a cloud, fails once -- the call is NOT made, nothing faults on the
device.  The call (or its adc_wait) must report it, and the SAME handle must deliver the undisturbed voxel cloud afterwards; no device
memory may stay behind.  Also counts the hooked calls of the plain cloud before and after a grid was set and cleared.  Prints one JSON
object; the test asserts on it."""
import ctypes as C
import json
import sys

import numpy as np

import adcensus_amd as A
from adcensus_amd import workloads

LEAF = 0.4


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
    L.adc_test_live_buffers.restype = C.c_long  # (the owner's allocations not yet freed, of any size: the table is below the 2 MiB margin here)
    hip = C.CDLL("libamdhip64.so")
    W, H, D = 96, 64, 16
    n = W * H
    calib = (100.0, 0.5, W / 2.0, H / 2.0, 0.0)
    left, right = workloads.structured_pair(W, H, D, seed=21)
    opt = A.ADCensusOption(max_disparity=D)
    grid = A.VoxelGrid(LEAF)
    out = {}

    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    disp = st.match(left, right)
    bufs = [L.adc_device_malloc(s) for s in (4 * n, 3 * n, 16 * n, 16)]
    dd, dl, pc, pn = bufs
    assert L.adc_memcpy_h2d(dd, disp.ctypes.data, 4 * n) == 0 and L.adc_memcpy_h2d(dl, np.ascontiguousarray(left).ctypes.data, 3 * n) == 0

    def reproject(handle=None):
        h = handle or st
        return h.reproject_device(dd, dl, calib, None, pc, n, pn, None) and h.wait()

    def fetch(handle=None):
        h = handle or st
        pts = np.empty(n, A.POINT_DTYPE)
        assert L.adc_memcpy_d2h(pts.ctypes.data, pc, pts.nbytes) == 0
        return pts[:h.cloud_count()].tobytes(), h.cloud_count()

    def match():
        d = np.empty((H, W), np.float32)
        req = A.Products.from_arrays(calib=calib, cloud=np.zeros(n, A.POINT_DTYPE))
        ok = st.match_async_products(left, right, d, req) and st.wait()
        return ok, req

    # ---- the plain cloud on a handle that never had a grid: its hooked HIP calls (behind the first use of the outputs' own scratch)
    assert reproject()
    L.adc_test_fail_at(0)
    assert reproject()
    out["plain_calls"] = int(L.adc_test_hip_calls())
    want_plain = fetch()
    # ---- the undisturbed voxel results and the number of HIP calls of each form
    L.adc_test_fail_at(0)
    st.set_cloud_voxel_grid(LEAF)
    out["setter_first_calls"] = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    assert reproject()
    out["voxel_calls"] = int(L.adc_test_hip_calls())
    want = fetch()
    want_report = st.voxel_report()
    out["voxels"], out["points"] = want[1], want_plain[1]
    assert 0 < want[1] < want_plain[1]
    L.adc_test_fail_at(0)
    st.set_cloud_voxel_grid(LEAF)
    out["setter_again_calls"] = int(L.adc_test_hip_calls())
    assert match()[0]  # (the first use of the host cloud's scratch is behind it)
    L.adc_test_fail_at(0)
    ok, req = match()
    assert ok
    out["match_calls"] = int(L.adc_test_hip_calls())
    want_match = (req._keep[4][:int(req.count[0])].tobytes(), int(req.count[0]))
    assert want_match == want  # (the same map, the same cloud)
    st.clear_cloud_voxel_grid()
    L.adc_test_fail_at(0)
    assert reproject()
    out["plain_calls_after_clear"] = int(L.adc_test_hip_calls())
    assert fetch() == want_plain
    st.Release()
    out["live_after_first"] = int(L.adc_test_live_buffers())
    L.adc_device_synchronize()
    base = free_bytes(hip)  # (after one handle has come and gone: the runtime's own pools exist)

    # ---- the setter's first use + a reprojection on a FRESH handle: every call fails once
    f = A.ADCensusStereo(device=0)
    assert f.Initialize(W, H, opt)
    L.adc_test_fail_at(0)
    f.set_cloud_voxel_grid(LEAF)
    assert reproject(f) and fetch(f) == want
    out["fresh_calls"] = int(L.adc_test_hip_calls())
    f.Release()
    not_failed, wrong_after = [], []
    for k in range(1, out["fresh_calls"] + 1):
        f = A.ADCensusStereo(device=0)
        L.adc_test_fail_at(0)
        assert f.Initialize(W, H, opt)
        L.adc_test_fail_at(k)
        ok = L.adc_set_cloud_voxel_grid(f._h, C.byref(grid)) == 0 and reproject(f)
        L.adc_test_fail_at(0)
        if ok or not A.last_error():
            not_failed.append(k)
        f.set_cloud_voxel_grid(LEAF)
        if not (reproject(f) and fetch(f) == want and f.voxel_report() == want_report):
            wrong_after.append(k)
        f.Release()
    out["fresh_not_failed"], out["fresh_wrong_after"] = not_failed, wrong_after
    out["live_after_fresh"] = int(L.adc_test_live_buffers())
    L.adc_device_synchronize()
    out["fresh_leak_bytes"] = base - free_bytes(hip)

    # ---- an asynchronous Match with a voxel cloud + adc_wait on one handle
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, opt)
    st.set_cloud_voxel_grid(LEAF)
    assert match()[0]
    not_failed, wrong_after = [], []
    for k in range(1, out["match_calls"] + 1):
        L.adc_test_fail_at(k)
        ok, _ = match()
        L.adc_test_fail_at(0)
        if ok or not A.last_error():
            not_failed.append(k)
        ok, req = match()
        if not (ok and (req._keep[4][:int(req.count[0])].tobytes(), int(req.count[0])) == want and st.voxel_report() == want_report):
            wrong_after.append(k)
    out["match_not_failed"], out["match_wrong_after"] = not_failed, wrong_after
    st.Release()
    out["live_after_match"] = int(L.adc_test_live_buffers())
    for b in bufs:
        L.adc_device_free(b)
    L.adc_device_synchronize()
    out["final_leak_bytes"] = base - free_bytes(hip)
    print("FAULT_PROBE " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
