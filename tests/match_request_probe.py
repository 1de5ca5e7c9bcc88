"""Runs inside a subprocess of tests/test_gpu_match_request.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has
the background).  No call is made to fail here: the build is used for its counter of hooked HIP calls.  On one warm handle, each older
entry point and its adc_*_products twin are called with the same request and the calls of each are counted -- one path delivers for
both, so the counts are equal.  Prints one JSON object; the test asserts on it."""
import ctypes as C
import json
import sys

import numpy as np

import adcensus_amd as A
from adcensus_amd import workloads

CALIB = (3740.0, 0.16, 64.0, 40.0, 0.5)
W, H, D = 128, 80, 32
N = W * H


def main():
    L = A.lib()
    assert hasattr(L, "adc_test_fail_at"), "not the fault-injection build"
    L.adc_test_fail_at.argtypes = [C.c_long]
    L.adc_test_fail_at.restype = None
    L.adc_test_hip_calls.restype = C.c_long
    left, right = workloads.structured_pair(W, H, D, seed=31)
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, A.ADCensusOption(max_disparity=D, do_filling=0))
    d = np.zeros((H, W), np.float32)
    prov, conf, depth, disp8 = np.zeros((H, W), np.uint8), np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W), np.uint8)
    cloud = np.zeros(N, A.POINT_DTYPE)
    sizes = dict(left=3 * N, right=3 * N, disp=4 * N, prov=N, conf=4 * N, depth=4 * N, cloud=16 * N, count=16, disp8=N)
    p = {k: L.adc_device_malloc(v) for k, v in sizes.items()}
    assert L.adc_memcpy_h2d(p["left"], np.ascontiguousarray(left).ctypes.data, 3 * N) == 0
    assert L.adc_memcpy_h2d(p["right"], np.ascontiguousarray(right).ctypes.data, 3 * N) == 0
    dev = (p["left"], p["right"], p["disp"])
    req_ex = A.Products.from_arrays(provenance=prov, confidence=conf)
    req_out = A.Products.from_arrays(calib=CALIB, depth=depth, cloud=cloud, disp8=disp8)
    dreq_ex = A.Products.from_addresses(p["prov"], p["conf"])
    dreq_out = A.Products.from_addresses(calib=CALIB, depth=p["depth"], cloud=p["cloud"], cloud_capacity=N, cloud_count=p["count"], disp8=p["disp8"])
    forms = {
        "plain": (lambda: st.Match(left, right, d), lambda: st.MatchProducts(left, right, d, None)),
        "ex": (lambda: st.MatchEx(left, right, d, prov, conf), lambda: st.MatchProducts(left, right, d, req_ex)),
        "out": (lambda: st.MatchOut(left, right, d, CALIB, depth, cloud, disp8), lambda: st.MatchProducts(left, right, d, req_out)),
        "device_plain": (lambda: st.match_device(*dev) and st.wait(), lambda: st.match_device_products(*dev, None) and st.wait()),
        "device_ex": (lambda: st.match_device_ex(*dev, p["prov"], p["conf"]) and st.wait(), lambda: st.match_device_products(*dev, dreq_ex) and st.wait()),
        "device_out": (lambda: st.match_device_out(*dev, CALIB, p["depth"], p["cloud"], N, p["count"], p["disp8"]) and st.wait(),
                       lambda: st.match_device_products(*dev, dreq_out) and st.wait()),
    }
    for _ in range(2):  # warm: every first-use allocation has happened, the handle has seen the pair
        for older, twin in forms.values():
            assert older() and twin(), A.last_error()
    out = {}
    for name, (older, twin) in forms.items():
        counts = []
        for call in (older, twin, older):
            L.adc_test_fail_at(0)
            assert call(), A.last_error()
            counts.append(int(L.adc_test_hip_calls()))
        out[name] = counts
    st.Release()
    for b in p.values():
        L.adc_device_free(b)
    print("REQUEST_PROBE " + json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
