"""Runs inside a subprocess of tests/test_gpu_mem_owner.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the
background).  The fault-injection build counts the allocations made through the owner of a handle's memory (adcensus_amd/csrc/dev_mem.h)
that are not yet freed: adc_test_live_buffers().  One handle uses every buffer that is allocated on first use, and the regrowing ones
twice; after Release the count must be back at 0 -- whatever the size of the buffer, which a comparison of hipMemGetInfo cannot say.
Then every hooked HIP call of adc_set_paper_modes (its allocations) fails once on a fresh handle: code 2 with a message, a retry works, a
Match afterwards is the undisturbed one, nothing stays behind.  The failures are injected return codes; no kernel is made to fault.
Ownership does not depend on the shape: the smallest valid pair, 64x48 with 16 disparities.  Prints one JSON object; the test asserts
on it."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import adcensus_amd as A  # noqa: E402
from adcensus_amd import workloads  # noqa: E402
from tests import register_cases as RC  # noqa: E402


def main():
    t0 = time.time()
    L = A.lib()
    assert hasattr(L, "adc_test_live_buffers"), "not the fault-injection build"
    L.adc_test_fail_at.argtypes = [C.c_long]
    L.adc_test_fail_at.restype = None
    L.adc_test_hip_calls.restype = C.c_long
    L.adc_test_live_buffers.restype = C.c_long
    live = lambda: int(L.adc_test_live_buffers())  # noqa: E731
    W, H, D = 64, 48, 16
    left, right = workloads.structured_pair(W, H, D, seed=31)
    opt = A.ADCensusOption(max_disparity=D)
    calib = A.Calib(*RC.calib_for(W, H))
    modes = A.PAPER_RIGHT_ARMS | A.PAPER_SO_SUM
    out = {"live_at_start": live()}

    def fresh():
        s = A.ADCensusStereo(device=0)
        L.adc_test_fail_at(0)
        assert s.Initialize(W, H, opt), A.last_error()
        return s

    # ---- Initialize alone: the same buffers on every handle
    counts = []
    for _ in range(2):
        st = fresh()
        counts.append(live())
        st.Release()
        counts.append(live())
    out["create_live"], out["after_first_release"], out["create_live_again"], out["after_second_release"] = counts

    # ---- one handle, every first-use owner once, the growing ones twice
    st = fresh()
    steps = [live()]
    st.set_speckle_filter(20, 1.0)
    want_filtered = st.match(left, right)
    steps.append(live())  # + sp_parent, sp_map
    d, prov, conf = st.match_ex(left, right)  # (adc_match_ex: the scratch of two maps, no staging)
    steps.append(live())
    ident = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    gray = A.RawFormat(W, H, W, A.PIX_GRAY8)
    st.set_rectify_maps(A.SIDE_LEFT, gray, ident[0], ident[1])
    st.set_rectify_maps(A.SIDE_RIGHT, gray, ident[0], ident[1])
    steps.append(live())  # + 2 x (records, two maps, valid map, raw image), the raw staging
    st.set_input_format(A.SIDE_LEFT, A.RawFormat(W, H, W * 4 + 8, A.PIX_BGRA8))  # more bytes per frame: raw image and staging regrow
    steps.append(live())
    st.clear_rectify()
    rng = np.random.default_rng(77)
    gl = rng.integers(1, 4 * D, (H, W)).astype(np.uint8)
    st.set_ground_truth(gl, np.roll(gl, -3, axis=1), scale=4.0)
    steps.append(live())  # + two ground-truth maps, occlusion map, report words, their pinned copy, the raw array
    st.evaluate(d, prov, conf, (1.0,), err=True, cls=True)
    steps.append(live())  # + the scratch of five maps
    st.set_register_target(RC.target("shift", W, H, 40, 30))
    steps.append(live())  # + report words, their pinned copy, the z-buffer
    st.set_register_target(RC.target("shift", W, H, 80, 56))  # the z-buffer regrows
    steps.append(live())
    st.register_depth(d, calib, depth=True, index=True)
    steps.append(live())  # + map, depth, index
    st.align_color(d, calib, rng.integers(1, 256, (56, 80, 3), dtype=np.uint8), valid=True)
    steps.append(live())  # + image, valid map, target image
    for cap in (10, W * H):  # the cloud scratch regrows
        p = st.match_products(left, right, calib=calib, provenance=True, confidence=True, depth=True, cloud=True, disp8=True, disp16_scale=256.0,
                              cloud_capacity=cap)
        assert np.array_equal(p["disparity"].view(np.uint32), want_filtered.view(np.uint32))
        steps.append(live())  # first: + output words, the scratch of three more maps, the staging of five, the cloud
    st.set_speckle_filter(0, 0.0)
    st.set_paper_modes(modes)
    want_paper = st.match(left, right)
    steps.append(live())  # + right-image arms, packed pixels, arm maxima, the third volume
    st.Release()
    out["steps"], out["after_release"] = steps, live()

    # ---- adc_set_paper_modes on fresh handles: every hooked call fails once
    st = fresh()
    L.adc_test_fail_at(0)
    st.set_paper_modes(modes)
    calls = int(L.adc_test_hip_calls())
    L.adc_test_fail_at(0)
    st.set_paper_modes(modes)
    out["paper_calls"], out["paper_again_calls"] = calls, int(L.adc_test_hip_calls())
    st.Release()
    bad, leaks = [], []
    for k in range(1, calls + 1):
        s = fresh()
        before = live()
        L.adc_test_fail_at(k)
        rc = L.adc_set_paper_modes(s._h, modes)
        L.adc_test_fail_at(0)
        if rc != 2 or not A.last_error().startswith("adc_set_paper_modes: "):
            bad.append(k)
        if k <= 3 and live() != before:  # (the three right-image buffers: all or none)
            bad.append(-k)
        if L.adc_set_paper_modes(s._h, modes) != 0 or live() != before + 4:
            bad.append(100 + k)
        if not np.array_equal(s.match(left, right).view(np.uint32), want_paper.view(np.uint32)):
            bad.append(1000 + k)
        s.Release()
        if live() != 0:
            leaks.append(k)
    out["paper_bad"], out["paper_leaks"], out["live_at_end"] = bad, leaks, live()
    out["seconds"] = round(time.time() - t0, 2)
    print("MEM_OWNER_PROBE " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
