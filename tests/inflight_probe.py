"""Runs inside a subprocess of tests/test_gpu_inflight.py with ADC_HIP_LIB = libadcensus_hip_faultinj.so (tests/fault_probe.py has the
background).  What is in flight on a handle lives in one struct (AdcInFlight, adcensus_amd/csrc/adc_internal.h) whose idle state is
all bytes zero; the fault-injection build can say whether it is: adc_test_inflight() returns bit 0 when some byte of the struct is
nonzero and bit 1 when the handle's image pointers are borrowed.  The probe walks every way state gets in flight -- an asynchronous
Match, the device form, an armed median fallback, a voting chain that has to be continued, an evaluation, a registration -- and
checks that adc_wait leaves the handle idle and the results untouched; then every hooked HIP call of a Match that asks for every
product fails once (an injected return code; no kernel is made to fault), synchronously and through match_async + wait: the handle is
idle behind the failure and the next Match, of another pair, is the undisturbed one in every product.  Each step runs under an alarm
of its own.  Prints one JSON object; the test asserts on it."""
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import adcensus_amd as A  # noqa: E402
from adcensus_amd import workloads  # noqa: E402
from tests import register_cases as RC  # noqa: E402

W, H, D = 64, 48, 64
# The voting continuation needs a chain of more than four kernels.  Run once with the parent's library: at 64x48 the chain of the
# structured pair is longer than that (counter 1 rises), so the step runs at the probe's own size (tests/test_gpu_inflight.py).
VOTING_SHAPE = (64, 48)
STEP_SECONDS = 30


def request(w, h, calib):
    """(map, every product array, the adc_products) -- fresh arrays"""
    d = np.zeros((h, w), np.float32)
    arrays = dict(provenance=np.zeros((h, w), np.uint8), confidence=np.zeros((h, w), np.float32), depth=np.zeros((h, w), np.float32),
                  cloud=np.zeros(w * h, A.POINT_DTYPE), disp8=np.zeros((h, w), np.uint8), disp16=np.zeros((h, w), np.uint16))
    return d, arrays, A.Products.from_arrays(calib=calib, disp16_scale=256.0, **arrays)


def snapshot(d, arrays, req):
    n = int(req.count[0])
    return [d.tobytes()] + [arrays[k].tobytes() for k in ("provenance", "confidence", "depth", "disp8", "disp16")] + [n, arrays["cloud"][:n].tobytes()]


def main():
    t0 = time.time()
    L = A.lib()
    assert hasattr(L, "adc_test_inflight"), "not the fault-injection build"
    L.adc_test_fail_at.argtypes = [C.c_long]
    L.adc_test_fail_at.restype = None
    L.adc_test_hip_calls.restype = C.c_long
    L.adc_test_inflight.argtypes = [C.c_void_p]
    L.adc_test_inflight.restype = C.c_int
    fly = lambda s: int(L.adc_test_inflight(s._h))  # noqa: E731
    same = lambda a, b: bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))  # noqa: E731
    step = lambda: signal.alarm(STEP_SECONDS)  # noqa: E731  (a step that hangs ends the probe)
    left, right = workloads.structured_pair(W, H, D, seed=31)
    left2, right2 = workloads.noise_pair(W, H, seed=32)
    opt = A.ADCensusOption(max_disparity=D)
    calib = RC.calib_for(W, H)
    out = {}

    def fresh(w=W, h=H):
        s = A.ADCensusStereo(device=0)
        L.adc_test_fail_at(0)
        assert s.Initialize(w, h, opt), A.last_error()
        return s

    # ---- 1. a new handle is idle
    step()
    st = fresh()
    out["after_create"] = fly(st)
    want, want2 = st.match(left, right), st.match(left2, right2)
    out["after_match"] = fly(st)

    # ---- 2. asynchronous Match
    step()
    d = np.zeros((H, W), np.float32)
    assert st.match_async(left, right, d), A.last_error()
    out["async_enqueued"] = fly(st)
    assert st.wait(), A.last_error()
    out["async_waited"], out["async_map_ok"] = fly(st), same(d, want)
    out["wait_again_ok"], out["wait_again"] = bool(st.wait()), fly(st)

    # ---- 3. device form, on a handle of its own: the caller's images are borrowed until adc_wait
    step()
    sd = fresh()
    n = W * H
    bufs = [L.adc_device_malloc(s) for s in (3 * n, 3 * n, 4 * n, 4 * n, 4 * n)]
    dl, dr, dd, ddepth, dindex = bufs
    assert all(bufs)
    assert L.adc_memcpy_h2d(dl, np.ascontiguousarray(left).ctypes.data, 3 * n) == 0
    assert L.adc_memcpy_h2d(dr, np.ascontiguousarray(right).ctypes.data, 3 * n) == 0
    assert sd.match_device(dl, dr, dd), A.last_error()
    out["device_enqueued"] = fly(sd)
    assert sd.wait(), A.last_error()
    got = np.zeros((H, W), np.float32)
    assert L.adc_memcpy_d2h(got.ctypes.data, dd, 4 * n) == 0
    out["device_waited"], out["device_map_ok"] = fly(sd), same(got, want)

    # ---- 4. armed median fallback (as if a band had timed out / as if a speculative seam had differed)
    for arg in (100, 101):
        step()
        c0 = st.debug_counter(0)
        st.debug_run(A.RUN_MEDIAN, arg)
        armed = fly(st)
        m = st.match(left, right)
        out["median_%d" % arg] = {"armed": armed, "after": fly(st), "fallbacks": st.debug_counter(0) - c0, "map_ok": same(m, want)}

    # ---- 5. voting continuation: a budget of four kernels is too small for the chain
    step()
    vw, vh = VOTING_SHAPE
    sv = st if (vw, vh) == (W, H) else fresh(vw, vh)
    vl, vr = (left, right) if sv is st else workloads.structured_pair(vw, vh, D, seed=31)
    vwant = want if sv is st else sv.match(vl, vr)
    c1 = sv.debug_counter(1)
    sv.debug_set_budget(4)
    m = sv.match(vl, vr)
    out["voting"] = {"shape": [vw, vh], "after": fly(sv), "continuations": sv.debug_counter(1) - c1, "map_ok": same(m, vwant)}
    if sv is not st:
        sv.Release()

    # ---- 6. every hooked call of one Match with every product fails once: synchronous, then match_async + wait
    def products(s, l, r, sync):
        d, arrays, req = request(W, H, calib)
        if sync:
            ok = s.MatchProducts(l, r, d, req)
            mid = fly(s)
        else:
            ok = s.match_async_products(l, r, d, req)
            mid = 0 if ok else fly(s)  # (enqueued: in flight by design; refused: the failure surfaced here)
            ok = ok and s.wait()
        return bool(ok), mid, fly(s), snapshot(d, arrays, req)

    for sync in (True, False):
        step()
        name = "sync" if sync else "async"
        assert products(st, left, right, sync)[0], A.last_error()  # (first use: scratch and staging exist from here on)
        want_p2 = products(st, left2, right2, sync)
        assert want_p2[:3] == (True, 0, 0), A.last_error()
        L.adc_test_fail_at(0)
        assert products(st, left, right, sync)[0]
        calls = int(L.adc_test_hip_calls())
        not_failed, not_idle, wrong_after = [], [], []
        for k in range(1, calls + 1):
            step()
            L.adc_test_fail_at(k)
            ok, mid, after, _ = products(st, left, right, sync)
            L.adc_test_fail_at(0)
            if ok or not A.last_error():
                not_failed.append(k)
            if mid != 0 or after != 0:
                not_idle.append(k)
            if products(st, left2, right2, sync) != want_p2:
                wrong_after.append(k)
        out[name + "_calls"], out[name + "_not_failed"], out[name + "_not_idle"], out[name + "_wrong_after"] = calls, not_failed, not_idle, wrong_after
    out["plain_after_faults_ok"] = same(st.match(left, right), want) and same(st.match(left2, right2), want2)

    # ---- 7. evaluation and registration: in flight until adc_wait; idle behind a failing hooked call
    step()
    rng = np.random.default_rng(77)
    gl = rng.integers(1, 4 * D, (H, W)).astype(np.uint8)
    st.set_ground_truth(gl, np.roll(gl, -3, axis=1), scale=4.0)
    st.set_register_target(RC.target("shift", W, H, 40, 30))
    assert L.adc_memcpy_h2d(dd, want.ctypes.data, 4 * n) == 0
    entry = {"eval": lambda: st.evaluate_device(dd), "reg": lambda: st.register_depth_device(dd, calib, d_depth=ddepth, d_index=dindex)}
    for name, call in entry.items():
        step()
        L.adc_test_fail_at(0)
        assert call(), A.last_error()
        calls, enq = int(L.adc_test_hip_calls()), fly(st)
        assert st.wait(), A.last_error()
        o = {"calls": calls, "enqueued": enq, "waited": fly(st), "not_failed": [], "not_idle": []}
        for k in range(1, calls + 1):
            L.adc_test_fail_at(k)
            ok = call()
            L.adc_test_fail_at(0)
            if ok or not A.last_error():
                o["not_failed"].append(k)
            if fly(st) != 0:
                o["not_idle"].append(k)
        o["clean_after"] = bool(call() and st.wait()) and fly(st) == 0
        out[name] = o
    out["plain_at_end_ok"] = same(st.match(left, right), want)
    signal.alarm(0)
    st.Release()
    sd.Release()
    for b in bufs:
        L.adc_device_free(b)
    out["seconds"] = round(time.time() - t0, 2)
    print("INFLIGHT_PROBE " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
