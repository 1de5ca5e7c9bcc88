"""What is in flight on a handle (AdcInFlight, adcensus_amd/csrc/adc_internal.h) on the GPU: tests/inflight_probe.py runs in its own
interpreter with the fault-injection build (tests/test_gpu_faults.py), whose adc_test_inflight() says whether any byte of the struct is
nonzero (bit 0) and whether the image pointers are borrowed (bit 1).  Idle is all zero: behind adc_create, behind every adc_wait, and
behind every failure -- whichever hooked HIP call of a Match it was.

Shapes: 64x48 with 64 disparities throughout.  The voting continuation also runs there: with the parent's library a chain budget
of four kernels is too small for the structured pair at 64x48 (counter 1 rises by one), so the 160x48 geometry of
tests/test_emul_learn.py is not needed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAULT_LIB = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")


@pytest.mark.gpu
def test_a_handle_is_idle_behind_every_wait_and_every_failure(hip):
    if not os.path.exists(FAULT_LIB):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=FAULT_LIB, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "inflight_probe.py")], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([l for l in r.stdout.splitlines() if l.startswith("INFLIGHT_PROBE ")][-1][len("INFLIGHT_PROBE "):])
    print(o)
    # 1. a new handle, and one behind synchronous Matches
    assert o["after_create"] == 0 and o["after_match"] == 0, o
    # 2. asynchronous Match: in flight until adc_wait; a second adc_wait has nothing to settle
    assert o["async_enqueued"] & 1 and o["async_waited"] == 0 and o["async_map_ok"], o
    assert o["wait_again_ok"] and o["wait_again"] == 0, o
    # 3. device form: the request and the borrowed images
    assert o["device_enqueued"] == 3 and o["device_waited"] == 0 and o["device_map_ok"], o
    # 4. armed median fallback: consumed by the next Match's wait, exactly one fallback, the same map
    for arg in ("median_100", "median_101"):
        assert o[arg]["armed"] & 1 and o[arg]["after"] == 0 and o[arg]["fallbacks"] == 1 and o[arg]["map_ok"], o
    # 5. voting continuation
    assert o["voting"]["after"] == 0 and o["voting"]["continuations"] == 1 and o["voting"]["map_ok"], o
    # 6. every hooked call of a Match with every product failed once (below 10 calls the probe is not on the path)
    for name in ("sync", "async"):
        assert o[name + "_calls"] >= 10, o
        assert o[name + "_not_failed"] == [] and o[name + "_not_idle"] == [] and o[name + "_wrong_after"] == [], o
    assert o["plain_after_faults_ok"], o
    # 7. evaluation and registration
    for name in ("eval", "reg"):
        assert o[name]["calls"] >= 1 and o[name]["enqueued"] & 1 and o[name]["waited"] == 0, o
        assert o[name]["not_failed"] == [] and o[name]["not_idle"] == [] and o[name]["clean_after"], o
    assert o["plain_at_end_ok"], o
    assert o["seconds"] < 20, o  # (a few seconds: 64x48 images, some 150 Matches)
