"""Injected HIP failures on the TSDF paths (tests/tsdf_fault_probe.py on libadcensus_hip_faultinj.so): each HIP call of the new entry
points returns a failure code once -- a substituted return value on the host, no kernel is made to fault -- and the call reports it
with code 2, nothing leaks, the handle and the volume stay usable and the next calls are bit-exact.  And "off means untouched": the
HIP calls of adc_create and of a plain Match are the parent's, before and while a volume exists."""
import json
import os
import subprocess
import sys

import pytest

from tests.test_gpu_rectify import PARENT_CALLS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _probe(*args):
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tsdf_fault_probe.py"), *args], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])


# The hooked HIP calls of the two scenarios of the probe.
# host, first use (40): adc_tsdf_create 5 (voxel words, colour words, report words, two memsets) + adc_tsdf_integrate 8 (two scratch
#   buffers, two uploads, the cleared report, the kernel, the read-back, the wait) + adc_tsdf_integrate without an image 5 + adc_tsdf_extract
#   counting 6 (the tile counts, the cleared report, two kernels, the read-back, the wait) + adc_tsdf_extract with records 13 (its point
#   scratch has to grow, so it counts first: 5; then the point scratch, the cleared report, three kernels, the read-back, the wait, the
#   copy-out: 8) + adc_tsdf_download 3 (the wait, two copies) = 40
# host, again (nothing is allocated, the point scratch does not grow): 4 + 6 + 5 + 5 + 7 + 3 = 30
# device, again: adc_tsdf_create 4 + adc_tsdf_upload 3 + adc_tsdf_reset 2 + wait 1 + two integrates with their waits 8 + extract 5 + wait 1
#   + adc_tsdf_download 3 = 27; on a fresh handle the report words and the tile counts are allocated: 29
HOST_FIRST, HOST_AGAIN, DEVICE_AGAIN, DEVICE_FIRST = 40, 30, 27, 29


def test_off_means_untouched(hip):
    """adc_create allocates nothing of the feature, and a plain adc_match and a plain adc_match_device + adc_wait make exactly the
    hooked HIP calls of the parent revision -- with the feature never called, and again while a volume exists that frames were fused into."""
    o = _probe("--counts-only")
    print(o)
    assert {k: o[k] for k in PARENT_CALLS} == PARENT_CALLS, o
    assert {k: o["after_" + k] for k in PARENT_CALLS if k != "create_calls"} == {k: v for k, v in PARENT_CALLS.items() if k != "create_calls"}, o
    assert (o["host_first_calls"], o["host_calls"], o["device_calls"]) == (HOST_FIRST, HOST_AGAIN, DEVICE_AGAIN) and o["updated"] > 1000 and o["points"] > 100, o


def test_hip_failures_on_the_tsdf_paths(hip):
    o = _probe()
    print(o)
    assert (o["host_first_calls"], o["host_calls"], o["device_calls"], o["fresh_device_first_calls"]) == (HOST_FIRST, HOST_AGAIN, DEVICE_AGAIN, DEVICE_FIRST), o
    assert o["updated"] > 1000 and o["points"] > 100
    for name in ("host", "device", "fresh_device"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert o["host_live_after"] == [] and o["fresh_device_live_after"] == [] and o["live_after_release"] == 0 and o["final_live"] == 0, o
    assert abs(o["final_leak_bytes"]) <= (2 << 20), o
