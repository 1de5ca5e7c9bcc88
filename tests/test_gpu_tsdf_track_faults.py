"""Injected HIP failures on the tracking paths (tests/tsdf_track_fault_probe.py on libadcensus_hip_faultinj.so): each HIP call of the new
entry points returns a failure code once -- a substituted return value on the host, no kernel is made to fault -- and the call reports
it with code 2, nothing leaks, the handle stays usable and the next calls are bit-exact."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The hooked HIP calls of the probe's scenarios (3 iterations).
# device, again (10): the cleared state, 3 x (reduce, solve), the device copy of the record, the read-back, and the wait
# device, first use (13): the state and the pinned record are allocated and the device's CU count is asked for
# host, first use (22): adc_tsdf_create 3 (voxel words, a memset, the report words) + adc_tsdf_upload 2 (the wait, a copy) +
#   adc_tsdf_track 17 (the scratch, the upload, the ray cast 3, the track 3 + 8 without a device record, the wait)
DEVICE_AGAIN, DEVICE_FIRST, HOST_FIRST = 10, 13, 22


def test_hip_failures_on_the_tracking_paths(hip):
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tsdf_track_fault_probe.py")], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])
    print(o)
    assert (o["device_calls"], o["fresh_device_first_calls"], o["host_first_calls"]) == (DEVICE_AGAIN, DEVICE_FIRST, HOST_FIRST), o
    assert o["used"] > 1000 and o["solves"] == 3
    for name in ("host", "device", "fresh_device"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert o["codes"] == [2], o
    assert o["host_live_after"] == [] and o["fresh_device_live_after"] == [] and o["live_after_release"] == 0 and o["final_live"] == 0, o
    assert abs(o["final_leak_bytes"]) <= (2 << 20), o
