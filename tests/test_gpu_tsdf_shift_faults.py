"""Injected HIP failures on the paths of the moving TSDF volume (tests/tsdf_shift_fault_probe.py on libadcensus_hip_faultinj.so): each
HIP call of the new entry points returns a failure code once -- a substituted return value on the host, no kernel is made to fault --
on a volume's first shift, which allocates the second planes, and on a later one.  The call reports it with code 2, nothing leaks, the
volume, its origin and its offset are what they were, and the same shift afterwards is exact byte for byte."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The hooked HIP calls of the probe's scenarios (a volume with colour, a list with a capacity, a count word).
# device, later (7): the cleared report, measure, scan, emit, the shift kernel, the read-back + the wait
# device, first (11): also the report words, the two second planes and the tile counts
# host, later (19): a counting pass 4 + its wait, the point scratch, a list pass 5 + its wait, the copy-out, the shift 5 + its wait
# host, first (23): also the report words and the tile counts (the counting pass), the two second planes (the shift)
DEVICE_LATER, DEVICE_FIRST, HOST_LATER, HOST_FIRST = 7, 11, 19, 23


def test_hip_failures_on_the_shift_paths(hip):
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tsdf_shift_fault_probe.py")], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])
    print(o)
    assert [o[k]["calls"] for k in ("device_later", "device_first", "host_later", "host_first")] == [DEVICE_LATER, DEVICE_FIRST, HOST_LATER, HOST_FIRST], o
    assert min(o["points"]) > 10, o
    for name in ("device_first", "device_later", "host_first", "host_later"):
        s = o[name]
        assert s["not_failed"] == [] and s["changed"] == [] and s["wrong_after"] == [] and s["live_after"] == [], (name, s)
        # only the device form can fail behind a shift that is already on the stream: in its adc_wait, the last call
        assert s["failed_in_wait"] == ([s["calls"]] if name.startswith("device") else []), (name, s)
    assert o["codes"] == [2], o
    assert o["final_live"] == 0 and abs(o["final_leak_bytes"]) <= (2 << 20), o
