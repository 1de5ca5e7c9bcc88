"""Injected HIP failures on the TSDF mesh paths (tests/tsdf_mesh_fault_probe.py on libadcensus_hip_faultinj.so): each HIP call of the
new entry points returns a failure code once -- a substituted return value on the host, no kernel is made to fault -- and the call
reports it with code 2, nothing leaks, the handle and the volume stay usable and the next calls are bit-exact."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The hooked HIP calls of the probe's scenarios.
# device, again (22): adc_tsdf_create 4 (voxel words, colour words, two memsets) + adc_tsdf_upload 3 (the wait, two copies) +
#   adc_tsdf_mesh_device for the vertices alone 6 (the cleared report, the fused measure, two scans, the vertex pass, the read-back) + wait 1 +
#   adc_tsdf_mesh_device for both lists 7 (the same and the triangle pass) + wait 1
# device, first use (25): the report words, the tile counts and the per-voxel first ranks are allocated
# host, first use (28): adc_tsdf_create 5 + adc_tsdf_upload 3 + adc_tsdf_mesh 20 -- both record scratches have to grow, so it counts first
#   (the tile counts, the cleared report, the measure, two scans, the read-back: 6, the wait: 1); then the two scratches 2, the device form 8
#   (the first ranks are allocated), the wait 1, two copies out 2
DEVICE_AGAIN, DEVICE_FIRST, HOST_FIRST = 22, 25, 28


def test_hip_failures_on_the_tsdf_mesh_paths(hip):
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tsdf_mesh_fault_probe.py")], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])
    print(o)
    assert (o["device_calls"], o["fresh_device_first_calls"], o["host_first_calls"]) == (DEVICE_AGAIN, DEVICE_FIRST, HOST_FIRST), o
    assert o["vertices"] > 1000 and o["triangles"] > 1000
    for name in ("host", "device", "fresh_device"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert o["codes"] == [2], o
    assert o["host_live_after"] == [] and o["fresh_device_live_after"] == [] and o["live_after_release"] == 0 and o["final_live"] == 0, o
    assert abs(o["final_leak_bytes"]) <= (2 << 20), o
