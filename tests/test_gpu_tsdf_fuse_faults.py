"""Injected HIP failures on the paths of the stereo-aware fusion (tests/tsdf_fuse_fault_probe.py on libadcensus_hip_faultinj.so): each
HIP call of the new entry points returns a failure code once -- a substituted return value on the host, no kernel is made to fault --
and the call reports it with code 2, nothing leaks, the handle stays usable and the next calls are bit-exact."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The hooked HIP calls of the probe's scenarios (a volume without colour).
# device, again (12): adc_tsdf_create 2 (voxel words, a memset) + adc_tsdf_weights_device 3 (the cleared report, the kernel, the
#   read-back) + the wait + adc_tsdf_fuse_device 3 (the same three) + the wait + adc_tsdf_download 2 (the wait, a copy)
# device, first use (14): the volume's report words and the report words of the weights are allocated
# host, first use (24): adc_tsdf_create 3 + adc_tsdf_weights 13 (four scratch buffers, three uploads, the device form's 4 with its report
#   words, the wait, the copy-out) + adc_tsdf_fuse 6 (two uploads, the device form's 3, the wait) + adc_tsdf_download 2
DEVICE_AGAIN, DEVICE_FIRST, HOST_FIRST = 12, 14, 24


def test_hip_failures_on_the_fusion_paths(hip):
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tsdf_fuse_fault_probe.py")], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])
    print(o)
    assert (o["device_calls"], o["fresh_device_first_calls"], o["host_first_calls"]) == (DEVICE_AGAIN, DEVICE_FIRST, HOST_FIRST), o
    assert o["updated"] > 1000 and o["interpolated"] > 1000 and o["nonzero"] > 1000
    for name in ("host", "device", "fresh_device"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert o["codes"] == [2], o
    assert o["host_live_after"] == [] and o["fresh_device_live_after"] == [] and o["live_after_release"] == 0 and o["final_live"] == 0, o
    assert abs(o["final_leak_bytes"]) <= (2 << 20), o
