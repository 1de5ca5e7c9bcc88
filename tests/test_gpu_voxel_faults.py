"""GPU tier, host-side failure injection on the voxel-grid path of the cloud: through libadcensus_hip_faultinj.so every HIP call of the
path returns an error once WITHOUT being made (nothing faults on the device).  tests/voxel_fault_probe.py runs in its own interpreter;
only the existing injection hook is used."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hip_failures_on_the_voxel_paths(hip):
    """Every HIP call of the setter's first use + adc_reproject_device + adc_wait on a fresh handle, and of adc_match_async_products +
    adc_wait, fails once: the call reports it, the same handle delivers the exact voxel cloud and report afterwards, nothing leaks.  The
    plain cloud makes the same number of hooked calls before a grid was ever set and after it was cleared."""
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "voxel_fault_probe.py")], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([line for line in r.stdout.splitlines() if line.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])
    print(o)
    # the hook sits on the new calls: three first-use allocations; the clear, four launches and two read-backs per voxel cloud, which
    # replace the plain cloud's three launches and one read-back
    assert o["setter_first_calls"] == 3 and o["setter_again_calls"] == 0, o
    assert o["voxel_calls"] == o["plain_calls"] + 3 and o["plain_calls_after_clear"] == o["plain_calls"], o
    assert o["fresh_calls"] >= o["setter_first_calls"] + o["voxel_calls"] and o["match_calls"] > o["voxel_calls"], o
    assert 0 < o["voxels"] < o["points"], o
    for name in ("fresh", "match"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert o["live_after_first"] == o["live_after_fresh"] == o["live_after_match"] == 0, o  # (every buffer of the feature went with its handle)
    assert abs(o["fresh_leak_bytes"]) <= (2 << 20) and abs(o["final_leak_bytes"]) <= (2 << 20), o
