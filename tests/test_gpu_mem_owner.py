"""The owner of a handle's device and pinned memory (adcensus_amd/csrc/dev_mem.h) on the GPU: tests/mem_owner_probe.py runs in its own
interpreter with the fault-injection build (tests/test_gpu_faults.py), whose adc_test_live_buffers() counts the owner's allocations not
yet freed.  A buffer of any size that adc_destroy forgot would show here; the hipMemGetInfo comparisons of the fault probes see only
what exceeds their 2 MiB margin."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAULT_LIB = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")

# Buffers each step of the probe's long-lived handle adds, read off capi.hip: speckle filter + Match (parent words, filtered map);
# adc_match_ex (scratch of two maps); rectify maps of both sides (2 x records, two maps, valid map, raw image; one raw staging);
# a larger raw format (regrowth: none); ground truth (two maps, occlusion, report words, pinned report, raw array); adc_evaluate (five
# maps); register target (report words, pinned report, z-buffer); a larger target (none); adc_register_depth (map, depth, index);
# adc_align_color (image, valid map, target image); products (output words, three more map scratches, five stagings, cloud); a larger
# cloud (none); paper modes (three right-image buffers, third volume)
STEP_BUFFERS = [2, 2, 11, 0, 6, 5, 3, 0, 3, 3, 10, 0, 4]


@pytest.mark.gpu
def test_every_buffer_of_a_handle_is_released(hip):
    if not os.path.exists(FAULT_LIB):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=FAULT_LIB, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mem_owner_probe.py")], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([l for l in r.stdout.splitlines() if l.startswith("MEM_OWNER_PROBE ")][-1][len("MEM_OWNER_PROBE "):])
    print(o)
    # Initialize alone: one allocation per buffer -- the 52 of alloc_all, and the ray table where the interpolation walks it -- and the
    # same on every handle
    assert o["live_at_start"] == 0 and o["create_live"] in (52, 53) and o["create_live_again"] == o["create_live"], o
    assert o["after_first_release"] == 0 and o["after_second_release"] == 0, o
    # every first-use owner: the buffers it adds, none for a regrowth, and nothing left behind Release
    steps = o["steps"]
    assert steps[0] == o["create_live"] and [b - a for a, b in zip(steps, steps[1:])] == STEP_BUFFERS, o
    assert o["after_release"] == 0, o
    # adc_set_paper_modes: its allocations are hooked, each fails once
    assert 1 <= o["paper_calls"] <= 4 and o["paper_again_calls"] == 0, o
    assert o["paper_bad"] == [] and o["paper_leaks"] == [] and o["live_at_end"] == 0, o
    assert o["seconds"] < 20, o  # (a few seconds: 64x48 images, a dozen handles)
