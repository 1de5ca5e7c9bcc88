"""CPU tier: adcensus_amd/csrc/dev_mem.h -- the one owner of a handle's device and pinned memory -- driven by tests/emul/emul_mem.cpp with
malloc / free in place of the HIP calls, a "fail the n-th allocation" switch and a live count of its own.  The program is built with the
address and undefined-behaviour sanitizers and run directly: a leak, a double free, a block freed by the other kind's function or an
overrun of the registry fails the case."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "emul_mem.cpp")
HDR = os.path.join(ROOT, "adcensus_amd", "csrc", "dev_mem.h")


@pytest.fixture(scope="module")
def exe():
    out_dir = os.path.join(ROOT, "tests", "emul", "_build")
    path = os.path.join(out_dir, "emul_mem")
    if not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(out_dir, exist_ok=True)
        tmp = "%s.%d" % (path, os.getpid())  # (built aside and renamed: another process may be running the old one)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-g", SRC, "-o", tmp])
        os.replace(tmp, path)
    return path


def _case(exe, name):
    o = subprocess.run([exe, name], capture_output=True, text=True)
    assert o.returncode == 0, o.stdout[-2000:] + o.stderr[-4000:]
    facts = dict(re.findall(r"(\w+)=([\w,]+)", o.stdout.splitlines()[-1]))
    assert facts["violations"] == "0" and facts["live"] == "0", facts
    return facts


def test_header_is_plain_cpp():
    text = open(HDR).read()
    assert "#include <hip" not in text and "hipMalloc" not in text


def test_once_makes_no_call_when_the_field_is_set(exe):
    f = _case(exe, "once")
    assert (f["calls"], f["registered"]) == ("2", "2")  # (four requests: a preset field and a repeated one cost nothing)


def test_a_failure_leaves_null_and_zero_and_the_next_try_succeeds(exe):
    f = _case(exe, "fail_retry")
    assert (f["calls"], f["live_before_release"], f["registered"]) == ("8", "2", "3")


def test_grow_8_4_8_16_allocates_twice(exe):
    f = _case(exe, "grow_sequence")
    assert (f["allocs"], f["frees"], f["bytes"], f["cap"]) == ("2", "1", "64,0,0,128", "16")


def test_interleaved_kinds_are_freed_by_their_own_function(exe):
    f = _case(exe, "kinds")
    assert (f["device_allocs"], f["pinned_allocs"], f["device_frees"], f["pinned_frees"], f["wrong_frees"]) == ("4", "4", "4", "4", "0")


def test_release_all_after_failures_and_regrowth_and_again(exe):
    f = _case(exe, "release_all")
    assert (f["live_before"], f["live_after"], f["second_release_frees"], f["second_release_calls"], f["wrong_frees"]) == ("3", "0", "0", "0", "0")


def test_a_full_registry_is_refused(exe):
    f = _case(exe, "full")
    slots = int(f["slots"])
    assert slots >= 150  # (a handle registers about 110 fields)
    assert (int(f["accepted"]), f["refused_full"], int(f["registered"]), int(f["live_before_release"])) == (slots, "4", slots, slots)


def test_sweep_every_allocation_of_a_script_fails_once(exe):
    f = _case(exe, "sweep")
    n = int(f["script_allocations"])
    assert n == 14 and int(f["runs"]) == 2 * n and f["runs_with_live_buffers"] == "0"
