"""GPU tier of the surface normals from a disparity map (adcensus_amd/csrc/k_normals.hip): the kernel against tests/normals_ref.py bit
for bit on every case of tests/normals_cases.py -- each output alone and both together, into poisoned buffers with a poisoned tail --
which also pins that sqrtf, the divisions and the int64 -> float conversions of the device code round as the definition says; the
host entry point, the default parameters, the report behind a refused call; one oracle case end to end; "off means untouched",
injected HIP failures, the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle
from tests import cases
from tests import normals_cases as NC
from tests import normals_ref as N
from tests.test_gpu_outputs import CONE_CALIB, POISON, DeviceBuffers, _handle
from tests.test_gpu_rectify import PARENT_CALLS
from tests.test_normals_api import check_cli_files, read_pfm, read_ply

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TAIL = 64  # poisoned bytes behind every output buffer


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _out(dev, nbytes):
    return dev.alloc(nbytes + TAIL, POISON)


def _tail_ok(dev, p, nbytes):
    return dev.get(p, nbytes + TAIL, np.uint8)[nbytes:].tobytes() == bytes([POISON]) * TAIL


def _normals(A, st, dev, dm, calib, params, what, normals=True, normals8=True):
    """one adc_normals_device + adc_wait into fresh poisoned buffers -> (normals, normals8, report words)"""
    H, W = st.height, st.width
    n = W * H
    pn = _out(dev, 16 * n) if normals else None
    p8 = _out(dev, 4 * n) if normals8 else None
    assert st.normals_device(dm, calib, params, pn, p8) and st.wait(), what + ": " + A.last_error()
    got = dev.get(pn, (H, W, 4), F) if normals else None
    got8 = dev.get(p8, (H, W, 4), np.uint8) if normals8 else None
    assert pn is None or _tail_ok(dev, pn, 16 * n), what + ": written behind normals"
    assert p8 is None or _tail_ok(dev, p8, 4 * n), what + ": written behind normals8"
    rep = st.normals_report()
    return got, got8, [rep.usable, rep.fitted, rep.few_points, rep.degenerate]


def _check(what, got, got8, rep, want):
    out, out8, wrep = want
    assert rep == N.report_words(wrep), (what, rep, wrep)
    if got is not None:
        assert np.array_equal(_u32(got), _u32(out)), (what, int((_u32(got) != _u32(out)).any(axis=-1).sum()))
    if got8 is not None:
        assert np.array_equal(got8, out8), (what, int((got8 != out8).any(axis=-1).sum()))


@pytest.mark.parametrize("name", NC.CASE_NAMES)
def test_kernel_equals_the_reference(hip, name):
    A = hip
    c = NC.case(name)
    if name in NC.MIXED_ALL_CLASSES:  # what a case is named for, on the reference's own counts: otherwise the test shows nothing
        rep = NC.reference(name)[2]
        assert rep["fitted"] > 0 and rep["few_points"] > 0 and rep["degenerate"] > 0, rep
    W, H = c["size"]
    params = A.NormalsParams(c["radius"], c["max_diff"], c["min_points"])
    st, dev = _handle(A, W, H, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        dm = dev.new(c["map"])
        for normals, normals8 in ((True, True), (True, False), (False, True)):
            what = "%s normals %d normals8 %d" % (name, normals, normals8)
            got, got8, rep = _normals(A, st, dev, dm, c["calib"], params, what, normals, normals8)
            _check(what, got, got8, rep, NC.reference(name))
    finally:
        dev.free()
        st.Release()


def test_host_entry_point_defaults_and_the_report(hip):
    """adc_normals (host pointers, scratch on first use), each output alone; params NULL = r 2, max_diff 1.0, min_points 5 through
    both entry points; the report of the last completed call stays in place behind a refused one."""
    A = hip
    c = NC.case("mixed_default")
    assert (c["radius"], c["max_diff"], c["min_points"]) == (N.DEFAULTS["radius"], N.DEFAULTS["max_diff"], N.DEFAULTS["min_points"])
    W, H = c["size"]
    st, dev = _handle(A, W, H, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        with pytest.raises(RuntimeError, match="no normals call"):
            st.normals_report()
        want = NC.reference("mixed_default")
        for normals, normals8 in ((True, True), (True, False), (False, True)):
            got, got8, rep = st.normals(c["map"], c["calib"], None, normals, normals8)
            _check("host defaults", got, got8, [rep.usable, rep.fitted, rep.few_points, rep.degenerate], want)
        got, got8, rep = _normals(A, st, dev, dev.new(c["map"]), c["calib"], None, "device defaults")
        _check("device defaults", got, got8, rep, want)
        c7 = NC.case("mixed_r7_gmax")
        p7 = A.NormalsParams(c7["radius"], c7["max_diff"], c7["min_points"])
        got, got8, rep = st.normals(c7["map"], c7["calib"], p7)
        _check("host r7", got, got8, [rep.usable, rep.fitted, rep.few_points, rep.degenerate], NC.reference("mixed_r7_gmax"))
        # refused calls: nothing is written, the last report stays
        n = W * H
        dm, pn, p8 = dev.new(c["map"]), _out(dev, 16 * n), _out(dev, 4 * n)
        before = bytes(st.normals_report())
        for kw, why in ((dict(params=A.NormalsParams(radius=8)), "radius"), (dict(params=A.NormalsParams(max_diff=0.0)), "max_diff"),
                        (dict(params=A.NormalsParams(min_points=26)), "min_points"), (dict(params=A.NormalsParams(flags=1)), "unknown flag"),
                        (dict(calib=(0.0, 0.16, 1.0, 1.0, 0.0)), "focal_px"), (dict(calib=(100.0, float("nan"), 1.0, 1.0, 0.0)), "non-finite"),
                        (dict(d_normals=pn + 4), "16-byte aligned"), (dict(d_normals8=p8 + 2), "4-byte aligned"), (dict(d_normals=None, d_normals8=None), "no output")):
            args = dict(dict(calib=c["calib"], params=None, d_normals=pn, d_normals8=p8), **kw)
            assert not st.normals_device(dm, args["calib"], args["params"], args["d_normals"], args["d_normals8"]) and why in A.last_error(), (why, A.last_error())
            assert bytes(st.normals_report()) == before
        assert st.wait()
        assert (dev.get(pn, 16 * n + TAIL, np.uint8) == POISON).all() and (dev.get(p8, 4 * n + TAIL, np.uint8) == POISON).all()
        assert bytes(st.normals_report()) == before
    finally:
        dev.free()
        st.Release()


def test_oracle_case_cone_and_a_pending_match(hip, oracle):
    """Cone: the normals of the map a Match delivers equal the definition applied to that map; refused while a Match is pending (a
    redo in adc_wait would rewrite the map behind the kernel); an exact Match afterwards."""
    A = hip
    left, right, opt = cases.make_case("cone")
    h, w = left.shape[:2]
    n = w * h
    want_d = oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n)
        pn, p8 = _out(dev, 16 * n), _out(dev, 4 * n)
        assert st.match_device(dl, dr, dd), A.last_error()
        assert not st.normals_device(dd, CONE_CALIB, None, pn, p8) and "Match is pending" in A.last_error()
        assert st.wait(), A.last_error()
        assert (dev.get(pn, 16 * n, np.uint8) == POISON).all() and (dev.get(p8, 4 * n, np.uint8) == POISON).all()
        assert np.array_equal(_u32(dev.get(dd, (h, w), F)), _u32(want_d))
        for params, args in ((None, (2, 1.0, 5)), (A.NormalsParams(7, 2.0, 30), (7, 2.0, 30))):
            want = N.normals(want_d, CONE_CALIB, *args)
            assert want[2]["fitted"] > 0.5 * n and want[2]["few_points"] + want[2]["degenerate"] > 0, want[2]
            got, got8, rep = _normals(A, st, dev, dd, CONE_CALIB, params, "cone r%d" % args[0])
            _check("cone r%d" % args[0], got, got8, rep, want)
        assert np.array_equal(_u32(st.match(left, right)), _u32(want_d))
    finally:
        dev.free()
        st.Release()


def _probe(*args):
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "normals_fault_probe.py"), *args], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])


def test_off_means_untouched(hip):
    """adc_create allocates nothing of the feature, and a plain adc_match and a plain adc_match_device + adc_wait make exactly the
    hooked HIP calls of the parent revision -- with the feature never called, and again after it has been called."""
    o = _probe("--counts-only")
    print(o)
    assert {k: o[k] for k in PARENT_CALLS} == PARENT_CALLS, o
    assert {k: o["after_" + k] for k in PARENT_CALLS if k != "create_calls"} == {k: v for k, v in PARENT_CALLS.items() if k != "create_calls"}, o
    # the hook sits on the new calls.  adc_normals: upload, the cleared words, the kernel, the read-back, the wait, 2 copy-outs; its first
    # use adds 3 scratch buffers and the report words
    assert o["normals_calls"] == 7 and o["normals_first_calls"] == 11 and o["fitted"] > 0, o


def test_hip_failures_on_the_normals_paths(hip):
    """The fault-injection build: every HIP call of adc_normals (first use included) and of adc_normals_device + adc_wait (first use
    included) fails once (an injected return code, never a device fault) -- the call reports it with code 2, nothing leaks, the same
    handle delivers the exact maps and report and an exact Match afterwards."""
    o = _probe()
    print(o)
    assert o["normals_calls"] == 7 and o["normals_first_calls"] == 11 and o["device_calls"] == 4 and o["device_first_calls"] == 5, o
    assert o["fitted"] > 0
    for name in ("host", "device"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert o["host_live_after"] == [] and o["live_after_release"] == 0 and o["final_live"] == 0, o
    assert abs(o["host_leak_bytes"]) <= (2 << 20) and abs(o["final_leak_bytes"]) <= (2 << 20), o


def test_cli_normals_on_cone(hip, oracle, tmp_path):
    """adcensus_cli ... --calib --normals on Cone: <out>-n.png holds the reference's bytes for the oracle's map, the ply the normals of
    its points; the other files of a run without the flag do not change; with --voxel the ply stays as it is."""
    from PIL import Image
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    left, right, opt = cases.make_case("cone")
    want_d = oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    Image.fromarray(np.ascontiguousarray(left[:, :, ::-1])).save(tmp_path / "left.png")
    Image.fromarray(np.ascontiguousarray(right[:, :, ::-1])).save(tmp_path / "right.png")
    env = dict(os.environ, ADC_VERBOSE="0")
    calib_arg = ["--calib", "3740,0.16,225,187.5,0"]
    runs = (("plain", calib_arg), ("nrm", calib_arg + ["--normals", "3,1.5,7"]), ("vox", calib_arg + ["--voxel", "0.01"]),
            ("voxn", calib_arg + ["--voxel", "0.01", "--normals", "3,1.5,7"]))
    for pref, extra in runs:
        out = subprocess.run([cli, str(tmp_path / "left.png"), str(tmp_path / "right.png"), "0", "64", str(tmp_path / pref)] + extra,
                             capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
    for suffix in ("-d.png", "-c.png", "-cloud.txt", ".pfm", "-depth.pfm"):
        assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / "nrm") + suffix, "rb").read(), suffix
    assert not os.path.exists(str(tmp_path / "plain") + "-n.png") and not read_ply(str(tmp_path / "plain") + "-cloud.ply")[0]
    assert np.array_equal(_u32(read_pfm(str(tmp_path / "nrm") + ".pfm")), _u32(want_d))
    rep = check_cli_files(str(tmp_path / "nrm"), str(tmp_path / "plain"), CONE_CALIB, 3, 1.5, 7)
    assert rep["fitted"] > 1000
    assert open(str(tmp_path / "vox") + "-cloud.ply", "rb").read() == open(str(tmp_path / "voxn") + "-cloud.ply", "rb").read()
    assert open(str(tmp_path / "nrm") + "-n.png", "rb").read() == open(str(tmp_path / "voxn") + "-n.png", "rb").read()
