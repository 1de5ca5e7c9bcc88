"""GPU tier of the triangle mesh from a disparity map (adcensus_amd/csrc/k_mesh.hip): the kernels against tests/mesh_ref.py bit for
bit on every case of tests/mesh_cases.py -- vertices as uint32 words, vertex_index, triangles, the report and the device count words,
each combination of outputs, into poisoned buffers whose bytes behind the last record must stay poisoned; the capacity cases; the
host entry point, the default parameters, the report behind a refused call; one oracle case end to end; "off means untouched",
injected HIP failures, the CLI."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle
from tests import cases
from tests import mesh_cases as MC
from tests import mesh_ref as M
from tests import normals_ref as N
from tests.test_gpu_outputs import CONE_CALIB, POISON, DeviceBuffers, _handle
from tests.test_gpu_rectify import PARENT_CALLS
from tests.test_mesh_api import check_mesh_ply, read_pfm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TAIL = 64  # poisoned bytes behind every output buffer


def _words(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint32)


def _report(rep):
    return [getattr(rep, k) for k in M.REPORT_FIELDS] + list(rep.reserved_)


def _mesh(A, st, dev, dm, c, what, vertices=True, vindex=True, triangles=True, image=None, counts=True, vcap=None, tcap=None, params=True):
    """one adc_mesh_device + adc_wait into fresh poisoned buffers -> dict(vertices uint32 [n][4], vindex, triangles, report, counts);
    only min(count, capacity) records may have been written: everything behind them must still be poisoned"""
    Wl, Hl = c["lattice"]
    vcap = Wl * Hl if vcap is None else vcap
    tcap = 2 * (Wl - 1) * (Hl - 1) if tcap is None else tcap
    pv = dev.alloc(16 * vcap + TAIL, POISON) if vertices else None
    pi = dev.alloc(4 * vcap + TAIL, POISON) if vindex else None
    pt = dev.alloc(12 * tcap + TAIL, POISON) if triangles else None
    pc = dev.alloc(8 + TAIL, POISON) if counts else None
    p = A.MeshParams(c["max_diff"], c["step"]) if params else None
    assert st.mesh_device(dm, c["calib"], p, image, pv, vcap, pi, pt, tcap, pc) and st.wait(), what + ": " + A.last_error()
    rep = st.mesh_report()
    out = dict(report=_report(rep))
    nv, nt = min(rep.vertices, vcap), min(rep.triangles, tcap)
    for key, ptr, size, n, cap in (("vertices", pv, 16, nv, vcap), ("vindex", pi, 4, nv, vcap), ("triangles", pt, 12, nt, tcap), ("counts", pc, 4, 2, 2)):
        if ptr is None:
            continue
        raw = dev.get(ptr, size * cap + TAIL, np.uint8)
        assert (raw[size * n:size * cap + TAIL] == POISON).all(), "%s: written behind record %d of %s" % (what, n, key)
        out[key] = np.frombuffer(raw[:size * n].tobytes(), np.uint32 if key != "vindex" else np.int32).reshape(-1, size // 4) if n else np.zeros((0, size // 4), np.uint32)
    return out


def _check(what, got, want, vcap=None, tcap=None):
    v, vi, t, rep = want
    words = M.report_words(rep) + [0, 0, 0]
    assert got["report"] == words, (what, got["report"], words)
    if "counts" in got:
        assert got["counts"].ravel().tolist() == [rep["vertices"], rep["triangles"]], (what, got["counts"])
    nv = len(v) if vcap is None else min(len(v), vcap)
    nt = len(t) if tcap is None else min(len(t), tcap)
    if "vertices" in got:
        assert np.array_equal(got["vertices"].ravel(), _words(v[:nv])), (what, "vertices")
    if "vindex" in got:
        assert np.array_equal(got["vindex"].ravel(), vi[:nv]), (what, "vertex_index")
    if "triangles" in got:
        assert np.array_equal(got["triangles"].reshape(-1, 3), t[:nt]), (what, "triangles")  # (true vertex numbers whatever the vertex capacity)


# each output combination: (vertices, vertex_index, triangles, colours)
COMBINATIONS = [(True, True, True, True), (True, False, True, False), (True, True, False, True), (True, False, False, False), (False, False, True, False)]


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_kernel_equals_the_reference(hip, name):
    A = hip
    c = MC.case(name)
    W, H = c["size"]
    st, dev = _handle(A, W, H, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        dm, di = dev.new(c["map"]), dev.new(c["image"])
        for vertices, vindex, triangles, colours in COMBINATIONS:
            what = "%s vertices %d index %d triangles %d colours %d" % (name, vertices, vindex, triangles, colours)
            got = _mesh(A, st, dev, dm, c, what, vertices, vindex, triangles, di if colours else None, counts=vindex)
            assert ("vertices" in got, "vindex" in got, "triangles" in got) == (vertices, vindex, triangles)
            _check(what, got, MC.reference(name, colours))
    finally:
        dev.free()
        st.Release()


def test_capacities(hip):
    """0, 1, one below / at / one above a chunk boundary of the reference's counts, the exact count: the first min(count, capacity)
    records and nothing behind them; the report, the count words and the triangles' vertex numbers do not depend on a capacity."""
    A = hip
    c = MC.case(MC.CAPACITY_CASE)
    W, H = c["size"]
    vcaps, tcaps = MC.capacities()
    st, dev = _handle(A, W, H, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        dm, di = dev.new(c["map"]), dev.new(c["image"])
        want = MC.reference(MC.CAPACITY_CASE)
        for vcap, tcap in list(zip(vcaps, tcaps)) + [(vcaps[-1], 0), (0, tcaps[-1])]:
            what = "capacities %d %d" % (vcap, tcap)
            _check(what, _mesh(A, st, dev, dm, c, what, image=di, vcap=vcap, tcap=tcap), want, vcap, tcap)
        # the host entry point copies out min(count, capacity) records into the caller's arrays
        for vcap, tcap in ((vcaps[2], tcaps[4]), (0, 0), (vcaps[-1] + 5, tcaps[-1] + 5)):
            v = np.full(vcap + 4, POISON, np.uint8).repeat(16).view(A.POINT_DTYPE)
            vi = np.full(vcap + 4, -2, np.int32)
            t = np.full((tcap + 4, 3), 0xA5A5A5A5, np.uint32)
            rep = A.MeshReport()
            cal = A.Calib(*c["calib"])
            rc = A.lib().adc_mesh(st._h, c["map"].ctypes.data, c["image"].ctypes.data, C.byref(cal), C.byref(A.MeshParams(c["max_diff"], c["step"])), v.ctypes.data, vcap,
                                  vi.ctypes.data, t.ctypes.data, tcap, C.byref(rep))
            assert rc == 0, A.last_error()
            nv, nt = min(vcap, len(want[0])), min(tcap, len(want[2]))
            assert _report(rep) == M.report_words(want[3]) + [0, 0, 0]
            assert v[:nv].tobytes() == want[0][:nv].tobytes() and (v[nv:].view(np.uint8) == POISON).all()
            assert np.array_equal(vi[:nv], want[1][:nv]) and (vi[nv:] == -2).all()
            assert np.array_equal(t[:nt], want[2][:nt]) and (t[nt:] == 0xA5A5A5A5).all()
    finally:
        dev.free()
        st.Release()


def test_host_entry_point_defaults_and_the_report(hip):
    """adc_mesh (host pointers, scratch on first use); params NULL = max_diff 1.0, step 1 through both entry points; the report of
    the last completed call stays in place behind a refused one, and a refused call writes nothing."""
    A = hip
    name = "mixed_s1_calib"
    c = MC.case(name)
    assert (c["max_diff"], c["step"]) == (M.DEFAULTS["max_diff"], M.DEFAULTS["step"])
    W, H = c["size"]
    st, dev = _handle(A, W, H, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        with pytest.raises(RuntimeError, match="no mesh call"):
            st.mesh_report()
        for colours in (True, False):
            want = MC.reference(name, colours)
            v, vi, t, rep = st.mesh(c["map"], c["calib"], None, c["image"] if colours else None)
            assert v.tobytes() == want[0].tobytes() and np.array_equal(vi, want[1]) and np.array_equal(t, want[2]) and _report(rep) == M.report_words(want[3]) + [0, 0, 0]
        dm = dev.new(c["map"])
        _check("device defaults", _mesh(A, st, dev, dm, c, "device defaults", params=False), MC.reference(name, False))
        for other in ("mixed_s3", "mixed_s16_calib"):  # the same handle, other parameters, no calibration
            co = MC.case(other)
            want = MC.reference(other)
            v, vi, t, rep = st.mesh(co["map"], co["calib"], A.MeshParams(co["max_diff"], co["step"]), co["image"])
            assert v.tobytes() == want[0].tobytes() and np.array_equal(vi, want[1]) and np.array_equal(t, want[2]) and _report(rep) == M.report_words(want[3]) + [0, 0, 0]
        # refused calls: nothing is written, the last report stays
        n = W * H
        pv, pi, pt, pc = (dev.alloc(size + TAIL, POISON) for size in (16 * n, 4 * n, 24 * n, 8))
        before = bytes(st.mesh_report())
        base = dict(calib=c["calib"], params=None, d_bgr_left=None, d_vertices=pv, vertex_capacity=n, d_vertex_index=pi, d_triangles=pt, triangle_capacity=2 * n, d_counts=pc)
        for kw, why in ((dict(params=A.MeshParams(step=0)), "step"), (dict(params=A.MeshParams(step=17)), "step"), (dict(params=A.MeshParams(max_diff=-1.0)), "max_diff"),
                        (dict(params=A.MeshParams(max_diff=float("nan"))), "max_diff"), (dict(params=A.MeshParams(flags=1)), "unknown flag"),
                        (dict(calib=(0.0, 0.16, 1.0, 1.0, 0.0)), "focal_px"), (dict(calib=(100.0, float("nan"), 1.0, 1.0, 0.0)), "non-finite"),
                        (dict(d_vertices=pv + 4), "16-byte aligned"), (dict(d_triangles=pt + 2), "4-byte aligned"), (dict(d_counts=pc + 1), "4-byte aligned"),
                        (dict(d_vertices=None, d_vertex_index=None, d_triangles=None), "no output"), (dict(d_vertices=None), "vertex_index needs vertices")):
            args = dict(base, **kw)
            assert not st.mesh_device(dm, **args) and why in A.last_error(), (why, A.last_error())
            assert bytes(st.mesh_report()) == before
        assert st.wait()
        for p, size in ((pv, 16 * n), (pi, 4 * n), (pt, 24 * n), (pc, 8)):
            assert (dev.get(p, size + TAIL, np.uint8) == POISON).all()
        assert bytes(st.mesh_report()) == before
    finally:
        dev.free()
        st.Release()


def test_oracle_case_cone_and_a_pending_match(hip, oracle):
    """Cone: the mesh of the map a Match delivers equals the definition applied to that map; refused while a Match is pending (a redo
    in adc_wait would rewrite the map behind the kernels); an exact Match afterwards."""
    A = hip
    left, right, opt = cases.make_case("cone")
    h, w = left.shape[:2]
    n = w * h
    want_d = oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n)
        pv, pt = dev.alloc(16 * n, POISON), dev.alloc(24 * n, POISON)
        assert st.match_device(dl, dr, dd), A.last_error()
        assert not st.mesh_device(dd, CONE_CALIB, None, dl, pv, n, None, pt, 2 * n, None) and "Match is pending" in A.last_error()
        assert st.wait(), A.last_error()
        assert (dev.get(pv, 16 * n, np.uint8) == POISON).all() and (dev.get(pt, 24 * n, np.uint8) == POISON).all()
        assert np.array_equal(_words(dev.get(dd, (h, w), F)), _words(want_d))
        for calib, max_diff, step in ((CONE_CALIB, 1.0, 1), (None, 1.5, 2), (CONE_CALIB, float("inf"), 5)):
            c = dict(calib=calib, max_diff=max_diff, step=step, lattice=(M.lattice(w, step), M.lattice(h, step)))
            want = M.mesh(want_d, calib, max_diff, step, left)
            assert want[3]["triangles"] > 0.5 * c["lattice"][0] * c["lattice"][1] and (want[3]["cells_one"] > 0 or max_diff == float("inf")), want[3]
            _check("cone step %d" % step, _mesh(A, st, dev, dd, c, "cone step %d" % step, image=dl), want)
        assert np.array_equal(_words(st.match(left, right)), _words(want_d))
    finally:
        dev.free()
        st.Release()


def _probe(*args):
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_fault_probe.py"), *args], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])


def test_off_means_untouched(hip):
    """adc_create allocates nothing of the feature, and a plain adc_match and a plain adc_match_device + adc_wait make exactly the
    hooked HIP calls of the parent revision -- with the feature never called, and again after it has been called."""
    o = _probe("--counts-only")
    print(o)
    assert {k: o[k] for k in PARENT_CALLS} == PARENT_CALLS, o
    assert {k: o["after_" + k] for k in PARENT_CALLS if k != "create_calls"} == {k: v for k, v in PARENT_CALLS.items() if k != "create_calls"}, o
    # the hook sits on the new calls.  adc_mesh: 2 uploads, the cleared words, 3 kernels, the read-back, the wait, 3 copy-outs; its first
    # use adds 5 scratch buffers and the handle's block of words
    assert o["mesh_calls"] == 11 and o["mesh_first_calls"] == 17 and o["triangles"] > 0, o


def test_hip_failures_on_the_mesh_paths(hip):
    """The fault-injection build: every HIP call of adc_mesh (first use included) and of adc_mesh_device + adc_wait (first use
    included) fails once (an injected return code, never a device fault) -- the call reports it with code 2, nothing leaks, the same
    handle delivers the exact mesh and report and an exact Match afterwards."""
    o = _probe()
    print(o)
    assert o["mesh_calls"] == 11 and o["mesh_first_calls"] == 17 and o["device_calls"] == 6 and o["device_first_calls"] == 7, o
    assert o["triangles"] > 0
    for name in ("host", "device"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert o["host_live_after"] == [] and o["live_after_release"] == 0 and o["final_live"] == 0, o
    assert abs(o["host_leak_bytes"]) <= (2 << 20) and abs(o["final_leak_bytes"]) <= (2 << 20), o


def test_cli_mesh_on_cone(hip, oracle, tmp_path):
    """adcensus_cli ... --calib --mesh 1.5,2 on Cone: <out>-mesh.ply equals the reference on the oracle's map; with --normals the
    vertex normals are those of tests/normals_ref.py at vertex_index; the other files of a run without the flag do not change."""
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
    runs = (("plain", calib_arg), ("mesh", calib_arg + ["--mesh", "1.5,2"]), ("nrm", calib_arg + ["--normals", "3,1.5,7"]),
            ("meshn", ["--mesh", "1.5,2"] + calib_arg + ["--normals", "3,1.5,7"]), ("bare", []), ("meshbare", ["--mesh", "inf,4"]))
    stdout = {}
    for pref, extra in runs:
        out = subprocess.run([cli, str(tmp_path / "left.png"), str(tmp_path / "right.png"), "0", "64", str(tmp_path / pref)] + extra,
                             capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
        stdout[pref] = out.stdout
    for a, b, suffixes in (("plain", "mesh", ("-d.png", "-c.png", "-cloud.txt", ".pfm", "-depth.pfm", "-cloud.ply")),
                           ("nrm", "meshn", ("-d.png", "-c.png", "-cloud.txt", ".pfm", "-depth.pfm", "-cloud.ply", "-n.png")),
                           ("bare", "meshbare", ("-d.png", "-c.png", "-cloud.txt", ".pfm"))):
        for suffix in suffixes:
            assert open(str(tmp_path / a) + suffix, "rb").read() == open(str(tmp_path / b) + suffix, "rb").read(), (a, b, suffix)
        assert not os.path.exists(str(tmp_path / a) + "-mesh.ply")
    assert np.array_equal(_words(read_pfm(str(tmp_path / "mesh") + ".pfm")), _words(want_d))
    rep = check_mesh_ply(str(tmp_path / "mesh"), left, CONE_CALIB, 1.5, 2, None, stdout["mesh"])
    assert rep["triangles"] > 1000 and rep["cells_one"] > 0
    nrm = N.normals(want_d, CONE_CALIB, 3, 1.5, 7)[0]
    check_mesh_ply(str(tmp_path / "meshn"), left, CONE_CALIB, 1.5, 2, nrm, stdout["meshn"])
    check_mesh_ply(str(tmp_path / "meshbare"), left, None, float("inf"), 4, None, stdout["meshbare"])
