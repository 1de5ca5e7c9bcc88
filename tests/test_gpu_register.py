"""GPU tier of the registration of depth into a second camera (adcensus_amd/csrc/k_register.hip): the scatter / resolve / align kernels
against tests/register_ref.py bit for bit on every case of tests/register_cases.py, with and without splat and the pre-test load; the
aligned image as the colours of a cloud; one oracle case end to end; refusals, "off means untouched", injected HIP failures, the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases, outputs_ref
from tests import register_cases as RC
from tests import register_ref as R
from tests.test_gpu_outputs import CONE_CALIB, POISON, DeviceBuffers, _handle
from tests.test_gpu_rectify import PARENT_CALLS
from tests.test_register_api import _target_text, read_pfm

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


def _registered(A, st, dev, dm, c, flags, what, depth=True, index=True):
    """one adc_register_depth_device + adc_wait into fresh poisoned buffers -> (depth, index, report words)"""
    (Wt, Ht) = c["tsize"]
    nt = Wt * Ht
    pz = _out(dev, 4 * nt) if depth else None
    pi = _out(dev, 4 * nt) if index else None
    assert st.register_depth_device(dm, c["calib"], c["kind"], flags, pz, pi) and st.wait(), what + ": " + A.last_error()
    z = dev.get(pz, (Ht, Wt), F) if depth else None
    i = dev.get(pi, (Ht, Wt), np.int32) if index else None
    for p in (pz, pi):
        assert p is None or _tail_ok(dev, p, 4 * nt), what + ": written behind an output"
    rep = st.register_report()
    return z, i, [rep.src_valid, rep.src_projected, rep.dst_filled, rep.reserved_]


@pytest.mark.parametrize("name", RC.CASE_NAMES)
def test_kernels_equal_the_reference(hip, name):
    A = hip
    c = RC.case(name)
    for cname, splat in RC.COLLISION_CASES:  # what a case is named for, on the reference's own counts: otherwise the test shows nothing
        if cname == name:
            rep = RC.reference(name, splat)[2]
            assert rep["candidates"] > rep["dst_filled"] > 0, rep
    for cname, splat in RC.TIE_CASES:
        if cname == name:
            assert RC.reference(name, splat)[2]["tied"] > 0
    (W, H), n = c["size"], c["size"][0] * c["size"][1]
    st, dev = _handle(A, W, H, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        st.set_register_target(c["target"])
        dm, dt = dev.new(c["map"]), dev.new(c["tbgr"])
        for flags in (0, A.REG_NO_SPLAT, A.REG_PRETEST, A.REG_NO_SPLAT | A.REG_PRETEST):
            what = "%s flags %d" % (name, flags)
            want_z, want_i, want_rep = RC.reference(name, not (flags & A.REG_NO_SPLAT))
            z, i, rep = _registered(A, st, dev, dm, c, flags, what)
            assert rep == R.report_words(want_rep), (what, rep, want_rep)
            assert np.array_equal(_u32(z), _u32(want_z)), (what, int((_u32(z) != _u32(want_z)).sum()))
            assert np.array_equal(i, want_i), (what, int((i != want_i).sum()))
        # one output alone
        z, _, _ = _registered(A, st, dev, dm, c, 0, name + " depth only", index=False)
        _, i, _ = _registered(A, st, dev, dm, c, 0, name + " index only", depth=False)
        assert np.array_equal(_u32(z), _u32(RC.reference(name, True)[0])) and np.array_equal(i, RC.reference(name, True)[1])
        # the other direction
        want_img, want_valid = RC.reference_align(name)
        po, pv = _out(dev, 3 * n), _out(dev, n)
        assert st.align_color_device(dm, c["calib"], dt, po, pv, c["kind"]) and st.wait(), A.last_error()
        assert np.array_equal(dev.get(po, (H, W, 3), np.uint8), want_img) and np.array_equal(dev.get(pv, (H, W), np.uint8), want_valid), name
        assert _tail_ok(dev, po, 3 * n) and _tail_ok(dev, pv, n)
        po2 = _out(dev, 3 * n)
        assert st.align_color_device(dm, c["calib"], dt, po2, None, c["kind"]) and st.wait(), A.last_error()
        assert np.array_equal(dev.get(po2, (H, W, 3), np.uint8), want_img) and _tail_ok(dev, po2, 3 * n)
    finally:
        dev.free()
        st.Release()


def test_host_entry_points_and_target_changes(hip):
    """adc_register_depth / adc_align_color (host pointers, scratch on first use), a target that grows and shrinks between calls, and a
    cleared target."""
    A = hip
    W, H = RC.case("rot5_small")["size"]
    st = _handle(A, W, H, pyoracle.Option(max_disparity=16))
    try:
        for name in ("rot5_small", "rot5_2x", "tiny_plain_3x3", "rot5_small"):
            c = RC.case(name)
            st.set_register_target(c["target"])
            for flags in (0, A.REG_NO_SPLAT):
                want_z, want_i, want_rep = RC.reference(name, not flags)
                z, i, rep = st.register_depth(c["map"], c["calib"], c["kind"], flags)
                assert np.array_equal(_u32(z), _u32(want_z)) and np.array_equal(i, want_i), (name, flags)
                assert [rep.src_valid, rep.src_projected, rep.dst_filled] == R.report_words(want_rep)[:3]
            img, valid = st.align_color(c["map"], c["calib"], c["tbgr"], c["kind"])
            assert np.array_equal(img, RC.reference_align(name)[0]) and np.array_equal(valid, RC.reference_align(name)[1]), name
        st.clear_register_target()
        with pytest.raises(RuntimeError, match="no target set"):
            st.register_depth(c["map"], c["calib"], c["kind"])
        assert st.register_report().dst_filled == RC.reference("rot5_small", False)[2]["dst_filled"]  # (the last completed report stays)
    finally:
        st.Release()


def test_aligned_image_colours_the_cloud(hip):
    """align_color_device writes what reproject_device takes as the left image: the cloud of the map with the target camera's colours."""
    A = hip
    c = RC.case("rot5_small")
    (W, H), n = c["size"], c["size"][0] * c["size"][1]
    st, dev = _handle(A, W, H, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        st.set_register_target(c["target"])
        dm, dt, po = dev.new(c["map"]), dev.new(c["tbgr"]), dev.alloc(3 * n, POISON)
        pc, pn = dev.alloc(16 * (n + 1), POISON), dev.alloc(16, POISON)
        assert st.align_color_device(dm, c["calib"], dt, po, None, c["kind"]) and st.wait(), A.last_error()
        assert st.reproject_device(dm, po, c["calib"], d_cloud=pc, cloud_capacity=n, d_cloud_count=pn) and st.wait(), A.last_error()
        aligned, valid = RC.reference_align("rot5_small")
        want = outputs_ref.cloud(c["map"], aligned, c["calib"])
        count = int(dev.get(pn, 1, np.uint32)[0])
        got = dev.get(pc, n + 1, A.POINT_DTYPE)
        assert count == len(want) == st.cloud_count() and got[:count].tobytes() == want.tobytes()
        assert got[count:].tobytes() == bytes([POISON]) * (16 * (n + 1 - count))
        seen = np.stack([want["b"], want["g"], want["r"]], axis=1)
        assert (seen != 0).all(axis=1).sum() > 0.5 * count and (seen == 0).all(axis=1).sum() > 0  # (colours of the target, and points it does not see)
    finally:
        dev.free()
        st.Release()


def test_oracle_case_cone(hip, oracle):
    """Cone: the depth a Match delivers, registered into a camera beside the left one, equals the definition applied to that depth;
    the delivered disparity map through FROM_DISPARITY gives the same bits."""
    A = hip
    left, right, opt = cases.make_case("cone")
    h, w = left.shape[:2]
    want_d = oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    T = A.RegTarget(width=w, height=h, fx=CONE_CALIB[0], fy=CONE_CALIB[0], cx=CONE_CALIB[2], cy=CONE_CALIB[3], t=[-0.08, 0.0, 0.0])
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        got = st.match_products(left, right, calib=CONE_CALIB, depth=True)
        assert np.array_equal(_u32(got["disparity"]), _u32(want_d))
        want_z, want_i, want_rep = R.register(got["depth"], R.FROM_DEPTH, CONE_CALIB, T)
        assert want_rep["candidates"] > want_rep["dst_filled"] > 0.5 * w * h
        st.set_register_target(T)
        c_depth = dict(calib=CONE_CALIB, kind=R.FROM_DEPTH, tsize=(w, h))
        c_disp = dict(calib=CONE_CALIB, kind=R.FROM_DISPARITY, tsize=(w, h))
        z, i, rep = _registered(A, st, dev, dev.new(got["depth"]), c_depth, 0, "cone depth")
        assert rep == R.report_words(want_rep) and np.array_equal(_u32(z), _u32(want_z)) and np.array_equal(i, want_i)
        z2, i2, rep2 = _registered(A, st, dev, dev.new(got["disparity"]), c_disp, 0, "cone disparity")
        assert rep2 == rep and np.array_equal(_u32(z2), _u32(z)) and np.array_equal(i2, i)
    finally:
        dev.free()
        st.Release()


def test_refusals_on_a_real_handle(hip):
    A = hip
    w, h, d = 256, 160, 64
    left, right = workloads.structured_pair(w, h, d, seed=41)
    n = w * h
    calib = RC.calib_for(w, h)
    T = RC.target("shift", w, h, w, h)
    st, dev = _handle(A, w, h, pyoracle.Option(max_disparity=d)), DeviceBuffers(A)
    try:
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n)
        outs = [dev.alloc(s, POISON) for s in (4 * n, 4 * n, 3 * n, n)]
        pz, pi, po, pv = outs
        dt = dev.alloc(3 * n, 7)

        def untouched():
            return all((dev.get(p, s, np.uint8) == POISON).all() for p, s in zip(outs, (4 * n, 4 * n, 3 * n, n)))

        def refused(ok, why):
            assert not ok and why in A.last_error() and untouched(), (why, A.last_error())

        refused(st.register_depth_device(dd, calib, d_depth=pz, d_index=pi), "no target set")
        refused(st.align_color_device(dd, calib, dt, po, pv), "no target set")
        with pytest.raises(RuntimeError, match="no registration"):
            st.register_report()
        for bad, why in ((dict(width=0), "[1, 32767]"), (dict(height=32768), "[1, 32767]"), (dict(fx=0.0), "fx and fy"), (dict(k2=float("nan")), "non-finite"),
                         (dict(t=[0, float("inf"), 0]), "non-finite")):
            with pytest.raises(RuntimeError, match=why.replace("[", r"\[")):
                st.set_register_target(A.RegTarget(**dict(dict(width=w, height=h, fx=100.0, fy=100.0), **bad)))
            refused(st.register_depth_device(dd, calib, d_depth=pz), "no target set")  # (a refused set call changes nothing)
        st.set_register_target(T)
        assert st.match_device(dl, dr, dd), A.last_error()
        # REFUSED while the Match is pending: a redo in adc_wait would rewrite the map behind the registration
        refused(st.register_depth_device(dd, calib, d_depth=pz, d_index=pi), "Match is pending")
        refused(st.align_color_device(dd, calib, dt, po, pv), "Match is pending")
        with pytest.raises(RuntimeError, match="Match is pending"):
            st.set_register_target(T)
        with pytest.raises(RuntimeError, match="Match is pending"):
            st.clear_register_target()
        assert st.wait(), A.last_error()
        want_d = dev.get(dd, (h, w), F)
        refused(st.register_depth_device(None, calib, d_depth=pz), "null map")
        refused(st.register_depth_device(dd, None, d_depth=pz), "null calibration")
        refused(st.register_depth_device(dd, calib, 2, d_depth=pz), "unknown input kind")
        refused(st.register_depth_device(dd, calib, flags=4, d_depth=pz), "unknown flag")
        refused(st.register_depth_device(dd, calib), "no output requested")
        refused(st.register_depth_device(dd, (0.0, 0.16, 1.0, 1.0, 0.0), d_depth=pz), "focal_px")
        refused(st.register_depth_device(dd, (100.0, float("nan"), 1.0, 1.0, 0.0), d_depth=pz), "non-finite")
        refused(st.align_color_device(dd, calib, None, po, pv), "null target image")
        refused(st.align_color_device(dd, calib, dt, None, pv), "no output requested")
        refused(st.align_color_device(dd, (100.0, 0.16, float("inf"), 1.0, 0.0), dt, po, pv), "non-finite")
        with pytest.raises(RuntimeError, match="no registration"):
            st.register_report()
        # after the refusals: an exact registration, then an exact Match
        assert st.register_depth_device(dd, calib, d_depth=pz, d_index=pi) and st.wait(), A.last_error()
        want_z, want_i, want_rep = R.register(want_d, R.FROM_DISPARITY, calib, T)
        assert np.array_equal(_u32(dev.get(pz, (h, w), F)), _u32(want_z)) and np.array_equal(dev.get(pi, (h, w), np.int32), want_i)
        assert st.register_report().dst_filled == want_rep["dst_filled"] > 0
        assert np.array_equal(_u32(st.match(left, right)), _u32(want_d))
    finally:
        dev.free()
        st.Release()


def _probe(*args):
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "register_fault_probe.py"), *args], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])


def test_off_means_untouched(hip):
    """adc_create allocates nothing of the feature, and on a handle that has a target set but does not use it a plain adc_match and a
    plain adc_match_device + adc_wait make exactly the hooked HIP calls of the parent revision."""
    o = _probe("--counts-only")
    print(o)
    assert {k: o[k] for k in PARENT_CALLS} == PARENT_CALLS, o
    # the hook sits on the new calls.  The first set call of a handle: the drain, the CU count, report words, pinned block, z-buffer (5);
    # a larger target: the drain and the z-buffer; the same target again: the drain alone
    assert o["set_first_calls"] == 5 and o["set_grow_calls"] == 2 and o["set_calls"] == 1, o


def test_hip_failures_on_the_registration_paths(hip):
    """The fault-injection build: every HIP call of adc_set_register_target (first use included), of adc_register_depth and
    adc_align_color (first use included) and of the device forms + adc_wait fails once (an injected return code, never a device fault)
    -- the call reports it, nothing leaks, the same handle delivers the exact maps and report and an exact Match afterwards."""
    o = _probe()
    print(o)
    # adc_register_depth: 3 first-use allocations; upload, 2 memsets, 2 kernels, read-back, the wait, 2 copy-outs.  adc_align_color: 4
    # allocations; 2 uploads, kernel, the wait, 2 copy-outs.  The device forms together: 5 + 1 + the wait
    assert o["reg_first_calls"] == o["reg_calls"] + 3 and o["reg_calls"] == 9, o
    assert o["align_first_calls"] == o["align_calls"] + 4 and o["align_calls"] == 6 and o["device_calls"] == 7, o
    assert o["filled"] > 0
    for name in ("set", "reg", "align", "device"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert abs(o["set_leak_bytes"]) <= (2 << 20) and abs(o["reg_leak_bytes"]) <= (2 << 20) and abs(o["align_leak_bytes"]) <= (2 << 20), o
    assert abs(o["final_leak_bytes"]) <= (2 << 20), o


def test_cli_register_on_cone(hip, oracle, tmp_path):
    """adcensus_cli ... --calib --register on Cone: <out>-reg.pfm equals the definition applied to the oracle's map, <out>-aligned.png
    the aligned colour image; the files of a run without the flag do not change."""
    from PIL import Image
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    left, right, opt = cases.make_case("cone")
    h, w = left.shape[:2]
    want_d = oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    wt, ht = 300, 260
    T = A_target = hip.RegTarget(width=wt, height=ht, fx=2500.0, fy=2480.0, cx=150.5, cy=128.25, R=RC.rot(0.5, 2.0), t=[-0.08, 0.01, 0.0], k1=-0.2, k2=0.05,
                                 p1=0.001, p2=-0.0005, k3=0.002)
    colour = np.random.default_rng(13).integers(1, 256, (ht, wt, 3), dtype=np.uint8)  # R, G, B as the PNG holds them
    Image.fromarray(np.ascontiguousarray(left[:, :, ::-1])).save(tmp_path / "left.png")
    Image.fromarray(np.ascontiguousarray(right[:, :, ::-1])).save(tmp_path / "right.png")
    Image.fromarray(colour).save(tmp_path / "colour.png")
    (tmp_path / "target.txt").write_text(_target_text(A_target))
    env = dict(os.environ, ADC_VERBOSE="0")
    calib_arg = ["--calib", "3740,0.16,225,187.5,0"]
    for pref, extra in (("plain", calib_arg), ("reg", calib_arg + ["--register", "%s,%s" % (tmp_path / "target.txt", tmp_path / "colour.png")])):
        out = subprocess.run([cli, str(tmp_path / "left.png"), str(tmp_path / "right.png"), "0", "64", str(tmp_path / pref)] + extra,
                             capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
    for suffix in ("-d.png", "-c.png", "-cloud.txt", ".pfm", "-depth.pfm"):
        assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / "reg") + suffix, "rb").read(), suffix
    assert not os.path.exists(str(tmp_path / "plain") + "-reg.pfm")
    assert np.array_equal(_u32(read_pfm(str(tmp_path / "reg") + ".pfm")), _u32(want_d))
    want_z, _, want_rep = R.register(want_d, R.FROM_DISPARITY, CONE_CALIB, T)
    assert want_rep["dst_filled"] > 1000
    assert np.array_equal(_u32(read_pfm(str(tmp_path / "reg") + "-reg.pfm")), _u32(want_z))
    aligned, valid = R.align(want_d, R.FROM_DISPARITY, CONE_CALIB, T, colour[:, :, ::-1])
    assert valid.sum() > 1000 and np.array_equal(np.array(Image.open(str(tmp_path / "reg") + "-aligned.png").convert("RGB")), aligned[:, :, ::-1])
