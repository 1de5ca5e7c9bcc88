"""GPU tier of the TSDF volume (adcensus_amd/csrc/k_tsdf.hip): the kernels against tests/tsdf_ref.py bit for bit on every case of
tests/tsdf_cases.py -- the whole volume (voxel words and colour words) through adc_tsdf_download after every frame, the reports, the
surface points as uint32 words into poisoned buffers whose bytes behind the last record must stay poisoned, the device count word;
the capacity cases; sequences (saturation, several poses, reset, frames enqueued back to back, an uploaded volume); colour with and
without volume and image; the host entry points; refusals that leave everything as it was; the CLI on Cone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from tests import cases
from tests import tsdf_cases as TC
from tests import tsdf_ref as T
from tests.test_gpu_outputs import CONE_CALIB, POISON, DeviceBuffers, _handle
from tests.test_tsdf_api import c_frame, c_params, read_tsdf_ply

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TAIL = 64  # poisoned bytes behind every output buffer
CONE_VOLUME = (64, 48, 128, 0.04, (-1.28, -0.96, 11.0), 0.16)  # nx, ny, nz, voxel, origin, trunc: the near part of the Cone scene


def _words(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint32)


def _irep(rep):
    return [getattr(rep, k) for k in T.REPORT_FIELDS] + list(rep.reserved_)


def _xrep(rep):
    return [getattr(rep, k) for k in T.EXTRACT_FIELDS] + list(rep.reserved_)


def _open(A, c, params=None):
    """a handle of the case's image size with the case's volume (and its initial words)"""
    W, H = c["size"]
    st = _handle(A, W, H, pyoracle.Option(max_disparity=16))
    assert st.tsdf_create(c_params(params or c["params"])), A.last_error()
    if c["init"] is not None:
        st.tsdf_upload(*c["init"])
    return st


def _same_volume(what, got, want):
    assert np.array_equal(got[0], want[0]), (what, "voxel words", int((got[0] != want[0]).sum()))
    assert (got[1] is None) == (want[1] is None), what
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "colour words", int((got[1] != want[1]).sum()))


def _integrate(A, st, dev, fr, m, img, what):
    assert st.tsdf_integrate_device(dev.new(m), c_frame(fr), None if img is None else dev.new(img)) and st.wait(), what + ": " + A.last_error()
    return _irep(st.tsdf_report()[0])


def _extract(A, st, dev, what, min_weight=1, cap=0, points=True, count=True, params=True):
    """one adc_tsdf_extract_device + adc_wait into fresh poisoned buffers -> (records uint32 [n][4], report words); only min(points,
    capacity) records may have been written: everything behind them must still be poisoned"""
    pp = dev.alloc(16 * cap + TAIL, POISON) if points else None
    pc = dev.alloc(4 + TAIL, POISON) if count else None
    assert st.tsdf_extract_device(pp, cap if points else 0, A.TsdfExtractParams(min_weight) if params else None, pc) and st.wait(), what + ": " + A.last_error()
    rep = st.tsdf_report()[1]
    n = min(rep.points, cap) if points else 0
    recs = np.zeros((0, 4), np.uint32)
    if points:
        raw = dev.get(pp, 16 * cap + TAIL, np.uint8)
        assert (raw[16 * n:] == POISON).all(), "%s: written behind record %d" % (what, n)
        recs = np.frombuffer(raw[:16 * n].tobytes(), np.uint32).reshape(-1, 4)
    if count:
        raw = dev.get(pc, 4 + TAIL, np.uint8)
        assert (raw[4:] == POISON).all() and np.frombuffer(raw[:4].tobytes(), np.uint32)[0] == rep.points, what
    return recs, _xrep(rep)


def _check_extract(what, got, pts, xrep, cap):
    recs, rep = got
    assert rep == T.report_words(xrep, T.EXTRACT_FIELDS) + [0] * 6, (what, rep, xrep)
    n = min(len(pts), cap)
    assert len(recs) == n and np.array_equal(recs.ravel(), _words(pts[:n])), (what, "points")


@pytest.mark.parametrize("name", TC.INTEGRATE_CASES + ("uploaded_edges",))
def test_kernels_equal_the_reference(hip, name):
    A = hip
    c, r = TC.case(name), TC.reference(name)
    st, dev = _open(A, c), DeviceBuffers(A)
    try:
        for i, ((fr, m, img), want, rep) in enumerate(zip(c["frames"], r["volumes"], r["reports"])):
            what = "%s frame %d" % (name, i)
            assert _integrate(A, st, dev, fr, m, img, what) == T.report_words(rep) + [0, 0, 0, 0], what
            _same_volume(what, st.tsdf_download(), want)
        _same_volume(name, st.tsdf_download(), r["final"])
        cap = len(r["points"]) + 7
        _check_extract(name, _extract(A, st, dev, name, c["min_weight"], cap), r["points"], r["xreport"], cap)
        d_tsdf, d_col, p = st.tsdf_volume_device()
        assert d_tsdf and bool(d_col) == (r["final"][1] is not None) and bytes(p) == bytes(c_params(c["params"]))
        assert np.array_equal(dev.get(d_tsdf, r["final"][0].shape, np.uint32), r["final"][0])
    finally:
        dev.free()
        st.Release()


def test_extraction_of_a_volume_whose_scan_takes_two_turns(hip):
    """128 x 128 x 72 = 4608 tiles of 256 voxels: the one-workgroup scan runs its second turn.  An uploaded volume, extraction only."""
    A = hip
    c, r = TC.case("big_scan"), TC.reference("big_scan")
    assert c["params"]["nx"] * c["params"]["ny"] * c["params"]["nz"] // TC.TILE > TC.SCAN_TURN and r["xreport"]["points"] > 10000
    st, dev = _open(A, c), DeviceBuffers(A)
    try:
        cap = len(r["points"])
        _check_extract("big", _extract(A, st, dev, "big", c["min_weight"], cap), r["points"], r["xreport"], cap)
        _check_extract("big, min_weight 1", _extract(A, st, dev, "big 1", 1, 100), *T.extract(c["init"], c["params"], 1), 100)
    finally:
        dev.free()
        st.Release()


def test_capacities_min_weight_and_counting(hip):
    """0, 1, around a tile boundary of the record list, the exact count, above: the first min(points, capacity) records and nothing
    behind them; the report and the count word do not depend on the capacity.  A NULL pointer and a capacity of 0 count only.
    min_weight above some voxels' weights.  NULL params = min_weight 1."""
    A = hip
    c, r = TC.case(TC.CAPACITY_CASE), TC.reference(TC.CAPACITY_CASE)
    st, dev = _open(A, c), DeviceBuffers(A)
    try:
        st.tsdf_upload(*r["final"])
        pts, xrep = r["points"], r["xreport"]
        assert len(pts) > TC.TILE
        for cap in TC.capacities(len(pts)):
            _check_extract("capacity %d" % cap, _extract(A, st, dev, "capacity %d" % cap, 1, cap), pts, xrep, cap)
        _check_extract("count only", _extract(A, st, dev, "count only", 1, 0, points=False), pts, xrep, 0)
        _check_extract("defaults", _extract(A, st, dev, "defaults", 1, len(pts), count=False, params=False), pts, xrep, len(pts))
        for mw in (2, 3, 4):
            want = T.extract(r["final"], c["params"], mw)
            assert 0 < want[1]["voxels_seen"] < xrep["voxels_seen"] or mw == 4
            _check_extract("min_weight %d" % mw, _extract(A, st, dev, "min_weight %d" % mw, mw, len(pts)), *want, len(pts))
        # the host entry point: min(points, capacity) records into the caller's array, nothing behind them
        for cap in (0, 5, len(pts), len(pts) + 9):
            buf = np.full(cap + 4, POISON, np.uint8).repeat(16).view(A.POINT_DTYPE)
            rep = A.TsdfExtractReport()
            assert A.lib().adc_tsdf_extract(st._h, None, buf.ctypes.data, cap, C.byref(rep)) == 0, A.last_error()
            n = min(cap, len(pts))
            assert _xrep(rep) == T.report_words(xrep, T.EXTRACT_FIELDS) + [0] * 6
            assert buf[:n].tobytes() == pts[:n].tobytes() and (buf[n:].view(np.uint8) == POISON).all()
        got, rep = st.tsdf_extract()
        assert got.tobytes() == pts.tobytes() and rep.points == len(pts)
    finally:
        dev.free()
        st.Release()


def test_sequences_reset_enqueued_frames_and_the_host_entry_point(hip):
    """integrate, reset, integrate; the frames of a case enqueued back to back with ONE wait (the stream orders them; the report is
    the last frame's); adc_tsdf_integrate (host pointers) against the device form; a second adc_tsdf_create replaces the volume."""
    A = hip
    name = "tilted_holes_two_poses"
    c, r = TC.case(name), TC.reference(name)
    st, dev = _open(A, c), DeviceBuffers(A)
    try:
        assert st.tsdf_report() == (None, None)
        (fr0, m0, img0), (fr1, m1, img1) = c["frames"]
        _integrate(A, st, dev, fr1, m1, img1, "junk")
        assert st.tsdf_reset() and st.wait()
        empty = T.empty(c["params"])
        _same_volume("reset", st.tsdf_download(), empty)
        assert _integrate(A, st, dev, fr0, m0, img0, "after reset") == T.report_words(r["reports"][0]) + [0, 0, 0, 0]
        _same_volume("after reset", st.tsdf_download(), r["volumes"][0])
        # back to back
        assert st.tsdf_reset()
        for fr, m, img in c["frames"]:
            assert st.tsdf_integrate_device(dev.new(m), c_frame(fr), None if img is None else dev.new(img)), A.last_error()
        assert st.wait()
        _same_volume("enqueued", st.tsdf_download(), r["final"])
        assert _irep(st.tsdf_report()[0]) == T.report_words(r["reports"][1]) + [0, 0, 0, 0]
        # host pointers
        assert st.tsdf_reset()
        for (fr, m, img), rep in zip(c["frames"], r["reports"]):
            assert _irep(st.tsdf_integrate(m, c_frame(fr), img)) == T.report_words(rep) + [0, 0, 0, 0]
        _same_volume("host", st.tsdf_download(), r["final"])
        # a second create: another shape, empty
        c2, r2 = TC.case("long_row"), TC.reference("long_row")
        assert st.tsdf_create(c_params(c2["params"])), A.last_error()
        _same_volume("replaced", st.tsdf_download(), T.empty(c2["params"]))
        fr, m, img = c2["frames"][0]
        _integrate(A, st, dev, fr, m, img, "replaced")
        _same_volume("replaced", st.tsdf_download(), r2["final"])
        assert st.tsdf_destroy() and not st.tsdf_reset() and "no volume" in A.last_error() and st.tsdf_destroy()
    finally:
        dev.free()
        st.Release()


def test_colour_volume_and_image_combinations(hip):
    """Volume with colour and frames with and without an image (no image: the colour words keep their bits); a volume without colour
    takes frames without an image and REFUSES one with an image, writing nothing."""
    A = hip
    name = "plane5_saturates"
    c, r = TC.case(name), TC.reference(name)
    plain = dict(c["params"], flags=0)
    st, dev = _open(A, c, plain), DeviceBuffers(A)
    try:
        fr, m, img = c["frames"][0]
        assert not st.tsdf_integrate_device(dev.new(m), c_frame(fr), dev.new(img)) and "needs a colour volume" in A.last_error()
        with pytest.raises(RuntimeError, match="needs a colour volume"):
            st.tsdf_integrate(m, c_frame(fr), img)
        assert st.wait()
        _same_volume("refused", st.tsdf_download(), T.empty(plain))
        _integrate(A, st, dev, fr, m, None, "no colour")
        _same_volume("no colour", st.tsdf_download(), (r["volumes"][0][0], None))
        with pytest.raises(RuntimeError, match="colour pointer needs a colour volume"):
            st.tsdf_upload(r["volumes"][0][0], r["volumes"][0][1])
        # colour volume, image only in the second frame
        assert st.tsdf_create(c_params(c["params"]))
        _integrate(A, st, dev, fr, m, None, "colour volume, no image")
        _same_volume("colour volume, no image", st.tsdf_download(), (r["volumes"][0][0], T.empty(c["params"])[1]))
        fr, m, img = c["frames"][1]
        _integrate(A, st, dev, fr, m, img, "second frame with image")
        _same_volume("second frame with image", st.tsdf_download(), T.integrate((r["volumes"][0][0], T.empty(c["params"])[1]), c["params"], fr, m, img)[0])
    finally:
        dev.free()
        st.Release()


def test_refused_calls_leave_everything_and_a_pending_match(hip, oracle):
    """Refused calls write nothing and keep the reports; while a Match is pending every call that touches the volume is refused (a
    redo in adc_wait would rewrite the map behind the kernels); the Match is exact afterwards, and so is the volume."""
    A = hip
    left, right, opt = cases.make_case("cone")
    h, w = left.shape[:2]
    n = w * h
    want_d = oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    p = T.params(*CONE_VOLUME, flags=T.COLOR)
    fr = T.frame(CONE_CALIB)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n)
        assert not st.tsdf_integrate_device(dd, c_frame(fr)) and "no volume" in A.last_error()
        assert st.tsdf_create(c_params(p)), A.last_error()
        assert st.match_device(dl, dr, dd), A.last_error()
        pp = dev.alloc(16 * 64 + TAIL, POISON)
        for call in (lambda: st.tsdf_integrate_device(dd, c_frame(fr), dl), lambda: st.tsdf_extract_device(pp, 64), st.tsdf_reset, st.tsdf_destroy,
                     lambda: st.tsdf_create(c_params(p))):
            assert not call() and "Match is pending" in A.last_error(), A.last_error()
        assert st.wait(), A.last_error()
        assert np.array_equal(_words(dev.get(dd, (h, w), F)), _words(want_d))
        _same_volume("pending", st.tsdf_download(), T.empty(p))
        assert (dev.get(pp, 16 * 64 + TAIL, np.uint8) == POISON).all()
        # the Match's own map and image fused and extracted
        want, rep = T.integrate(T.empty(p), p, fr, want_d, left)
        assert rep["updated"] > 10000
        assert st.tsdf_integrate_device(dd, c_frame(fr), dl) and st.wait(), A.last_error()
        _same_volume("cone", st.tsdf_download(), want)
        pts, xrep = T.extract(want, p, 1)
        assert len(pts) > 1000
        _check_extract("cone", _extract(A, st, dev, "cone", 1, len(pts)), pts, xrep, len(pts))
        before = [bytes(x) for x in st.tsdf_report()]
        bad = c_frame(fr)
        bad.R[4] = float("nan")
        for call, why in ((lambda: st.tsdf_integrate_device(dd, bad), "non-finite"), (lambda: st.tsdf_integrate_device(dd + 2, c_frame(fr)), "4-byte aligned"),
                          (lambda: st.tsdf_extract_device(pp + 4, 8), "16-byte aligned"), (lambda: st.tsdf_extract_device(pp, 8, A.TsdfExtractParams(0)), "min_weight"),
                          (lambda: st.tsdf_create(A.TsdfParams(6, 8, 8, 0.1, (0, 0, 0), 0.2)), "multiple of 4")):
            assert not call() and why in A.last_error(), (why, A.last_error())
        assert st.wait() and [bytes(x) for x in st.tsdf_report()] == before
        _same_volume("after refusals", st.tsdf_download(), want)
        assert np.array_equal(_words(st.match(left, right)), _words(want_d))
        _same_volume("after a Match", st.tsdf_download(), want)
    finally:
        dev.free()
        st.Release()


def test_a_match_enqueued_behind_pending_tsdf_calls(hip, oracle):
    """adc_tsdf_integrate_device, adc_tsdf_extract_device, then adc_match_device of the next pair (Cone: LR check and filling, so the
    voting chain reads its state back into the pinned block) and ONE adc_wait: both reports, the count word, the points, the volume and
    the Match's map are exact -- the report words lie where no Match writes."""
    A = hip
    left, right, opt = cases.make_case("cone")
    assert opt.do_lr_check and opt.do_filling
    h, w = left.shape[:2]
    n = w * h
    want_d = oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    p = T.params(*CONE_VOLUME, flags=T.COLOR)
    fr = T.frame(CONE_CALIB)
    want, rep = T.integrate(T.empty(p), p, fr, want_d, left)
    pts, xrep = T.extract(want, p, 1)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        dl, dr, dm, dd = dev.new(left), dev.new(right), dev.new(want_d), dev.alloc(4 * n, POISON)
        cap = len(pts) + 3
        pp, pc = dev.alloc(16 * cap + TAIL, POISON), dev.alloc(4 + TAIL, POISON)
        assert st.tsdf_create(c_params(p)), A.last_error()
        for turn in range(2):  # (the second turn: into the volume that holds the frame, behind a handle that has matched)
            assert st.tsdf_integrate_device(dm, c_frame(fr), dl), A.last_error()
            assert st.tsdf_extract_device(pp, cap, None, pc), A.last_error()
            assert st.match_device(dl, dr, dd), A.last_error()
            assert st.wait(), A.last_error()
            irep, xr = st.tsdf_report()
            assert _irep(irep) == T.report_words(rep) + [0, 0, 0, 0], (turn, _irep(irep))
            assert _xrep(xr) == T.report_words(xrep, T.EXTRACT_FIELDS) + [0] * 6, (turn, _xrep(xr))
            raw = dev.get(pp, 16 * cap + TAIL, np.uint8)
            assert np.array_equal(np.frombuffer(raw[:16 * len(pts)].tobytes(), np.uint32), _words(pts)) and (raw[16 * len(pts):] == POISON).all(), turn
            assert dev.get(pc, 1, np.uint32)[0] == len(pts)
            assert np.array_equal(_words(dev.get(dd, (h, w), F)), _words(want_d)), turn
            _same_volume("turn %d" % turn, st.tsdf_download(), want)
            want, rep = T.integrate(want, p, fr, want_d, left)
            pts2, xrep2 = T.extract(want, p, 1)
            if turn == 0:
                assert len(pts2) <= cap
                pts, xrep = pts2, xrep2
                dev.put(pp, np.full(16 * cap + TAIL, POISON, np.uint8))
    finally:
        dev.free()
        st.Release()


def test_cli_tsdf_on_cone(hip, oracle, tmp_path):
    """adcensus_cli ... --calib --tsdf NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC on Cone: <out>-tsdf.ply holds the reference's points on the
    oracle's map, as many as the report it prints; with --pose the frame is the file's; the other files do not change."""
    from PIL import Image
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    left, right, opt = cases.make_case("cone")
    want_d = oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    Image.fromarray(np.ascontiguousarray(left[:, :, ::-1])).save(tmp_path / "left.png")
    Image.fromarray(np.ascontiguousarray(right[:, :, ::-1])).save(tmp_path / "right.png")
    R, t = TC.rot(2.0, -3.0, 1.0), (0.5, -0.25, 1.0)
    (tmp_path / "pose.txt").write_text(" ".join("%.9g" % v for v in R + t) + "\n")
    env = dict(os.environ, ADC_VERBOSE="0")
    calib_arg = ["--calib", "3740,0.16,225,187.5,0"]
    spec = "64,48,128,0.04,-1.28,-0.96,11,0.16"
    p = T.params(*CONE_VOLUME, flags=T.COLOR)
    stdout = {}
    for pref, extra in (("plain", calib_arg), ("tsdf", calib_arg + ["--tsdf", spec]), ("posed", ["--tsdf", spec + ",2", "--pose", str(tmp_path / "pose.txt")] + calib_arg)):
        out = subprocess.run([cli, str(tmp_path / "left.png"), str(tmp_path / "right.png"), "0", "64", str(tmp_path / pref)] + extra,
                             capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
        stdout[pref] = out.stdout
    for suffix in ("-d.png", "-c.png", "-cloud.txt", ".pfm", "-depth.pfm", "-cloud.ply"):
        for other in ("tsdf", "posed"):
            assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / other) + suffix, "rb").read(), (other, suffix)
    assert not os.path.exists(str(tmp_path / "plain") + "-tsdf.ply")
    for pref, fr, mw in (("tsdf", T.frame(CONE_CALIB), 1), ("posed", T.frame(CONE_CALIB, R, t), 2)):
        vol, rep = T.integrate(T.empty(p), p, fr, want_d, left)
        pts, xrep = T.extract(vol, p, mw)
        pts = pts.copy()
        pts["pad"] = 0  # (the file does not carry the weight)
        assert read_tsdf_ply(str(tmp_path / pref) + "-tsdf.ply").tobytes() == pts.tobytes() and (len(pts) > 1000 or mw == 2)
        assert "TSDF: %u voxels in the frustum, %u without depth, %u occluded, %u updated; %u voxels seen, %u surface points\n" % tuple(
            T.report_words(rep) + T.report_words(xrep, T.EXTRACT_FIELDS)) in stdout[pref], stdout[pref]
