"""GPU tier of the moving TSDF volume (adcensus_amd/csrc/k_tsdf_shift.hip): the kernels against tests/tsdf_shift_ref.py byte for byte on
every case of tests/tsdf_shift_cases.py -- both planes, the point list in a poisoned buffer whose bytes behind the list must stay
poisoned, d_count, the report, the offset and the origin --; two shifts against one; the round trip through integrate, extract, mesh and
ray cast on the shifted volume; the exactly-once property of the leaving lists over a session, which rests on adc_tsdf_extract alone; and
the HIP calls of the existing entry points, which a handle that never shifts must not see change."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle
from tests import tsdf_mesh_ref as MR
from tests import tsdf_raycast_ref as RR
from tests import tsdf_ref as T
from tests import tsdf_shift_cases as SC
from tests import tsdf_shift_ref as SR
from tests.test_gpu_outputs import POISON, DeviceBuffers, _handle
from tests.test_tsdf_api import c_frame, c_params
from tests.test_tsdf_raycast_api import c_view

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TAIL = 4  # poisoned records behind every point list
OPT = pyoracle.Option(max_disparity=16)
W, H = 64, 48


def _srep(rep):
    return [getattr(rep, k) for k in SR.SHIFT_FIELDS] + list(rep.reserved_)


def _same_volume(what, got, want):
    assert np.array_equal(got[0], want[0]), (what, "voxel words", int((got[0] != want[0]).sum()))
    assert (got[1] is None) == (want[1] is None), what
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "colour words", int((got[1] != want[1]).sum()))


def _origin(st):
    return tuple(st.tsdf_volume_device()[2].origin)


def _shift_device(A, st, dev, s, mw, cap, what, with_count=True):
    """adc_tsdf_shift_device into poisoned buffers -> (the records written, the count word, the report words)"""
    d_pts = dev.alloc((cap + TAIL) * 16, POISON)
    d_cnt = dev.alloc(16, POISON) if with_count else None
    assert st.tsdf_shift_device(A.TsdfShiftParams(s, mw), d_pts, cap, d_count=d_cnt), what + ": " + A.last_error()
    assert st.wait(), what + ": " + A.last_error()
    rep = st.tsdf_shift_report()
    n = min(rep.points, cap)
    raw = dev.get(d_pts, (cap + TAIL) * 16, np.uint8)
    assert (raw[16 * n:] == POISON).all(), what + ": written behind the list"
    cnt = None
    if with_count:
        words = dev.get(d_cnt, 4, np.uint32)
        assert (words[1:] == 0xA5A5A5A5).all(), what
        cnt = int(words[0])
    return raw[:16 * n].tobytes(), cnt, _srep(rep)


@pytest.mark.parametrize("colour", (False, True))
@pytest.mark.parametrize("vol", tuple(SC.VOLUMES))
def test_kernels_equal_the_reference(hip, vol, colour):
    A = hip
    p, old = SC.params(vol, colour), SC.volume(vol, colour)
    st, dev = _handle(A, W, H, OPT), DeviceBuffers(A)
    try:
        assert st.tsdf_shift_report() is None
        for s in SC.shifts(vol):
            for mw in SC.MIN_WEIGHTS:
                new, q, off, pts, rep = SC.reference(vol, colour, s, mw)
                for cap in (SC.capacities(rep["points"]) if mw == 1 else [rep["points"] + 5]):
                    what = "%s colour=%d shift=%s min_weight=%d capacity=%d" % (vol, colour, s, mw, cap)
                    assert st.tsdf_create(c_params(p)), A.last_error()  # (a new volume: the offset starts at 0, the second planes are gone)
                    st.tsdf_upload(*old)
                    assert st.tsdf_offset() == ((0, 0, 0), tuple(float(F(v)) for v in p["origin"])), what
                    before = st.tsdf_volume_device()[:2]
                    got, cnt, words = _shift_device(A, st, dev, s, mw, cap, what)
                    assert words == SR.report_words(rep) + [0] * 4, (what, words, rep)
                    assert cnt == rep["points"], (what, cnt)
                    assert got == pts[:cap].tobytes(), what
                    _same_volume(what, st.tsdf_download(), new)
                    assert st.tsdf_offset() == (off, tuple(float(F(v)) for v in p["origin"])), (what, st.tsdf_offset())
                    assert _origin(st) == tuple(float(F(v)) for v in q["origin"]), (what, _origin(st), q["origin"])
                    after = st.tsdf_volume_device()[:2]
                    assert (after == before) == (s == (0, 0, 0)) and (after[1] is None) == (not colour), (what, before, after)
            dev.free()
    finally:
        dev.free()
        st.Release()


def test_host_form_null_pointers_and_refusals_on_a_real_handle(hip):
    A = hip
    vol = "v12x7x9"
    p, old = SC.params(vol, True), SC.volume(vol, True)
    st, dev = _handle(A, W, H, OPT), DeviceBuffers(A)
    try:
        assert not st.tsdf_shift_device((1, 0, 0)) and "no volume" in A.last_error()
        with pytest.raises(RuntimeError):
            st.tsdf_offset()
        assert st.tsdf_create(c_params(p)), A.last_error()
        for s, mw in (((3, -2, 1), 1), ((-4, 0, 0), 3), ((0, 0, 0), 1), ((0, 9, 0), 1)):
            new, q, off, pts, rep = SC.reference(vol, True, s, mw)
            for cap in (None, 0, max(rep["points"] - 1, 0)):
                assert st.tsdf_create(c_params(p)), A.last_error()
                st.tsdf_upload(*old)
                got, hrep = st.tsdf_shift(s, mw, cap)
                assert got.tobytes() == (pts if cap is None else pts[:cap]).tobytes() and _srep(hrep) == SR.report_words(rep) + [0] * 4, (s, mw, cap)
                _same_volume((s, mw, cap), st.tsdf_download(), new)
                assert st.tsdf_offset()[0] == off and bytes(st.tsdf_shift_report()) == bytes(hrep)
            # no list, no count word: the volume moves all the same
            assert st.tsdf_create(c_params(p)), A.last_error()
            st.tsdf_upload(*old)
            assert st.tsdf_shift_device(s, None, 0, mw) and st.wait(), A.last_error()
            assert _srep(st.tsdf_shift_report()) == SR.report_words(rep) + [0] * 4
            _same_volume((s, mw, "no list"), st.tsdf_download(), new)
        # refusals change nothing
        assert st.tsdf_create(c_params(p)), A.last_error()
        st.tsdf_upload(*old)
        pp = dev.alloc(16 * 64, POISON)
        for call, why in ((lambda: st.tsdf_shift_device((1, 0, 0), pp + 8, 4), "16-byte aligned"), (lambda: st.tsdf_shift_device((1, 0, 0), pp, 4, d_count=pp + 2), "4-byte aligned"),
                          (lambda: st.tsdf_shift_device((1, 0, 0), None, 4), "null points"), (lambda: st.tsdf_shift_device((1, 0, 0), pp, 4, 0), "min_weight"),
                          (lambda: st.tsdf_shift_device((0, (1 << 24) + 1, 0), pp, 4), "2^24"), (lambda: st.tsdf_shift_device(A.TsdfShiftParams((1, 0, 0), 1, 4), pp, 4), "unknown flag")):
            assert not call() and why in A.last_error(), (why, A.last_error())
        assert (dev.get(pp, 16 * 64, np.uint8) == POISON).all() and st.tsdf_offset()[0] == (0, 0, 0)
        _same_volume("refused", st.tsdf_download(), old)
        # the offset is a sum, and adc_tsdf_reset keeps it
        assert st.tsdf_shift_device((0, 0, 1 << 24)) and st.tsdf_reset() and st.wait(), A.last_error()
        assert st.tsdf_offset()[0] == (0, 0, 1 << 24) and _origin(st)[2] == float(F(p["origin"][2]) + F(1 << 24) * F(p["voxel"]))
        assert not st.tsdf_shift_device((0, 0, 1)) and "2^24" in A.last_error()
        assert st.tsdf_shift_device((0, 0, -(1 << 25))) and st.wait() and st.tsdf_offset()[0] == (0, 0, -(1 << 24)), A.last_error()
        assert st.tsdf_destroy() and not st.tsdf_shift_device((1, 0, 0)) and "no volume" in A.last_error()
    finally:
        dev.free()
        st.Release()


def test_two_shifts_against_one(hip):
    """enqueued back to back with one wait: numpy applied twice; against the single shift by their sum the volume differs exactly where
    data left in between"""
    A = hip
    vol = "v12x7x9"
    p, old = SC.params(vol, True), SC.volume(vol, True)
    a, b = (3, 0, -2), (-3, 1, 2)
    v1, p1, o1, pts1, _ = SR.shift(old, p, SR.shift_params(a))
    v2, p2, o2, pts2, rep2 = SR.shift(v1, p1, SR.shift_params(b), o1, p["origin"])
    one, q, off, _, _ = SR.shift(old, p, SR.shift_params((0, 1, 0)))
    st, dev = _handle(A, W, H, OPT), DeviceBuffers(A)
    try:
        assert st.tsdf_create(c_params(p)), A.last_error()
        st.tsdf_upload(*old)
        d1, d2 = dev.alloc(16 * (len(pts1) + TAIL), POISON), dev.alloc(16 * (len(pts2) + TAIL), POISON)
        assert st.tsdf_shift_device(a, d1, len(pts1) + TAIL) and st.tsdf_shift_device(b, d2, len(pts2) + TAIL) and st.wait(), A.last_error()
        assert dev.get(d1, 16 * len(pts1), np.uint8).tobytes() == pts1.tobytes() and dev.get(d2, 16 * len(pts2), np.uint8).tobytes() == pts2.tobytes()
        assert _srep(st.tsdf_shift_report()) == SR.report_words(rep2) + [0] * 4  # (the report is that of the last)
        two = st.tsdf_download()
        _same_volume("two shifts", two, v2)
        assert st.tsdf_offset()[0] == o2 == off and _origin(st) == tuple(float(F(v)) for v in p2["origin"]) == tuple(float(F(v)) for v in q["origin"])
        assert st.tsdf_create(c_params(p)), A.last_error()
        st.tsdf_upload(*old)
        assert st.tsdf_shift_device((0, 1, 0)) and st.wait(), A.last_error()
        single = st.tsdf_download()
        _same_volume("one shift", single, one)
        lost = SR.move(SR.move(np.ones_like(old[0]), a), b) == 0
        assert np.array_equal(two[0] != single[0], lost & (single[0] != 0)) and (two[0] != single[0]).any()
    finally:
        dev.free()
        st.Release()


def _frame_scene():
    """a small depth frame that sees the 12 x 7 x 9 volume after the shift (3, -2, 1): a noisy wall through its middle"""
    rng = np.random.default_rng(3)
    depth = (2.2 + 0.05 * rng.standard_normal((H, W))).astype(F)
    depth[rng.random((H, W)) < 0.05] = 0.0
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return depth, image, T.frame((60.0, 0.16, 50.0, 24.0, 0.0), kind=T.FROM_DEPTH)


def test_round_trip_through_the_other_entry_points(hip):
    """integrate after a shift = the same integrate into a fresh volume created with the new origin and given the shifted words; extract,
    mesh and ray cast of the shifted volume = their numpy references on the shifted words and the new origin"""
    A = hip
    vol, s = "v12x7x9", (3, -2, 1)
    p, old = SC.params(vol, True), SC.volume(vol, True)
    new, q, off, _, _ = SC.reference(vol, True, s, 1)
    depth, image, fr = _frame_scene()
    want, irep = T.integrate(new, q, fr, depth, image)
    assert irep["updated"] > 100 and not np.array_equal(want[0], new[0])  # (the frame is worth integrating)
    view = RR.view(40, 30, 60.0, 32.0, 14.0, z_near=0.5, z_far=6.0, step=SC.VOXEL / 2, skip=SC.VOXEL * 2)
    st, fresh, dev = _handle(A, W, H, OPT), _handle(A, W, H, OPT), DeviceBuffers(A)
    try:
        d_map, d_img = dev.new(depth), dev.new(image)
        assert st.tsdf_create(c_params(p)), A.last_error()
        st.tsdf_upload(*old)
        assert st.tsdf_shift_device(s) and st.wait(), A.last_error()
        # the consumers of the shifted volume, before anything is fused into it
        for mw in SC.MIN_WEIGHTS:
            pts, xrep = st.tsdf_extract(A.TsdfExtractParams(mw))
            wpts, wrep = T.extract(new, q, mw)
            assert pts.tobytes() == wpts.tobytes() and (xrep.voxels_seen, xrep.points) == (wrep["voxels_seen"], wrep["points"]), mw
            vtx, tri, mrep = st.tsdf_mesh(A.TsdfExtractParams(mw))
            wv, wt, wm = MR.mesh(new, q, mw)
            assert vtx.tobytes() == wv.tobytes() and np.array_equal(tri, wt) and mrep.triangles == wm["triangles"], mw
        d, n, b, status, rrep = st.tsdf_raycast(c_view(view), bgr=True)
        wr = RR.raycast(new, q, view)
        assert d.tobytes() == wr["depth"].tobytes() and n.tobytes() == wr["normals"].tobytes() and b.tobytes() == wr["bgr"].tobytes() and status.tobytes() == wr["status"].tobytes()
        assert wr["report"]["no_surface"] > 20, wr["report"]  # (noise: few rays end on a surface; see below)
        # the integrate, against a fresh volume and against numpy
        assert st.tsdf_integrate_device(d_map, c_frame(fr), d_img) and st.wait(), A.last_error()
        assert fresh.tsdf_create(c_params(q)), A.last_error()
        fresh.tsdf_upload(*new)
        assert fresh.tsdf_integrate_device(d_map, c_frame(fr), d_img) and fresh.wait(), A.last_error()
        got, other = st.tsdf_download(), fresh.tsdf_download()
        _same_volume("fresh volume", got, other)
        _same_volume("numpy", got, want)
        assert bytes(st.tsdf_report()[0]) == bytes(fresh.tsdf_report()[0]) and st.tsdf_report()[0].updated == irep["updated"]
        # three more frames make a wall of it: the ray cast of a volume that moved and was fused into
        for _ in range(3):
            assert st.tsdf_integrate_device(d_map, c_frame(fr), d_img), A.last_error()
            want, _ = T.integrate(want, q, fr, depth, image)
        d, n, b, status, rrep = st.tsdf_raycast(c_view(view), bgr=True)
        wr = RR.raycast(want, q, view)
        assert d.tobytes() == wr["depth"].tobytes() and n.tobytes() == wr["normals"].tobytes() and b.tobytes() == wr["bgr"].tobytes() and status.tobytes() == wr["status"].tobytes()
        assert wr["report"]["hit"] > 20 and rrep.hit == wr["report"]["hit"], wr["report"]
        # upload / download act on the volume where it is now
        st.tsdf_upload(*old)
        _same_volume("upload after a shift", st.tsdf_download(), old)
        assert _origin(st) == tuple(float(F(v)) for v in q["origin"])
    finally:
        dev.free()
        st.Release()
        fresh.Release()


def _records(points):
    return sorted(np.ascontiguousarray(points).view("V16").ravel().tolist())


@pytest.mark.parametrize("colour", (False, True))
def test_every_crossing_is_handed_out_exactly_once(hip, colour):
    """This check does not rest on the rule's code: only adc_tsdf_extract on the untouched volume, the leaving lists and
    adc_tsdf_extract on what is left.  Dyadic geometry (voxel = 2^-5, origin0 a multiple of it below 2^10): every origin and every
    voxel centre is exact in binary32, so the records of the same crossing are bit-identical before and after a shift.  Six shifts,
    signs mixed across the axes, none reversing an earlier one on its axis: the concatenated leaving lists plus the final extraction
    are the records of the extraction of the untouched volume, as a multiset."""
    A = hip
    vol = "v12x7x9"
    p, old = SC.params(vol, colour), SC.volume(vol, colour)
    seq = [(1, 0, 0), (0, -2, 1), (2, -1, 0), (0, 0, 3), (3, -1, 1), (1, 0, 2)]  # x: + + + +, y: - - -, z: + + + +
    assert all(sum(abs(s[a]) for s in seq) < n for a, n in enumerate(SC.VOLUMES[vol]))  # (something is left for the final extraction)
    st = _handle(A, W, H, OPT)
    try:
        for mw in SC.MIN_WEIGHTS:
            assert st.tsdf_create(c_params(p)), A.last_error()
            st.tsdf_upload(*old)
            full, _ = st.tsdf_extract(A.TsdfExtractParams(mw))
            assert len(full) > 50
            handed = []
            for s in seq:
                pts, rep = st.tsdf_shift(s, mw)
                assert rep.points == len(pts) > 0, (s, mw)
                handed.append(pts)
            rest, _ = st.tsdf_extract(A.TsdfExtractParams(mw))
            assert len(rest) > 0 and st.tsdf_offset()[0] == tuple(sum(s[a] for s in seq) for a in range(3))
            got = _records(np.concatenate(handed + [rest]))
            assert len(got) == len(full) and got == _records(full), (mw, len(got), len(full))
    finally:
        st.Release()


# The hooked HIP calls of the existing entry points (a 12 x 7 x 9 volume with colour), read off capi.hip as it was before the shift
# existed: adc_tsdf_create 5 (two planes, the report words, two memsets), again 2 more frees nothing hooked: 4 (the report words exist);
# adc_tsdf_integrate_device 3 (the cleared report, the kernel, the read-back); adc_tsdf_extract_device 6 the first time (the tile
# counts; the cleared report, measure, scan, emit, the read-back), 5 after that.
CALLS_WITHOUT_A_SHIFT = dict(create=5, create_again=4, integrate=3, extract_first=6, extract=5)


def test_hip_calls_of_the_existing_entry_points_are_unchanged(hip):
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tsdf_shift_fault_probe.py"), "calls"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("CALLS_PROBE ")][-1][len("CALLS_PROBE "):])
    print(o)
    assert {k: o["plain"][k] for k in CALLS_WITHOUT_A_SHIFT} == CALLS_WITHOUT_A_SHIFT, o
    # a handle that has shifted: the same calls for everything that follows (the tile counts exist: the shift allocated them), and
    # the replacing adc_tsdf_create allocates what the first one did
    assert o["shifted"]["integrate"] == o["plain"]["integrate"] and o["shifted"]["extract"] == o["plain"]["extract"] and o["shifted"]["match"] == o["plain"]["match"], o
    assert o["shifted"]["create_again"] == o["plain"]["create_again"] and o["plain"]["match"] == o["plain"]["match_before_volume"] > 10, o
    # the shift itself: the report words, two second planes and the tile counts the first time (4), then the cleared report, measure,
    # scan, emit, the shift kernel and the read-back (6); all leaving adds two memsets; a zero shift clears, writes the count, reads back
    assert (o["shift_first"], o["shift"], o["shift_all"], o["shift_zero"]) == (10, 6, 8, 3), o
    assert o["live"] == 0, o
