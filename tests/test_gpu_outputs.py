"""GPU tier: depth, point cloud and 8-bit image of adc_match_out / adc_match_device_out / adc_reproject_device against
tests/outputs_ref.py, bit for bit (uint32 view for floats, raw bytes for points, exact count) -- the kernels alone on the oracle's
final maps and on synthetic validity patterns, the whole calls, refusals, a cloud buffer that is too small, every redo adc_wait can
take, KITTI size and 1080p, the reference's result images, and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases, outputs_ref
from tests.test_outputs_api import read_pfm, read_ply

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["cone", "cone_nofill", "cone_nolr", "cone_neg", "cone_pos", "q_3x3_d2", "q_9x20_d8", "noise_160x90_d128", "s2_80x20_d2047"]
CONE_CALIB = (3740.0, 0.16, 225.0, 187.5, 0.0)
POISON = 0xA5


def _calibs(w, h):
    """no calibration, then doffs = 0, positive and negative"""
    return [None, (3740.0, 0.16, w / 2.0, h / 2.0, 0.0), (1234.5, 0.537, w / 3.0, h / 1.7, 2.75), (900.0, 0.1, 1.25, -3.5, -1.5)]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_u32(a), _u32(b))


def _final(oracle, left, right, opt):
    return oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]


def _handle(A, w, h, opt):
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt)), A.last_error()
    return st


class DeviceBuffers:
    """adc_device_malloc'ed buffers that are freed together"""

    def __init__(self, A):
        self.L = A.lib()
        self.bufs = []

    def alloc(self, nbytes, fill=None):
        p = self.L.adc_device_malloc(max(16, nbytes))
        assert p
        self.bufs.append(p)
        if fill is not None:
            self.put(p, np.full(max(16, nbytes), fill, np.uint8))
        return p

    def put(self, p, arr):
        arr = np.ascontiguousarray(arr)
        assert self.L.adc_memcpy_h2d(p, arr.ctypes.data, arr.nbytes) == 0
        return p

    def new(self, arr):
        arr = np.ascontiguousarray(arr)
        return self.put(self.alloc(arr.nbytes), arr)

    def get(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        assert self.L.adc_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.L.adc_device_free(p)
        self.bufs = []


def _check_outputs(what, disp, left, calib, depth, cloud, count, disp8):
    """the outputs a call delivered (None = not asked for) against the numpy definition of (disp, left, calib)"""
    want_z, want_pts, want_g = outputs_ref.outputs(disp, left, calib)
    if depth is not None:
        assert _same(depth, want_z), "%s: depth differs on %d pixels" % (what, int((_u32(depth) != _u32(want_z)).sum()))
    if disp8 is not None:
        assert np.array_equal(disp8, want_g), "%s: disp8 differs on %d pixels" % (what, int((disp8 != want_g).sum()))
    if cloud is not None:
        assert count == len(want_pts), "%s: count %d, expected %d" % (what, count, len(want_pts))
        assert len(cloud) == count and cloud.tobytes() == want_pts.tobytes(), "%s: the points differ" % what


def _reproject(A, st, dev, disp, left, calib, want=("depth", "cloud", "disp8"), capacity=None):
    """adc_reproject_device on a host map: returns (depth, cloud buffer [capacity + 1] as POINT_DTYPE, count, disp8, device count
    word); every output buffer is poisoned first"""
    h, w = disp.shape
    n = w * h
    cap = n if capacity is None else capacity
    dd, dl = dev.new(disp), dev.new(left)
    pz = dev.alloc(4 * n, POISON) if "depth" in want and calib is not None else None
    pc = dev.alloc(16 * (cap + 1), POISON) if "cloud" in want else None
    pn = dev.alloc(16, POISON) if "cloud" in want else None
    pg = dev.alloc(n, POISON) if "disp8" in want else None
    assert st.reproject_device(dd, dl, calib, pz, pc, cap, pn, pg), A.last_error()
    assert st.wait(), A.last_error()
    depth = dev.get(pz, (h, w), np.float32) if pz else None
    cloud = dev.get(pc, cap + 1, A.POINT_DTYPE) if pc else None
    word = int(dev.get(pn, 1, np.uint32)[0]) if pn else None
    disp8 = dev.get(pg, (h, w), np.uint8) if pg else None
    return depth, cloud, (st.cloud_count() if pc else None), disp8, word


def _check_reprojection(A, st, dev, what, disp, left, calib):
    depth, cloud, count, disp8, word = _reproject(A, st, dev, disp, left, calib)
    assert word == count, what
    assert cloud[count:].tobytes() == bytes([POISON]) * (16 * (len(cloud) - count)), what + ": written behind the last point"
    _check_outputs(what, disp, left, calib, depth, cloud[:count], count, disp8)
    dev.free()


@pytest.mark.parametrize("name", CASES)
def test_kernels_on_the_reference_maps(hip, oracle, name):
    """Stage-isolated: adc_reproject_device on the ORACLE's disp_final and the left image, without and with a calibration (doffs 0,
    positive, negative)."""
    A = hip
    left, right, opt = cases.make_case(name)
    h, w = left.shape[:2]
    disp = _final(oracle, left, right, opt)
    if name == "cone":  # the figures of the numpy definition on Cone's reference map
        z, valid = outputs_ref.depth(disp, (3740, 0.16, 0, 0, 0))
        print("cone: valid", int(valid.sum()), "max Z", float(z[valid].max()))
        assert int(valid.sum()) == 168746 and abs(float(z[valid].max()) - 276.66) < 0.01
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        for calib in _calibs(w, h):
            _check_reprojection(A, st, dev, "%s calib=%s" % (name, calib), disp, left, calib)
        # each output alone
        for one in ("depth", "cloud", "disp8"):
            depth, cloud, count, disp8, _ = _reproject(A, st, dev, disp, left, CONE_CALIB, want=(one,))
            _check_outputs("%s, %s alone" % (name, one), disp, left, CONE_CALIB, depth, None if cloud is None else cloud[:count], count, disp8)
            dev.free()
    finally:
        dev.free()
        st.Release()


def _synthetic_maps():
    rng = np.random.default_rng(77)
    inf = np.float32(np.inf)

    def values(shape):
        v = (rng.random(shape, dtype=np.float32) * np.float32(60)).astype(np.float32)
        v[rng.random(shape) < 0.1] *= np.float32(-1)
        v[rng.random(shape) < 0.02] = 0
        return v

    maps = {}
    for w, h in ((333, 41), (64, 16), (1030, 5), (7, 300)):
        v = values((h, w))
        edge = np.full((h, w), inf, np.float32)
        edge[-1, :] = v[-1, :]
        edge[:, -1] = v[:, -1]
        maps["edges_%dx%d" % (w, h)] = edge  # valid pixels only in the last column and the last row
        alt = v.copy()
        alt.reshape(-1)[0::2] = inf  # alternating validity per pixel (in raster order)
        maps["alternating_%dx%d" % (w, h)] = alt
        alt2 = v.copy()
        alt2.reshape(-1)[1::2] = inf
        maps["alternating_odd_%dx%d" % (w, h)] = alt2
    maps["all_invalid_100x30"] = np.full((30, 100), inf, np.float32)
    maps["first_pixel_only_100x30"] = np.full((30, 100), inf, np.float32)
    maps["first_pixel_only_100x30"][0, 0] = 5
    maps["all_valid_130x33"] = values((33, 130))
    maps["constant_negative_70x20"] = np.full((20, 70), -12.5, np.float32)
    maps["above_width_8x40"] = values((40, 8)) + np.float32(100)  # every |d| > W: mn stays float(W)
    runs = values((50, 257))
    runs.reshape(-1)[rng.random(runs.size) < 0.5] = inf  # random holes
    maps["random_holes_257x50"] = runs
    return maps


SYNTHETIC = _synthetic_maps()


@pytest.mark.parametrize("name", sorted(SYNTHETIC))
def test_kernels_on_synthetic_maps(hip, name):
    """Tile and wave boundaries of the ordered compaction: validity patterns at widths that are not multiples of 64."""
    A = hip
    disp = SYNTHETIC[name]
    h, w = disp.shape
    left = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    st, dev = _handle(A, w, h, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        for calib in _calibs(w, h):
            _check_reprojection(A, st, dev, "%s calib=%s" % (name, calib), disp, left, calib)
    finally:
        dev.free()
        st.Release()


@pytest.mark.parametrize("name", CASES)
def test_whole_calls_equal_reference(hip, oracle, name):
    """match_out and match_device_out: the disparity equals disp_final, the outputs equal outputs_ref(disp_final); each output alone
    equals its part; a plain Match on the same handle afterwards is undisturbed."""
    A = hip
    left, right, opt = cases.make_case(name)
    h, w = left.shape[:2]
    n = w * h
    want = _final(oracle, left, right, opt)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        for calib in (None, CONE_CALIB, (1234.5, 0.537, w / 3.0, h / 1.7, -1.5)):
            d, z, pts, g = st.match_out(left, right, calib, depth=calib is not None, cloud=True, disp8=True)
            assert _same(d, want), "%s: disparity differs" % name
            _check_outputs("%s match_out calib=%s" % (name, calib), want, left, calib, z, pts, st.cloud_count(), g)
        for one in ("depth", "cloud", "disp8"):
            d, z, pts, g = st.match_out(left, right, CONE_CALIB, depth=one == "depth", cloud=one == "cloud", disp8=one == "disp8")
            assert _same(d, want) and [x is not None for x in (z, pts, g)] == [one == "depth", one == "cloud", one == "disp8"]
            _check_outputs("%s match_out %s alone" % (name, one), want, left, CONE_CALIB, z, pts, None if pts is None else len(pts), g)
        assert _same(st.match(left, right), want), name + ": plain Match after MatchOut"
        d, z, pts, g = st.match_out(left, right)  # nothing asked for: exactly Match
        assert _same(d, want) and z is None and pts is None and g is None
        # the device entry point, twice into the same buffers, then one output alone, then a plain match_device
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n)
        pz, pc, pn, pg = dev.alloc(4 * n), dev.alloc(16 * n), dev.alloc(16), dev.alloc(n)
        for rep in range(2):
            assert st.match_device_out(dl, dr, dd, CONE_CALIB, pz, pc, n, pn, pg) and st.wait(), A.last_error()
            count = st.cloud_count()
            assert int(dev.get(pn, 1, np.uint32)[0]) == count
            assert _same(dev.get(dd, (h, w), np.float32), want)
            _check_outputs("%s match_device_out %d" % (name, rep), want, left, CONE_CALIB, dev.get(pz, (h, w), np.float32),
                           dev.get(pc, count, A.POINT_DTYPE), count, dev.get(pg, (h, w), np.uint8))
        dev.put(pc, np.full(16 * n, POISON, np.uint8))
        assert st.match_device_out(dl, dr, dd, None, None, pc, n, None, None) and st.wait(), A.last_error()
        count = st.cloud_count()
        _check_outputs("%s match_device_out cloud alone" % name, want, left, None, None, dev.get(pc, count, A.POINT_DTYPE), count, None)
        assert st.match_device(dl, dr, dd) and st.wait()
        assert _same(dev.get(dd, (h, w), np.float32), want)
    finally:
        dev.free()
        st.Release()


def test_refusals(hip, oracle):
    """depth without a calibration, focal_px <= 0 and a NaN field: 1 with a message, nothing enqueued, a plain Match afterwards exact."""
    A = hip
    L = A.lib()
    left, right, opt = cases.make_case("q_9x20_d8")
    h, w = left.shape[:2]
    n = w * h
    want = _final(oracle, left, right, opt)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        assert _same(st.match(left, right), want)
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n, POISON)
        pz, pc, pg = dev.alloc(4 * n, POISON), dev.alloc(16 * n, POISON), dev.alloc(n, POISON)
        d, z, pts, g = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32), np.zeros(n, A.POINT_DTYPE), np.zeros((h, w), np.uint8)
        bad = [(None, "calibration"), ((0.0, 0.16, 1, 1, 0), "focal_px"), ((-5.0, 0.16, 1, 1, 0), "focal_px"),
               ((float("nan"), 0.16, 1, 1, 0), "finite"), ((100.0, 0.16, float("nan"), 1, 0), "finite"),
               ((100.0, 0.16, 1, 1, float("inf")), "finite"), ((100.0, float("-inf"), 1, 1, 0), "finite")]
        for calib, word in bad:
            host = A._outputs(calib, z.ctypes.data, pts.ctypes.data, n, None, g.ctypes.data)
            devr = A._outputs(calib, pz, pc, n, None, pg)
            assert L.adc_match_out(st._h, left.ctypes.data, right.ctypes.data, d.ctypes.data, C.byref(host)) == 1, calib
            assert word in A.last_error(), (calib, A.last_error())
            assert L.adc_match_device_out(st._h, dl, dr, dd, C.byref(devr)) == 1 and word in A.last_error(), calib
            assert L.adc_reproject_device(st._h, dd, dl, C.byref(devr)) == 1 and word in A.last_error(), calib
            assert not st.MatchOut(left, right, d, calib, depth=z)
        assert st.wait()
        # nothing was enqueued: the host arrays and the poisoned device buffers are untouched
        assert not d.any() and not z.any() and not g.any() and not pts.view(np.uint8).any()
        for p, size in ((dd, 4 * n), (pz, 4 * n), (pc, 16 * n), (pg, n)):
            assert np.all(dev.get(p, size, np.uint8) == POISON)
        # a cloud without a calibration is no refusal, and an unaligned device cloud address is one
        assert st.match_device_out(dl, dr, dd, None, None, pc + 4, n - 1, None, None) is False and "aligned" in A.last_error()
        assert _same(st.match(left, right), want)
        assert st.match_device(dl, dr, dd) and st.wait() and _same(dev.get(dd, (h, w), np.float32), want)
    finally:
        dev.free()
        st.Release()


def test_capacity_smaller_than_count(hip, oracle):
    """A poisoned cloud buffer with capacity < count: the first capacity points are right, the rest is still poison, count is the
    full number (getter and device word) -- through reproject, match_device_out and match_out."""
    A = hip
    left, right, opt = cases.make_case("cone_nofill")
    h, w = left.shape[:2]
    n = w * h
    disp = _final(oracle, left, right, opt)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        for calib in (None, CONE_CALIB):
            want = outputs_ref.cloud(disp, left, calib)
            assert 1500 < len(want) < n
            for cap in (0, 1, 63, 1024, 1500, len(want) - 1, len(want), len(want) + 5):
                _, cloud, count, _, word = _reproject(A, st, dev, disp, left, calib, want=("cloud",), capacity=cap)
                k = min(cap, len(want))
                assert count == word == len(want), (cap, count, word)
                assert cloud[:k].tobytes() == want[:k].tobytes(), cap
                assert cloud[k:].tobytes() == bytes([POISON]) * (16 * (cap + 1 - k)), cap
                dev.free()
        cap = 1000
        want = outputs_ref.cloud(disp, left, None)
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n)
        pc, pn = dev.alloc(16 * (cap + 8), POISON), dev.alloc(16, POISON)
        assert st.match_device_out(dl, dr, dd, None, None, pc, cap, pn, None) and st.wait(), A.last_error()
        assert st.cloud_count() == len(want) and dev.get(pn, 4, np.uint32).tolist() == [len(want)] + [0xA5A5A5A5] * 3
        got = dev.get(pc, cap + 8, A.POINT_DTYPE)
        assert got[:cap].tobytes() == want[:cap].tobytes() and got[cap:].tobytes() == bytes([POISON]) * (16 * 8)
        d = np.empty((h, w), np.float32)
        pts = np.frombuffer(bytearray([POISON]) * (16 * (cap + 8)), A.POINT_DTYPE)
        assert st.MatchOut(left, right, d, None, cloud=pts[:cap]) and _same(d, disp)
        assert st.cloud_count() == len(want)
        assert pts[:cap].tobytes() == want[:cap].tobytes() and pts[cap:].tobytes() == bytes([POISON]) * (16 * 8)
    finally:
        dev.free()
        st.Release()


def _match_all(st, left, right, calib=CONE_CALIB):
    d, z, pts, g = st.match_out(left, right, calib, depth=True, cloud=True, disp8=True)
    return d, z, pts, st.cloud_count(), g


def _check_all(what, got, want_disp, left, calib=CONE_CALIB):
    d, z, pts, count, g = got
    assert _same(d, want_disp), what + ": disparity differs"
    _check_outputs(what, want_disp, left, calib, z, pts, count, g)


def test_redo_paths_keep_the_outputs_exact(hip, oracle, monkeypatch):
    """The sequence of tests/test_gpu_extras.py::test_redo_paths_keep_the_maps_exact with match_out: the aggregation ring redo
    (counter 2), the continued voting chain (budget of 4 kernels, counter 1), then the median fallback in both forms (counter 0)
    -- the counters show the path was taken, the outputs come from the delivered map."""
    A = hip
    w, h, d = 256, 160, 64
    opt = pyoracle.Option(max_disparity=d)
    s_pair = workloads.structured_pair(w, h, d, seed=41)
    n_pair = workloads.noise_pair(w, h, seed=42)
    want_s, want_n = _final(oracle, *s_pair, opt), _final(oracle, *n_pair, opt)
    monkeypatch.setenv("ADC_AGG_DUAL", "0")
    st = _handle(A, w, h, opt)
    try:
        _check_all("structured, first", _match_all(st, *s_pair), want_s, s_pair[0])
        _check_all("noise", _match_all(st, *n_pair), want_n, n_pair[0])
        _check_all("noise, small ring assumed", _match_all(st, *n_pair), want_n, n_pair[0])
        redo0 = st.debug_counter(2)
        _check_all("structured, aggregation redo", _match_all(st, *s_pair), want_s, s_pair[0])
        assert st.debug_counter(2) == redo0 + 1, "the aggregation redo path was not taken"
    finally:
        st.Release()
    st = _handle(A, w, h, opt)
    try:
        _check_all("structured, new handle", _match_all(st, *s_pair), want_s, s_pair[0])
        st.debug_set_budget(4)
        over = st.debug_counter(1)
        _check_all("structured, voting chain continued", _match_all(st, *s_pair), want_s, s_pair[0])
        assert st.debug_counter(1) == over + 1, "the voting continuation path was not taken"
    finally:
        st.Release()
    # the median fallback: 330 rows = the banded filter with speculative bands (tests/test_gpu_api.py::test_median_speculative_bands);
    # without filling, so that the map has holes and the compaction has work
    w, h, d = 240, 330, 32
    left, right = workloads.structured_pair(w, h, d, seed=11)
    opt = pyoracle.Option(max_disparity=d, do_filling=0)
    want = _final(oracle, left, right, opt)
    assert np.isinf(want).any()
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        _check_all("median, first", _match_all(st, left, right), want, left)
        for arg in (100, 101):
            fall = st.debug_counter(0)
            st.debug_run(A.RUN_MEDIAN, arg)
            _check_all("median fallback %d" % arg, _match_all(st, left, right), want, left)
            assert st.debug_counter(0) == fall + 1, "the median fallback path was not taken"
        # ... and through the device entry point
        n = w * h
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n)
        pz, pc, pn, pg = dev.alloc(4 * n, POISON), dev.alloc(16 * n, POISON), dev.alloc(16), dev.alloc(n, POISON)
        fall = st.debug_counter(0)
        st.debug_run(A.RUN_MEDIAN, 100)
        assert st.match_device_out(dl, dr, dd, CONE_CALIB, pz, pc, n, pn, pg) and st.wait(), A.last_error()
        assert st.debug_counter(0) == fall + 1
        count = st.cloud_count()
        assert int(dev.get(pn, 1, np.uint32)[0]) == count
        _check_all("median fallback, device", (dev.get(dd, (h, w), np.float32), dev.get(pz, (h, w), np.float32), dev.get(pc, count, A.POINT_DTYPE),
                                              count, dev.get(pg, (h, w), np.uint8)), want, left)
    finally:
        dev.free()
        st.Release()


@pytest.mark.parametrize("size", ["kitti_structured", "full_noise", "full_structured_nofill"])
def test_large_sizes(hip, oracle, size):
    """A KITTI-size structured pair (1242x375), the headline noise pair (1920x1080, seed 12345) and a 1080p structured pair without
    filling (holes), D = 128: match_out with all three outputs.  At 1080p the cloud is 33 MB."""
    A = hip
    kw = {}
    if size == "kitti_structured":
        w, h = 1242, 375
        left, right = workloads.structured_pair(w, h, 128, seed=4243)
    elif size == "full_noise":
        w, h = 1920, 1080
        left, right = workloads.noise_pair(w, h, 12345)
    else:
        w, h = 1920, 1080
        left, right = workloads.structured_pair(w, h, 128, seed=4244)
        kw = dict(do_filling=0)
    opt = pyoracle.Option(max_disparity=128, **kw)
    want = _final(oracle, left, right, opt)
    if kw:
        assert np.isinf(want).any()
    calib = (1050.0, 0.54, w / 2.0, h / 2.0, 0.0)
    st = _handle(A, w, h, opt)
    try:
        _check_all(size, _match_all(st, left, right, calib), want, left, calib)
        d, z, pts, g = st.match_out(left, right, None, cloud=True)
        assert _same(d, want)
        _check_outputs(size + ", uncalibrated cloud", want, left, None, None, pts, st.cloud_count(), None)
    finally:
        st.Release()


@pytest.mark.parametrize("case,ref,ident,within1", [("cone", "cone", 0.8355, 0.9938), ("cloth3", "cloth", 0.8994, 0.9849), ("piano", "piano", 0.6349, 0.8480)])
def test_disp8_against_the_reference_images(hip, oracle, case, ref, ident, within1):
    """disp8 of match_out equals the numpy formula exactly and is as close to the AUTHOR's result image as the reference compiled
    here is: the two thresholds per image of tests/test_gpu_api.py::test_cpp_facade_cli (the author's MSVC libm)."""
    from PIL import Image
    A = hip
    left, right, opt = cases.make_case(case)
    h, w = left.shape[:2]
    want = _final(oracle, left, right, opt)
    st = _handle(A, w, h, opt)
    try:
        d, _, _, g = st.match_out(left, right, disp8=True)
    finally:
        st.Release()
    assert _same(d, want)
    a = np.abs(want)
    mn, mx = np.float32(a.min()), np.float32(a.max())
    assert np.array_equal(g, ((a - mn) / (mx - mn) * np.float32(255)).astype(np.uint8))  # the formula test_cpp_facade_cli pins
    assert np.array_equal(g, outputs_ref.disp8(want))
    refd = np.array(Image.open(os.path.join(cases.GOLDEN_DIR, "ref_%s-d.png" % ref)))
    diff = np.abs(g.astype(int) - refd.astype(int))
    print(case, "identical", (diff == 0).mean(), "within one", (diff <= 1).mean())
    assert (diff == 0).mean() >= ident and (diff <= 1).mean() >= within1, ((diff == 0).mean(), (diff <= 1).mean())


def test_cli_calib(hip, oracle, tmp_path):
    """adcensus_cli ... --calib on Cone: <out>-depth.pfm and the PLY payload equal outputs_ref; -d.png, -c.png, -cloud.txt and .pfm
    are byte for byte those of a run without the flag."""
    from PIL import Image
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    left, right, opt = cases.make_case("cone")
    want = _final(oracle, left, right, opt)
    Image.fromarray(np.ascontiguousarray(left[:, :, ::-1])).save(tmp_path / "left.png")
    Image.fromarray(np.ascontiguousarray(right[:, :, ::-1])).save(tmp_path / "right.png")
    env = dict(os.environ, ADC_VERBOSE="0")
    for pref, extra in (("plain", []), ("cal", ["--calib", "3740,0.16,225,187.5,0"])):
        out = subprocess.run([cli, str(tmp_path / "left.png"), str(tmp_path / "right.png"), "0", "64", str(tmp_path / pref)] + extra,
                             capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
    for suffix in ("-d.png", "-c.png", "-cloud.txt", ".pfm"):
        assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / "cal") + suffix, "rb").read(), suffix
    assert not os.path.exists(str(tmp_path / "plain") + "-depth.pfm")
    assert _same(read_pfm(str(tmp_path / "cal") + ".pfm"), want)
    want_z, want_pts, _ = outputs_ref.outputs(want, left, CONE_CALIB)
    assert _same(read_pfm(str(tmp_path / "cal") + "-depth.pfm"), want_z)
    n, rows = read_ply(str(tmp_path / "cal") + "-cloud.ply")
    assert n == len(rows) == len(want_pts) == 168746
    for name in ("x", "y", "z"):
        assert np.array_equal(_u32(rows[name]), _u32(want_pts[name])), name
    assert all(np.array_equal(rows[c], want_pts[c]) for c in "rgb")


def test_hip_failures_on_the_output_paths(hip):
    """The fault-injection build (tests/test_gpu_faults.py): every HIP call of adc_match_out (first use included: the scratch
    allocations), adc_match_device_out + adc_wait and adc_reproject_device + adc_wait fails once -- the call reports it, the same
    handle delivers the exact outputs afterwards, nothing leaks.  tests/outputs_fault_probe.py runs in its own interpreter."""
    import json
    import sys
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "outputs_fault_probe.py")], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([l for l in r.stdout.splitlines() if l.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])
    print(o)
    # the hook sits on the new calls: memset, three launches, count read-back (5), three copy-outs, four first-use allocations
    assert o["host_calls"] >= o["plain_calls"] + 8 and o["first_calls"] >= o["host_calls"] + 4, o
    assert o["device_calls"] >= o["device_plain_calls"] + 5 and o["reproject_calls"] >= 5, o
    for name in ("host", "device", "reproject"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert abs(o["host_leak_bytes"]) <= (2 << 20) and abs(o["final_leak_bytes"]) <= (2 << 20), o
