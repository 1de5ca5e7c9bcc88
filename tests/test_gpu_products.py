"""GPU tier: every optional product of a Match through adc_products -- synchronous, asynchronous, device-resident and through the pair
farm -- and the 16-bit fixed-point map (k_disp16), bit for bit (uint32 view for floats, raw bytes for points and uint16).  Expected
values come from the oracle's stage dumps through tests/extras_ref.py, tests/outputs_ref.py, tests/speckle_ref.py and
tests/products_ref.py; every output buffer is poisoned (0xA5) first."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases, products_ref, rawfmt_ref
from tests.test_gpu_outputs import DeviceBuffers, _handle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
F = np.float32
CALIB = (3740.0, 0.16, 48.0, 32.0, 0.5)  # doffs > 0: every finite pixel is a point, the zero included
SCALE = 256.0
MAPS = (("provenance", np.uint8), ("confidence", np.float32), ("depth", np.float32), ("disp8", np.uint8), ("disp16", np.uint16))
ALL = tuple(n for n, _ in MAPS) + ("cloud",)


def _poison(n, dtype):
    return np.frombuffer(bytearray([POISON]) * (n * np.dtype(dtype).itemsize), dtype)


class Request:
    """poisoned host arrays for the products in `which`, the map, and the adc_products that points at them; the cloud array has
    `capacity` points and 8 poisoned ones behind them"""

    def __init__(self, A, w, h, which=ALL, calib=CALIB, scale=SCALE, capacity=None, arrays=None):
        n = w * h
        self.cap = n if capacity is None else capacity
        self.disp = _poison(n, F).reshape(h, w) if arrays is None else arrays["disparity"]
        self.arr = {name: (_poison(n, dt).reshape(h, w) if arrays is None else arrays[name]) for name, dt in MAPS if name in which}
        self.cloud_all = None
        if "cloud" in which:
            self.cloud_all = _poison(self.cap + 8, A.POINT_DTYPE) if arrays is None else arrays["cloud"]
        self.req = A.Products.from_arrays(calib=calib, cloud=None if self.cloud_all is None else self.cloud_all[:self.cap], disp16_scale=scale,
                                          **self.arr)

    def check(self, what, want):
        """every requested product equals the definition's; nothing behind the last point was written"""
        assert self.disp.tobytes() == want["disparity"].tobytes(), what + ": the map differs"
        for name, a in self.arr.items():
            assert a.tobytes() == np.ascontiguousarray(want[name]).tobytes(), "%s: %s differs on %d elements" % (what, name, int((a != want[name]).sum()))
        if self.cloud_all is not None:
            pts = want["cloud"]
            assert int(self.req.count[0]) == len(pts), "%s: count %d, expected %d" % (what, int(self.req.count[0]), len(pts))
            k = min(self.cap, len(pts))
            assert self.cloud_all[:k].tobytes() == pts[:k].tobytes(), what + ": the points differ"
            assert self.cloud_all[k:].tobytes() == bytes([POISON]) * (16 * (self.cap + 8 - k)), what + ": written behind the last point"

    def buffers(self):
        return [self.disp] + list(self.arr.values()) + ([] if self.cloud_all is None else [self.cloud_all])

    def untouched(self):
        return all(b.tobytes() == bytes([POISON]) * b.nbytes for b in self.buffers())

    def repoison(self):
        for b in self.buffers():
            b.view(np.uint8).reshape(-1)[:] = POISON


_WANT = {}


def _want(oracle, key, left, right, opt, speckle=None, calib=CALIB, scale=SCALE):
    """the products of one oracle run (computed once per key, shared, never modified)"""
    if key not in _WANT:
        o = oracle.run(left, right, opt, stages=products_ref.STAGES)
        _WANT[key] = products_ref.products(o, opt, left, calib, scale, speckle)
    return _WANT[key]


def _pair_96(kind):
    return workloads.noise_pair(96, 64, seed=71) if kind == "noise" else workloads.structured_pair(96, 64, 16, seed=71)


def _want_96(oracle, kind, filling):
    left, right = _pair_96(kind)
    return _want(oracle, ("96", kind, filling), left, right, pyoracle.Option(max_disparity=16, do_filling=filling))


def _special_values():
    tiny, den, big = F(np.finfo(np.float32).tiny), F(1e-45), F(np.finfo(np.float32).max)
    rng = np.random.default_rng(9)
    rnd = (rng.random(4096, dtype=np.float32) * F(300) - F(40)).astype(F)
    return np.concatenate([np.array([0.0, -0.0, 2.5, -2.5, np.nan, np.inf, -np.inf, den, -den, tiny, big, -big, 3.999, 0.999, 255.998, 7.99994, 65534.99,
                                     0.0039], F), rnd])


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (61, 37), (64, 4)])
def test_disp16_kernel_alone(hip, size):
    """adc_disp16_device on synthetic maps holding the CPU tier's values: the vector form with its tail, then the element-wise form
    (the output address moved by 2 bytes inside a larger allocation); one poisoned element behind the end stays."""
    A = hip
    w, h = size
    n = w * h
    vals = _special_values()
    disp = np.roll(np.resize(vals, n), 0).reshape(h, w).astype(F)
    st, dev = _handle(A, w, h, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        dd = dev.new(disp)
        for scale in (256.0, 4.0, 1.0, 8192.0):
            want = products_ref.disp16(disp, scale).reshape(-1)
            for shift in (0, 1):  # elements: 0 = the allocation's start (vector form), 1 = 2 bytes in (element-wise form)
                po = dev.alloc(2 * (n + 2) + 16, POISON)
                assert st.disp16_device(dd, scale, po + 2 * shift) and st.wait(), A.last_error()
                got = dev.get(po, n + 2, np.uint16)
                assert np.array_equal(got[shift:shift + n], want), (size, scale, shift, int((got[shift:shift + n] != want).sum()))
                assert got[shift + n] == 0xA5A5 and (shift == 0 or got[0] == 0xA5A5), (size, scale, shift)
        assert not st.disp16_device(dd, 256.0, po + 1) and "even" in A.last_error()
        assert not st.disp16_device(dd, float("nan"), po) and not st.disp16_device(dd, 0.0, po) and "scale" in A.last_error()
    finally:
        dev.free()
        st.Release()


def _sync_cases():
    out = {name: cases.make_case(name) for name in ("cone_nofill", "cone_neg", "q_9x20_d8")}
    out["noise_61x37_d8"] = workloads.noise_pair(61, 37, seed=72) + (pyoracle.Option(max_disparity=8),)
    return out


@pytest.mark.parametrize("name", ["cone_nofill", "cone_neg", "q_9x20_d8", "noise_61x37_d8"])
def test_synchronous_call(hip, oracle, name):
    """adc_match_products with everything requested, then each product alone, then none; and the device entry point."""
    A = hip
    left, right, opt = _sync_cases()[name]
    h, w = left.shape[:2]
    n = w * h
    calib = (3740.0, 0.16, w / 2.0, h / 2.0, 0.5)
    want = _want(oracle, ("sync", name), left, right, opt, calib=calib)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        for rep in range(2):
            r = Request(A, w, h, calib=calib)
            assert st.MatchProducts(left, right, r.disp, r.req), A.last_error()
            r.check("%s all %d" % (name, rep), want)
        for one in ALL:
            r = Request(A, w, h, which=(one,), calib=calib)
            assert st.MatchProducts(left, right, r.disp, r.req), A.last_error()
            r.check("%s %s alone" % (name, one), want)
        for req in (None, A.Products.from_arrays()):
            d = _poison(n, F).reshape(h, w)
            assert st.MatchProducts(left, right, d, req) and d.tobytes() == want["disparity"].tobytes()
        got = st.match_products(left, right, calib, provenance=True, cloud=True, disp16_scale=SCALE)
        assert sorted(got) == ["cloud", "cloud_count", "disp16", "disparity", "provenance"] and got["cloud"].tobytes() == want["cloud"].tobytes()
        # the device entry point: the caller's device buffers, written directly
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n, POISON)
        p = {name_: dev.alloc(n * np.dtype(dt).itemsize, POISON) for name_, dt in MAPS}
        pc, pn = dev.alloc(16 * (n + 1), POISON), dev.alloc(16, POISON)
        req = A.Products.from_addresses(p["provenance"], p["confidence"], calib, p["depth"], pc, n, pn, p["disp8"], p["disp16"], SCALE)
        assert st.match_device_products(dl, dr, dd, req) and st.wait(), A.last_error()
        assert dev.get(dd, (h, w), F).tobytes() == want["disparity"].tobytes()
        for name_, dt in MAPS:
            assert dev.get(p[name_], (h, w), dt).tobytes() == np.ascontiguousarray(want[name_]).tobytes(), name_
        count = st.cloud_count()
        assert count == len(want["cloud"]) == int(dev.get(pn, 1, np.uint32)[0])
        pts = dev.get(pc, n + 1, A.POINT_DTYPE)
        assert pts[:count].tobytes() == want["cloud"].tobytes() and pts[count:].tobytes() == bytes([POISON]) * (16 * (n + 1 - count))
    finally:
        dev.free()
        st.Release()


def _async(A, st, left, right, r):
    """adc_match_async_products with copies of the images that are overwritten as soon as the call returns, then adc_wait"""
    l, rt = left.copy(), right.copy()
    ok = st.match_async_products(l, rt, r.disp, r.req)
    l[:] = 0x5A
    rt[:] = 0xC3
    return ok and st.wait()


@pytest.mark.parametrize("shape", ["noise_fill0", "noise_fill1", "structured_fill0", "structured_fill1", "noise_61x37"])
def test_asynchronous_call(hip, oracle, shape):
    """adc_match_async_products + adc_wait; a cloud capacity of 1000 where 1964 pixels are valid; a second adc_wait delivers nothing."""
    A = hip
    if shape == "noise_61x37":
        left, right = workloads.noise_pair(61, 37, seed=72)
        opt = pyoracle.Option(max_disparity=8)
        want = _want(oracle, "async61", left, right, opt)
    else:
        kind, filling = shape.split("_fill")
        left, right = _pair_96(kind)
        opt = pyoracle.Option(max_disparity=16, do_filling=int(filling))
        want = _want_96(oracle, kind, int(filling))
    h, w = left.shape[:2]
    st = _handle(A, w, h, opt)
    try:
        caps = [None]
        if shape == "noise_fill0":
            assert len(want["cloud"]) == 1964 and int((want["disp16"] == 0).sum()) == 4180
            caps = [None, 1000, 0]
        if shape == "structured_fill0":
            assert len(want["cloud"]) == 5824
        for cap in caps:
            r = Request(A, w, h, capacity=cap)
            assert _async(A, st, left, right, r), A.last_error()
            r.check("%s capacity %s" % (shape, cap), want)
            assert st.cloud_count() == len(want["cloud"])
            r.repoison()
            assert st.wait() and r.untouched(), "a second adc_wait without a Match delivered something"
        # a plain asynchronous Match on the same handle afterwards
        d = _poison(w * h, F).reshape(h, w)
        assert st.match_async(left, right, d) and st.wait() and d.tobytes() == want["disparity"].tobytes()
    finally:
        st.Release()


FARM_KINDS = ["noise", "structured", "structured", "noise", "noise", "structured", "structured"]  # tickets 2, 4, 6: 5824, 1964, 5824 points


def test_farm(hip, oracle):
    """7 pairs through 3 pipelines: odd tickets plain, even tickets with every product (each pipeline serves both kinds in turn),
    consecutive clouds of 5824 and 1964 points; wait(2), then drain() == 7."""
    A = hip
    w, h = 96, 64
    opt = pyoracle.Option(max_disparity=16, do_filling=0)
    wants = {k: _want_96(oracle, k, 0) for k in ("noise", "structured")}
    assert (len(wants["noise"]["cloud"]), len(wants["structured"]["cloud"])) == (1964, 5824)
    farm = A.PairFarm(w, h, cases.to_product_option(opt), device=0, pipelines=3)
    try:
        reqs = []
        for i, kind in enumerate(FARM_KINDS):
            left, right = (a.copy() for a in _pair_96(kind))
            r = Request(A, w, h)
            t = farm.submit(left, right, r.disp, r.req if (i + 1) % 2 == 0 else None)
            left[:] = 0x5A
            right[:] = 0xC3
            assert t == i + 1
            reqs.append(r)
        farm.wait(2)
        reqs[1].check("ticket 2 after wait(2)", wants[FARM_KINDS[1]])
        assert farm.drain() == 7
        for i, (kind, r) in enumerate(zip(FARM_KINDS, reqs)):
            if (i + 1) % 2 == 0:
                r.check("ticket %d" % (i + 1), wants[kind])
            else:
                assert r.disp.tobytes() == wants[kind]["disparity"].tobytes(), i + 1
                r.disp.view(np.uint8).reshape(-1)[:] = POISON
                assert r.untouched(), "ticket %d carried no request: its product buffers must stay poisoned" % (i + 1)
    finally:
        farm.close()


def test_registered_destinations(hip, oracle):
    """Destinations inside an adc_host_register'ed range are written in place and hold the same bytes."""
    A = hip
    w, h = 96, 64
    n = w * h
    left, right = _pair_96("noise")
    opt = pyoracle.Option(max_disparity=16, do_filling=0)
    want = _want_96(oracle, "noise", 0)
    sizes = [("disparity", 4 * n), ("provenance", n), ("confidence", 4 * n), ("depth", 4 * n), ("disp8", n), ("disp16", 2 * n), ("cloud", 16 * (n + 8))]
    big = _poison(sum((s + 63) // 64 * 64 for _, s in sizes) + 64, np.uint8)
    arrays, at = {}, (-big.ctypes.data) % 64
    for (name, size), dt in zip(sizes, (F, np.uint8, F, F, np.uint8, np.uint16, A.POINT_DTYPE)):
        a = big[at:at + size].view(dt)
        arrays[name] = a if name == "cloud" else a.reshape(h, w)
        at += (size + 63) // 64 * 64
    st = _handle(A, w, h, opt)
    A.host_register(big)
    try:
        r = Request(A, w, h, arrays=arrays)
        assert _async(A, st, left, right, r), A.last_error()
        r.check("registered, asynchronous", want)
        big[:] = POISON
        assert st.MatchProducts(left, right, r.disp, r.req), A.last_error()
        r.check("registered, synchronous", want)
        plain = Request(A, w, h)
        assert _async(A, st, left, right, plain)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plain.buffers(), r.buffers()))
    finally:
        st.Release()
        A.host_unregister(big)


def test_redo_paths_keep_the_products_exact(hip, oracle, monkeypatch):
    """The sequence of tests/test_gpu_outputs.py::test_redo_paths_keep_the_outputs_exact through adc_match_async_products: the
    aggregation ring redo (counter 2), the continued voting chain (counter 1), the median fallback in both forms (counter 0)."""
    A = hip
    w, h, d = 256, 160, 64
    opt = pyoracle.Option(max_disparity=d)
    s_pair = workloads.structured_pair(w, h, d, seed=41)
    n_pair = workloads.noise_pair(w, h, seed=42)
    want_s, want_n = _want(oracle, "redo_s", *s_pair, opt), _want(oracle, "redo_n", *n_pair, opt)
    monkeypatch.setenv("ADC_AGG_DUAL", "0")

    def run(st, what, pair, want, ww=w, hh=h):
        r = Request(A, ww, hh)
        assert _async(A, st, pair[0], pair[1], r), A.last_error()
        r.check(what, want)

    st = _handle(A, w, h, opt)
    try:
        run(st, "structured, first", s_pair, want_s)
        run(st, "noise", n_pair, want_n)
        run(st, "noise, small ring assumed", n_pair, want_n)
        redo0 = st.debug_counter(2)
        run(st, "structured, aggregation redo", s_pair, want_s)
        assert st.debug_counter(2) == redo0 + 1, "the aggregation redo path was not taken"
    finally:
        st.Release()
    st = _handle(A, w, h, opt)
    try:
        run(st, "structured, new handle", s_pair, want_s)
        st.debug_set_budget(4)
        over = st.debug_counter(1)
        run(st, "structured, voting chain continued", s_pair, want_s)
        assert st.debug_counter(1) == over + 1, "the voting continuation path was not taken"
    finally:
        st.Release()
    w2, h2, d2 = 240, 330, 32
    pair = workloads.structured_pair(w2, h2, d2, seed=11)
    opt2 = pyoracle.Option(max_disparity=d2, do_filling=0)
    want = _want(oracle, "redo_median", *pair, opt2)
    assert np.isinf(want["disparity"]).any()
    st = _handle(A, w2, h2, opt2)
    try:
        run(st, "median, first", pair, want, w2, h2)
        for arg in (100, 101):
            fall = st.debug_counter(0)
            st.debug_run(A.RUN_MEDIAN, arg)
            run(st, "median fallback %d" % arg, pair, want, w2, h2)
            assert st.debug_counter(0) == fall + 1, "the median fallback path was not taken"
    finally:
        st.Release()


def test_handle_state_on_the_farm(hip, oracle):
    """Speckle filter (50, 1.0) and a conversion-only ADC_PIX_GRAY8 input format on a farm with products: the numpy definitions on the
    oracle's map of the converted pair; ADC_PROV_SPECKLE where speckle_ref removes pixels; cloud colours from the converted image."""
    A = hip
    w, h = 96, 64
    src_l, src_r = _pair_96("noise")
    raw_l, raw_r = np.ascontiguousarray(src_l[..., 1]), np.ascontiguousarray(src_r[..., 1])
    left = rawfmt_ref.decode(raw_l, w, h, w, rawfmt_ref.GRAY8).astype(np.uint8)
    right = rawfmt_ref.decode(raw_r, w, h, w, rawfmt_ref.GRAY8).astype(np.uint8)
    assert left.shape == (h, w, 3) and np.array_equal(left[..., 0], raw_l) and np.array_equal(left[..., 2], raw_l)
    opt = pyoracle.Option(max_disparity=16)
    want = _want(oracle, "farm_state", left, right, opt, speckle=(50, 1.0))
    removed = (want["provenance"] & products_ref.PROV_SPECKLE) != 0
    assert removed.any() and np.all(np.isinf(want["disparity"][removed]))
    farm = A.PairFarm(w, h, cases.to_product_option(opt), device=0, pipelines=2)
    try:
        farm.set_speckle_filter(50, 1.0)
        for side in (A.SIDE_LEFT, A.SIDE_RIGHT):
            farm.set_input_format(side, A.RawFormat(w, h, 0, A.PIX_GRAY8))
        reqs = [Request(A, w, h) for _ in range(3)]
        for r in reqs:
            farm.submit(raw_l, raw_r, r.disp, r.req)
        assert farm.drain() == 3
        for i, r in enumerate(reqs):
            r.check("farm pair %d" % i, want)
    finally:
        farm.close()


def test_refusals(hip, oracle):
    """Each refusal returns 1 with adc_last_error and writes nothing; a correct call on the same handle afterwards is exact."""
    A = hip
    L = A.lib()
    left, right, opt = cases.make_case("q_9x20_d8")
    h, w = left.shape[:2]
    n = w * h
    want = _want(oracle, ("sync", "q_9x20_d8"), left, right, opt, calib=(3740.0, 0.16, w / 2.0, h / 2.0, 0.5))
    calib = (3740.0, 0.16, w / 2.0, h / 2.0, 0.5)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    farm = A.PairFarm(w, h, cases.to_product_option(opt), device=0, pipelines=2)
    try:
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n, POISON)
        p = {name: dev.alloc(n * np.dtype(dt).itemsize + 16, POISON) for name, dt in MAPS}
        pc = dev.alloc(16 * n + 16, POISON)
        held = []

        def refused(word, which=ALL, device_req=None, **kw):
            """the three host forms, the farm and (device_req) the device form refuse the request; nothing is written"""
            r = Request(A, w, h, which=which, **kw)
            held.append(r)
            lp, rp = left.ctypes.data, right.ctypes.data
            for fn in (L.adc_match_products, L.adc_match_async_products):
                assert fn(st._h, lp, rp, r.disp.ctypes.data, C.byref(r.req)) == 1 and word in A.last_error(), (word, A.last_error())
            t = C.c_uint64(0)
            assert L.adc_farm_submit_products(farm._f, lp, rp, r.disp.ctypes.data, C.byref(r.req), C.byref(t)) == 1 and word in A.last_error(), word
            if device_req is not None:
                assert L.adc_match_device_products(st._h, dl, dr, dd, C.byref(device_req)) == 1 and word in A.last_error(), (word, A.last_error())
            assert st.wait() and farm.drain() == 0 and r.untouched(), word

        refused("calibration", calib=None, device_req=A.Products.from_addresses(depth=p["depth"]))
        for bad, word in (((0.0, 0.16, 1, 1, 0), "focal_px"), ((float("nan"), 0.16, 1, 1, 0), "finite"), ((100.0, 0.16, 1, 1, float("inf")), "finite")):
            refused(word, calib=bad, device_req=A.Products.from_addresses(calib=bad, disp8=p["disp8"]))
        for scale in (float("nan"), float("inf"), 0.0, -256.0):
            refused("disp16_scale", scale=scale, device_req=A.Products.from_addresses(disp16=p["disp16"], disp16_scale=scale))
        st.set_paper_modes(A.PAPER_CENSUS5X5)
        r = Request(A, w, h, which=("provenance",))
        assert not st.MatchProducts(left, right, r.disp, r.req) and "paper" in A.last_error() and r.untouched()
        assert not st.match_device_products(dl, dr, dd, A.Products.from_addresses(confidence=p["confidence"])) and "paper" in A.last_error()
        st.set_paper_modes(0)
        # device addresses: an odd one for disp16, a cloud that is not 16-byte aligned
        assert not st.match_device_products(dl, dr, dd, A.Products.from_addresses(disp16=p["disp16"] + 1)) and "even" in A.last_error()
        assert not st.match_device_products(dl, dr, dd, A.Products.from_addresses(cloud=pc + 4, cloud_capacity=n - 1)) and "aligned" in A.last_error()
        # the farm has no per-ticket getter: a cloud needs cloud_count
        r = Request(A, w, h, which=("cloud",))
        r.req.out.cloud_count = None
        t = C.c_uint64(0)
        assert L.adc_farm_submit_products(farm._f, left.ctypes.data, right.ctypes.data, r.disp.ctypes.data, C.byref(r.req), C.byref(t)) == 1
        assert "cloud_count" in A.last_error() and t.value == 0 and farm.drain() == 0 and r.untouched()
        # a products call while a Match is pending on the handle
        d0 = _poison(n, F).reshape(h, w)
        assert st.match_async(left, right, d0)
        r = Request(A, w, h)
        assert not st.match_async_products(left, right, r.disp, r.req) and "pending" in A.last_error()
        assert not st.MatchProducts(left, right, r.disp, r.req) and "pending" in A.last_error()
        assert not st.match_device_products(dl, dr, dd, A.Products.from_addresses(disp16=p["disp16"])) and "pending" in A.last_error()
        assert st.wait() and d0.tobytes() == want["disparity"].tobytes() and r.untouched()
        # nothing reached the device buffers either
        for name, dt in MAPS:
            assert np.all(dev.get(p[name], n * np.dtype(dt).itemsize, np.uint8) == POISON), name
        assert np.all(dev.get(dd, 4 * n, np.uint8) == POISON) and np.all(dev.get(pc, 16 * n, np.uint8) == POISON)
        # correct calls afterwards are exact: the handle, and the farm
        r = Request(A, w, h, calib=calib)
        assert _async(A, st, left, right, r), A.last_error()
        r.check("after the refusals", want)
        r = Request(A, w, h, calib=calib)
        assert farm.submit(left, right, r.disp, r.req) == 1 and farm.drain() == 1
        r.check("farm after the refusals", want)
    finally:
        farm.close()
        dev.free()
        st.Release()


def test_plain_paths_unchanged_and_hip_failures(hip):
    """The fault-injection build: a NULL request makes the HIP calls of the plain entry points; every HIP call of an asynchronous
    products Match and of a farm products submit + drain fails once (an injected return code) -- the call or its wait reports it, the
    next call on the same handle / farm is exact, nothing leaks.  tests/products_fault_probe.py runs in its own interpreter."""
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "products_fault_probe.py")], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([l for l in r.stdout.splitlines() if l.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])
    print(o)
    for name in ("sync", "async", "farm"):
        assert o[name + "_null_calls"] == o[name + "_plain_calls"] and o[name + "_empty_calls"] == o[name + "_plain_calls"], (name, o)
    # the hook sits on the new calls: the outputs' memset, three launches and count read-back, the disp16 launch, five staging copies
    # and the cloud copy-out (12), and on the first-use allocations (seven device blocks, five pinned ones)
    assert o["async_calls"] >= o["async_plain_calls"] + 12 and o["async_first_calls"] >= o["async_calls"] + 11, o
    assert o["farm_calls"] >= o["farm_plain_calls"] + 12, o
    for name in ("async", "farm"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert abs(o["async_leak_bytes"]) <= (2 << 20) and abs(o["final_leak_bytes"]) <= (2 << 20), o
