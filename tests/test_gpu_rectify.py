"""GPU tier: the rectification (k_rectify.hip) against tests/rectify_ref.py, bit for bit -- the remap and the maps alone (images, valid
maps, the model's float maps through their uint32 view) over sizes, formats, pitches and degenerate maps; raw pairs end to end through
every match entry point against a plain Match on rectify_ref's images; every redo adc_wait can take; refusals; every HIP call of the new
paths failing once; and a handle that never had a side set making exactly the parent's HIP calls."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases
from tests import rectify_ref as RR
from tests.speckle_ref import speckle_ref
from tests.test_gpu_outputs import CONE_CALIB, POISON, DeviceBuffers, _check_outputs, _final, _handle, _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256  # poisoned bytes behind every buffer the kernels write
F = np.float32
# hooked HIP calls of a handle that never had a side set, 256x144, D = 64, no filling (tests/rectify_fault_probe.py --plain-only), of
# the parent revision: adc_match 17 and adc_match_device + adc_wait 15 (measured there); adc_create 87, counted in the
# parent's capi.hip: 1 stream + 2 + 7 + 9 events, 63 calls of alloc_all (D <= 128: the seam buffer included), 5 of upload_tables
PARENT_CALLS = {"create_calls": 87, "plain_calls": 17, "device_plain_calls": 15}


def _model(A, m):
    return A.CameraModel(**m)


def _raw_format(A, ws, hs, fmt, pad):
    return A.RawFormat(ws, hs, ws * RR.BPP[fmt] + pad, fmt)


def _remap_on_device(A, st, dev, side, raw):
    """adc_rectify_device on a poisoned output buffer with a guard behind it -> uint8 [H][W][3]"""
    n = st.width * st.height * 3
    pr, po = dev.new(raw), dev.alloc(n + GUARD, POISON)
    assert st.rectify_device(side, pr, po) and st.wait(), A.last_error()
    got = dev.get(po, n + GUARD, np.uint8)
    assert np.all(got[n:] == POISON), "written behind the rectified image"
    dev.free()
    return got[:n].reshape(st.height, st.width, 3)


def _check_side(A, st, dev, what, side, raw, fmt_desc, mx, my, model_mode):
    ws, hs, pitch, fmt = fmt_desc
    want_img, want_valid = RR.remap(raw, ws, hs, pitch, fmt, mx, my)
    got = _remap_on_device(A, st, dev, side, raw)
    assert np.array_equal(got, want_img), "%s: image differs on %d pixels" % (what, int((got != want_img).any(axis=2).sum()))
    gx, gy, gv = st.rectify_maps(side)
    assert np.array_equal(gv, want_valid), "%s: valid map differs on %d pixels" % (what, int((gv != want_valid).sum()))
    assert _same(gx, mx) and _same(gy, my), "%s: float maps (%s)" % (what, "computed" if model_mode else "returned as given")
    return want_valid


def _sources(rng, W, H):
    """(Ws, Hs) of a source larger, smaller and of the destination's size"""
    return [(W + 37, H + 21), (max(1, W - W // 3), max(1, H - H // 4)), (W, H)]


@pytest.mark.parametrize("size", [(333, 41), (130, 33), (64, 16), (1, 70), (200, 1), (1242, 375), (1920, 1080)])
def test_remap_and_maps_against_the_reference(hip, size):
    A = hip
    W, H = size
    big = W * H > 200000
    rng = np.random.default_rng(W * 31 + H)
    st, dev = _handle(A, W, H, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        k = 0
        for fmt in (RR.BGR8, RR.RGB8, RR.GRAY8, RR.BGRA8):
            for (ws, hs) in (_sources(rng, W, H)[:1] if big else _sources(rng, W, H)):
                pad = [0, 5, 3, 16][k % 4] if not big else [7, 0, 1, 4][fmt]
                side = k % 2
                k += 1
                raw_fmt = _raw_format(A, ws, hs, fmt, pad)
                raw = rng.integers(0, 256, (hs, raw_fmt.pitch_bytes), dtype=np.uint8)
                desc = (ws, hs, raw_fmt.pitch_bytes, fmt)
                what = "%dx%d <- %dx%d fmt %d pitch %d" % (W, H, ws, hs, fmt, raw_fmt.pitch_bytes)
                # the example model: most pixels valid, fractional taps
                m = RR.example_model(ws, hs, W, H)
                st.set_rectify_model(side, raw_fmt, _model(A, m))
                v = _check_side(A, st, dev, what + " example model", side, raw, desc, *RR.model_maps(m, W, H), True)
                if big:
                    print(what, "valid %.2f %%" % (100.0 * v.mean()))
                    continue
                # all coefficients 0, R = I
                m = RR.identity_model(cx=ws / 2.0, cy=hs / 2.0, f=500.0)
                m.update(new_cx=W / 2.0, new_cy=H / 2.0)
                st.set_rectify_model(side, raw_fmt, _model(A, m))
                _check_side(A, st, dev, what + " identity model", side, raw, desc, *RR.model_maps(m, W, H), True)
                # caller's maps: random around the image, salted with NaN / inf / huge, ties of the 1/32 grid, integer positions
                mx = (rng.random((H, W)) * (ws + 8) - 4).astype(F)
                my = (rng.random((H, W)) * (hs + 8) - 4).astype(F)
                grid = rng.random((H, W)) < 0.3
                mx[grid] = (rng.integers(-40, 32 * ws + 40, int(grid.sum())) / 32.0 + rng.choice([0.0, 1 / 64.0], int(grid.sum()))).astype(F)
                my[grid] = (rng.integers(-40, 32 * hs + 40, int(grid.sum())) / 32.0).astype(F)
                for mm in (mx, my):
                    salt = rng.random((H, W))
                    mm[salt < 0.02] = np.nan
                    mm[(salt >= 0.02) & (salt < 0.03)] = np.inf
                    mm[(salt >= 0.03) & (salt < 0.04)] = -np.inf
                    mm[(salt >= 0.04) & (salt < 0.06)] = F(rng.choice([32768.0, -32768.0, 32767.99, -32767.99, 1e30, -3e38]))
                st.set_rectify_maps(side, raw_fmt, mx, my)
                _check_side(A, st, dev, what + " salted maps", side, raw, desc, mx, my, False)
        # maps wholly outside; the last row / column with a zero fraction; the host convenience
        ws, hs = 40, 30
        raw_fmt = _raw_format(A, ws, hs, RR.BGR8, 2)
        raw = rng.integers(1, 256, (hs, raw_fmt.pitch_bytes), dtype=np.uint8)
        desc = (ws, hs, raw_fmt.pitch_bytes, RR.BGR8)
        for name, (mx, my) in {"outside": (np.full((H, W), -7.5, F), np.full((H, W), 1e9, F)),
                               "corner": (np.full((H, W), ws - 1, F), np.full((H, W), hs - 1, F))}.items():
            st.set_rectify_maps(A.SIDE_LEFT, raw_fmt, mx, my)
            v = _check_side(A, st, dev, "%dx%d %s" % (W, H, name), A.SIDE_LEFT, raw, desc, mx, my, False)
            assert v.all() == (name == "corner") and v.any() == (name == "corner")
            assert np.array_equal(st.rectify(raw, A.SIDE_LEFT), RR.remap(raw, ws, hs, raw_fmt.pitch_bytes, RR.BGR8, mx, my)[0])
    finally:
        dev.free()
        st.Release()


def _raw_pair(left, right, fmts, pads, grow):
    """The golden pair warped under second_model into raw frames of another size, packed into the given formats: what a rig with
    that lens would deliver.  -> per side (raw bytes, (ws, hs, pitch, fmt))"""
    H, W = left.shape[:2]
    out = []
    for img, fmt, pad, (gw, gh) in zip((left, right), fmts, pads, grow):
        ws, hs = W + gw, H + gh
        mx, my = RR.model_maps(RR.second_model(W, H, ws, hs), ws, hs)
        frame = RR.remap(img, W, H, W * 3, RR.BGR8, mx, my)[0]
        pitch = ws * RR.BPP[fmt] + pad
        out.append((RR.pack_source(frame, fmt, pitch), (ws, hs, pitch, fmt)))
    return out


def _set_both(A, obj, raws, W, H):
    """example_model on both sides of a handle or a farm -> the rectified pair rectify_ref expects"""
    want = []
    for side, (raw, (ws, hs, pitch, fmt)) in enumerate(raws):
        m = RR.example_model(ws, hs, W, H)
        obj.set_rectify_model(side, A.RawFormat(ws, hs, pitch, fmt), _model(A, m))
        want.append(RR.remap(raw, ws, hs, pitch, fmt, *RR.model_maps(m, W, H))[0])
    return want


@pytest.mark.parametrize("name", ["cone", "full_structured"])
def test_end_to_end_equals_a_plain_match_on_the_reference_images(hip, oracle, name):
    A = hip
    if name == "cone":
        left, right, opt = cases.make_case("cone")
        raws = _raw_pair(left, right, (RR.BGR8, RR.BGRA8), (5, 0), ((38, 22), (-30, -14)))
    else:
        left, right = workloads.structured_pair(1920, 1080, 128, seed=4245)
        opt = pyoracle.Option(max_disparity=128)
        raws = _raw_pair(left, right, (RR.RGB8, RR.BGR8), (0, 12), ((128, 72), (128, 72)))
    H, W = left.shape[:2]
    n = W * H
    plain = _handle(A, W, H, opt)
    st, dev = _handle(A, W, H, opt), DeviceBuffers(A)
    try:
        rl, rr = _set_both(A, st, raws, W, H)
        raw_l, raw_r = raws[0][0], raws[1][0]
        assert np.array_equal(st.rectify(raw_l, 0), rl) and np.array_equal(st.rectify(raw_r, 1), rr)
        want = plain.match(rl, rr)
        assert np.isfinite(want).mean() > 0.5
        if name == "cone":
            assert _same(want, _final(oracle, rl, rr, opt)), "the plain Match differs from the oracle on the rectified images"
        assert not _same(want, plain.match(left, right))
        assert _same(st.match(raw_l, raw_r), want), name + ": match"
        d = np.full((H, W), 7, F)
        assert st.match_async(raw_l, raw_r, d) and st.wait() and _same(d, want), name + ": match_async"
        dl, dr, dd = dev.new(raw_l), dev.new(raw_r), dev.alloc(4 * n, POISON)
        assert st.match_device(dl, dr, dd) and st.wait(), A.last_error()
        assert _same(dev.get(dd, (H, W), F), want), name + ": match_device"
        assert np.array_equal(dev.get(dl, raw_l.shape, np.uint8), raw_l), "the caller's raw image was written"
        d0, p0, c0 = plain.match_ex(rl, rr)
        d, p, c = st.match_ex(raw_l, raw_r)
        assert _same(d, want) and np.array_equal(p, p0) and _same(c, c0), name + ": match_ex"
        pp, pc = dev.alloc(n, POISON), dev.alloc(4 * n, POISON)
        assert st.match_device_ex(dl, dr, dd, pp, pc) and st.wait(), A.last_error()
        assert _same(dev.get(dd, (H, W), F), want) and np.array_equal(dev.get(pp, (H, W), np.uint8), p0) and _same(dev.get(pc, (H, W), F), c0)
        # depth, cloud COLOURS (the rectified left image) and 8-bit image
        d, z, pts, g = st.match_out(raw_l, raw_r, CONE_CALIB, depth=True, cloud=True, disp8=True)
        assert _same(d, want), name + ": match_out"
        _check_outputs(name + " match_out", want, rl, CONE_CALIB, z, pts, st.cloud_count(), g)
        pz, pcl, pn, pg = dev.alloc(4 * n), dev.alloc(16 * n), dev.alloc(16), dev.alloc(n)
        assert st.match_device_out(dl, dr, dd, CONE_CALIB, pz, pcl, n, pn, pg) and st.wait(), A.last_error()
        count = st.cloud_count()
        _check_outputs(name + " match_device_out", want, rl, CONE_CALIB, dev.get(pz, (H, W), F), dev.get(pcl, count, A.POINT_DTYPE), count,
                       dev.get(pg, (H, W), np.uint8))
        # with the speckle filter on as well
        want_f = speckle_ref(want, 100, 1.0)[0]
        st.set_speckle_filter(100, 1.0)
        assert _same(st.match(raw_l, raw_r), want_f), name + ": match with the speckle filter"
        assert st.match_device(dl, dr, dd) and st.wait() and _same(dev.get(dd, (H, W), F), want_f)
        st.set_speckle_filter(0, 0.0)
        # the farm
        farm = A.PairFarm(W, H, cases.to_product_option(opt), device=0, pipelines=2)
        try:
            _set_both(A, farm, raws, W, H)
            outs = [np.zeros((H, W), F) for _ in range(3)]
            for o in outs:
                farm.submit(raw_l, raw_r, o)
            with pytest.raises(RuntimeError):  # refused while a pair is in flight
                farm.clear_rectify()
            assert "in flight" in A.last_error()
            farm.drain()
            assert all(_same(o, want) for o in outs), name + ": farm"
            farm.clear_rectify()
            farm.submit(rl, rr, outs[0])
            farm.drain()
            assert _same(outs[0], want), name + ": farm, rectification off again"
        finally:
            farm.close()
        # off again: plain results on plain inputs
        st.clear_rectify()
        assert _same(st.match(rl, rr), want), name + ": after clear_rectify"
        dl2, dr2 = dev.new(rl), dev.new(rr)
        assert st.match_device(dl2, dr2, dd) and st.wait() and _same(dev.get(dd, (H, W), F), want)
        with pytest.raises(RuntimeError):
            st.rectify_maps(0)
    finally:
        dev.free()
        st.Release()
        plain.Release()


def _match_all(st, left, right):
    d, z, pts, g = st.match_out(left, right, CONE_CALIB, depth=True, cloud=True, disp8=True)
    return d, z, pts, st.cloud_count(), g


def _check_all(what, got, want, rect_left):
    d, z, pts, count, g = got
    assert _same(d, want), what + ": the map differs"
    _check_outputs(what, want, rect_left, CONE_CALIB, z, pts, count, g)


def test_redo_paths_with_rectification_on(hip, monkeypatch):
    """The sequence of tests/test_gpu_speckle.py's redo test with rectification on: the aggregation ring redo (counter 2), the
    scanline seam redo (counter 4, when this pair takes it), the continued voting chain (counter 1), the median fallback in both
    forms (counter 0).  The delivered map and the outputs (cloud colours included) are those of a plain Match on rectify_ref's images."""
    A = hip
    w, h, d = 256, 160, 64
    opt = pyoracle.Option(max_disparity=d)
    s_pair = workloads.structured_pair(w, h, d, seed=41)
    n_pair = workloads.noise_pair(w, h, seed=42)
    monkeypatch.setenv("ADC_AGG_DUAL", "0")
    plain = _handle(A, w, h, opt)
    s_raw = _raw_pair(*s_pair, (RR.BGR8, RR.GRAY8), (3, 0), ((20, 12), (20, 12)))
    # the noise pair goes through an identity model (raw == rectified): it keeps the short arms that make the next pair's ring too shallow
    n_fmt, n_model = A.RawFormat(w, h, 0, A.PIX_BGR8), RR.identity_model(cx=w / 2.0, cy=h / 2.0)
    st = _handle(A, w, h, opt)

    def noise_on():
        for side in (0, 1):
            st.set_rectify_model(side, n_fmt, _model(A, n_model))

    try:
        s_rect = _set_both(A, st, s_raw, w, h)
        n_rect = [RR.remap(img, w, h, w * 3, RR.BGR8, *RR.model_maps(n_model, w, h))[0] for img in n_pair]
        assert np.array_equal(n_rect[0], n_pair[0]) and np.array_equal(n_rect[1], n_pair[1])
        want_s, want_n = plain.match(*s_rect), plain.match(*n_rect)
        s_in = (s_raw[0][0], s_raw[1][0])
        _check_all("structured, first", _match_all(st, *s_in), want_s, s_rect[0])
        noise_on()
        _check_all("noise", _match_all(st, *n_pair), want_n, n_rect[0])
        _check_all("noise, small ring assumed", _match_all(st, *n_pair), want_n, n_rect[0])
        _set_both(A, st, s_raw, w, h)
        redo0, seam0 = st.debug_counter(2), st.debug_counter(4)
        _check_all("structured, aggregation redo", _match_all(st, *s_in), want_s, s_rect[0])
        print("aggregation redos", st.debug_counter(2) - redo0, "seam redos", st.debug_counter(4) - seam0, "partial", st.debug_counter(11))
        assert st.debug_counter(2) + st.debug_counter(4) >= redo0 + seam0 + 1, "no redo path was taken"
        st.debug_set_budget(4)
        over = st.debug_counter(1)
        _check_all("structured, voting chain continued", _match_all(st, *s_in), want_s, s_rect[0])
        assert st.debug_counter(1) == over + 1, "the voting continuation path was not taken"
    finally:
        st.Release()
        plain.Release()
    # the median fallback: 330 rows = the banded filter with speculative bands
    w, h, d = 240, 330, 32
    pair = workloads.structured_pair(w, h, d, seed=11)
    opt = pyoracle.Option(max_disparity=d, do_filling=0)
    raws = _raw_pair(*pair, (RR.BGRA8, RR.RGB8), (0, 7), ((-16, 10), (24, -8)))
    plain, st, dev = _handle(A, w, h, opt), _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        rect = _set_both(A, st, raws, w, h)
        want = plain.match(*rect)
        ins = (raws[0][0], raws[1][0])
        _check_all("median, first", _match_all(st, *ins), want, rect[0])
        for arg in (100, 101):
            fall = st.debug_counter(0)
            st.debug_run(A.RUN_MEDIAN, arg)
            _check_all("median fallback %d" % arg, _match_all(st, *ins), want, rect[0])
            assert st.debug_counter(0) == fall + 1, "the median fallback path was not taken"
        n = w * h
        dl, dr, dd = dev.new(ins[0]), dev.new(ins[1]), dev.alloc(4 * n, POISON)
        fall = st.debug_counter(0)
        st.debug_run(A.RUN_MEDIAN, 100)
        assert st.match_device(dl, dr, dd) and st.wait(), A.last_error()
        assert st.debug_counter(0) == fall + 1 and _same(dev.get(dd, (h, w), F), want)
    finally:
        dev.free()
        st.Release()
        plain.Release()


def test_one_side_set_and_refusals(hip):
    """Exactly one side set: every Match is refused with a message and the handle stays usable; the bad arguments of the set calls on a
    real handle; the setters while a Match is pending."""
    A = hip
    L = A.lib()
    w, h, d = 96, 40, 16
    left, right = workloads.structured_pair(w, h, d, seed=3)
    opt = pyoracle.Option(max_disparity=d)
    n = w * h
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        want = st.match(left, right)
        fmt = A.RawFormat(w, h, 0, A.PIX_BGR8)
        m = RR.identity_model(cx=w / 2.0, cy=h / 2.0)
        model = _model(A, m)
        st.set_rectify_model(A.SIDE_RIGHT, fmt, model)
        out = np.full((h, w), 7, F)
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n, POISON)
        lp, rp, op = np.ascontiguousarray(left).ctypes.data, np.ascontiguousarray(right).ctypes.data, out.ctypes.data
        for rc in (L.adc_match(st._h, lp, rp, op), L.adc_match_async(st._h, lp, rp, op), L.adc_match_device(st._h, dl, dr, dd),
                   L.adc_match_ex(st._h, lp, rp, op, None, op), L.adc_match_device_ex(st._h, dl, dr, dd, None, dd)):
            assert rc == 1 and "one side only" in A.last_error(), (rc, A.last_error())
        assert (out == 7).all() and np.all(dev.get(dd, 4 * n, np.uint8) == POISON)
        assert st.wait()
        st.clear_rectify()
        assert _same(st.match(left, right), want)
        # the identity model on both sides: raw == rectified
        st.set_rectify_model(A.SIDE_LEFT, fmt, model)
        st.set_rectify_model(A.SIDE_RIGHT, fmt, model)
        assert st.rectify_maps(0)[2].all() and _same(st.match(left, right), want)
        # bad arguments on a real handle, with the message; the state is untouched
        mp = np.zeros((h, w), F).ctypes.data
        for bad, word in ((A.RawFormat(w, h, w * 3, 9), "format"), (A.RawFormat(0, h, w * 3, 0), "width"), (A.RawFormat(w, 40000, w * 3, 0), "width"),
                          (A.RawFormat(w, h, w * 3 - 1, 0), "pitch"), (A.RawFormat(30000, 30000, 90000, 0), "2 GiB")):
            assert L.adc_set_rectify_maps(st._h, 0, C.byref(bad), mp, mp) == 1 and word in A.last_error(), A.last_error()
            assert L.adc_set_rectify_model(st._h, 0, C.byref(bad), C.byref(model)) == 1 and word in A.last_error(), A.last_error()
        assert L.adc_set_rectify_model(st._h, 5, C.byref(fmt), C.byref(model)) == 1 and "side" in A.last_error()
        assert L.adc_set_rectify_model(st._h, 0, C.byref(fmt), C.byref(_model(A, dict(m, fy=0.0)))) == 1 and "finite" in A.last_error()
        assert L.adc_set_rectify_model(st._h, 0, C.byref(fmt), C.byref(_model(A, dict(m, k2=float("nan"))))) == 1
        assert _same(st.match(left, right), want)
        # while a Match is pending
        assert st.match_device(dl, dr, dd)
        assert L.adc_set_rectify_model(st._h, 0, C.byref(fmt), C.byref(model)) == 1 and "pending" in A.last_error()
        assert L.adc_set_rectify_maps(st._h, 0, C.byref(fmt), mp, mp) == 1 and "pending" in A.last_error()
        assert L.adc_clear_rectify(st._h) == 1 and "pending" in A.last_error()
        assert st.wait() and _same(dev.get(dd, (h, w), F), want)
        st.clear_rectify()
        assert _same(st.match(left, right), want)
    finally:
        dev.free()
        st.Release()


def _probe(lib, *args):
    env = dict(os.environ, ADC_HIP_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rectify_fault_probe.py"), *args], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])


def _fault_lib():
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    return fault_lib


def test_hip_failures_on_the_rectify_paths(hip):
    """The fault-injection build: every HIP call of the two set calls' first use + a rectified adc_match, of a rectified
    adc_match_device + adc_wait, of adc_rectify_device + adc_wait and of adc_get_rectify_maps fails once -- the call reports it, the
    same handle is exact afterwards, nothing leaks.  tests/rectify_fault_probe.py runs in its own interpreter."""
    o = _probe(_fault_lib())
    print(o)
    # the hook sits on the new calls.  First set call of a handle: 8 [H][W] buffers, raw buffer, raw staging, 2 kernels, 1 wait; the
    # other side through maps: its raw buffer, 2 uploads, 1 kernel, 1 wait; a side again with the same geometry: 2 kernels, 1 wait;
    # a rectified Match: the two remap launches on top of the plain one
    assert (o["set_first_calls"], o["set_maps_calls"], o["set_second_calls"]) == (13, 5, 3), o
    assert o["rect_calls"] == o["plain_calls"] + 2 and o["device_calls"] == o["device_plain_calls"] + 2 and o["remap_calls"] >= 2, o
    for name in ("host", "device", "remap", "getmaps"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert abs(o["host_leak_bytes"]) <= (2 << 20) and abs(o["final_leak_bytes"]) <= (2 << 20), o


def test_off_equals_the_parent_revision(hip):
    """Neither set call has been made: the hooked HIP calls of adc_create, adc_match and adc_match_device + adc_wait are the parent
    revision's (profiles/rectify_kernel_stats.md has both measurements and the kernel trace of the plain Match)."""
    o = _probe(_fault_lib(), "--plain-only")
    print(o)
    assert {k: o[k] for k in PARENT_CALLS} == PARENT_CALLS, o
