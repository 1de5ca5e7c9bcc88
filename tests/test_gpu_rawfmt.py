"""GPU tier: the camera layouts (16-bit gray, Bayer, YUYV / UYVY, NV12; k_rectify.hip) against tests/rawfmt_ref.py, bit for bit, no
tolerance anywhere -- the conversion alone (adc_set_input_format + adc_rectify_device) and the remap with the new decodes over sizes,
pitches and significant bits; Cone as camera frames end to end through every match entry point against the oracle's Match on the
numpy-decoded (and numpy-remapped) images; every redo adc_wait can take with a Bayer side; refusals; the CLI's --raw; every HIP call of
the new paths failing once."""
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
from tests import rawfmt_ref as RF
from tests import rectify_ref as RR
from tests.test_gpu_outputs import CONE_CALIB, POISON, DeviceBuffers, _check_outputs, _final, _handle, _same
from tests.test_outputs_api import read_pfm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256  # poisoned bytes behind every buffer the kernels write
F = np.float32


def _variants(fmt):
    """the format words a layout is tested with: 10 and 12 significant bits for the 16-bit ones"""
    return [RF.pix_bits(fmt, 10), RF.pix_bits(fmt, 12)] if fmt in RF.SIXTEEN else [fmt]


def _legal(fmt, ws, hs):
    (w0, h0), (sw, sh) = RF.min_size(fmt)
    return ws >= w0 and hs >= h0 and ws % sw == 0 and hs % sh == 0


def _pitch(fmt, ws, pad):
    """a row of the layout plus `pad` bytes (kept even for the 16-bit layouts)"""
    return ws * RF.BPP[fmt & 0xff] + (pad + (pad & 1) if (fmt & 0xff) in RF.SIXTEEN else pad)


def _on_device(A, st, dev, side, raw):
    """adc_rectify_device on a poisoned output buffer with a guard behind it -> uint8 [H][W][3]"""
    n = st.width * st.height * 3
    pr, po = dev.new(raw), dev.alloc(n + GUARD, POISON)
    assert st.rectify_device(side, pr, po) and st.wait(), A.last_error()
    got = dev.get(po, n + GUARD, np.uint8)
    assert np.all(got[n:] == POISON), "written behind the image"
    dev.free()
    return got[:n].reshape(st.height, st.width, 3)


@pytest.mark.parametrize("size", [(2, 2), (4, 2), (6, 4), (64, 16), (130, 34), (334, 42), (1920, 1080), (3, 3), (333, 41)])
def test_conversion_alone_against_the_reference(hip, size):
    """adc_set_input_format + adc_rectify_device == rawfmt_ref.decode for every layout, with the exact and a padded pitch (the odd
    sizes: Bayer and GRAY16, where they are legal).  1920 x 1080: every layout once, pitch and bits alternating."""
    A = hip
    W, H = size
    big = W * H > 200000
    rng = np.random.default_rng(W * 131 + H)
    st, dev = _handle(A, W, H, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        k = tested = 0
        for code in (RF.BGR8, RF.RGB8, RF.GRAY8, RF.BGRA8) + RF.NEW_FORMATS:
            if not _legal(code, W, H) or ((W & 1 or H & 1) and code in RR.BPP):
                continue
            k += 1
            combos = [(fmt, pad) for fmt in _variants(code) for pad in (0, [5, 16, 3, 2][k % 4])]
            if big:
                combos = [combos[k % len(combos)]]
            tested += 1
            for fmt, pad in combos:
                pitch = _pitch(fmt, W, pad)
                raw = RF.random_frame(rng, W, H, pitch, fmt)
                side = (k + pad) % 2
                st.set_input_format(side, A.RawFormat(W, H, pitch, fmt))
                want = RF.decode(raw, W, H, pitch, fmt).astype(np.uint8)
                got = _on_device(A, st, dev, side, raw)
                what = "%dx%d %s bits %d pitch %d" % (W, H, RF.NAMES[code], fmt >> 8, pitch)
                assert np.array_equal(got, want), "%s: differs on %d pixels" % (what, int((got != want).any(axis=2).sum()))
                with pytest.raises(RuntimeError):  # no maps on such a side
                    st.rectify_maps(side)
                assert "no maps" in A.last_error()
        assert tested == (9 if (W & 1 or H & 1) else 16)
    finally:
        dev.free()
        st.Release()


def _synthetic_map(W, H, ws, hs):
    """Quasi-random positions on the 1/32 grid from 3 pixels outside to 2 pixels behind the source on every side, and on fixed pixels:
    exits by whole pixels on all four sides, the last row / column exactly (zero-weight taps outside) and a fraction behind it, the
    fractional positions next to every edge whose inside taps reflect (Bayer), NaN and +-inf."""
    t = np.arange(W * H, dtype=np.float64)
    mx = (np.round((-3.0 + (ws + 5.0) * ((t * 0.6180339887498949) % 1.0)) * 32.0) / 32.0).astype(F)
    my = (np.round((-3.0 + (hs + 5.0) * ((t * 0.7548776662466927) % 1.0)) * 32.0) / 32.0).astype(F)
    fr = 11 / 32.0
    special = [(-1, 1), (-2, hs - 1), (ws, 0), (ws + 1, 1), (1, -1), (0, -2), (1, hs), (0, hs + 1),                 # whole pixels outside
               (ws - 1, 0 + fr), (0 + fr, hs - 1), (ws - 1, hs - 1), (ws - 1 + fr, 0), (1, hs - 1 + fr),             # the last row / column
               (ws - 2 + fr, hs - 2 + fr), (fr, fr), (ws - 2 + fr, fr), (fr, hs - 2 + fr), (0, 0), (ws - 2, hs - 2),  # reflecting taps
               (-fr, 1), (1, -fr), (-1 + fr, -1 + fr),                                                              # fractions outside
               (np.nan, 1), (1, np.nan), (np.inf, 0), (0, -np.inf), (-np.inf, np.inf)]
    assert W * H >= 2 * len(special)
    at = (np.arange(len(special)) * ((W * H) // len(special))).astype(np.int64)  # spread over the destination
    mx[at] = np.array([s[0] for s in special], F)
    my[at] = np.array([s[1] for s in special], F)
    return mx.reshape(H, W), my.reshape(H, W)


def test_the_synthetic_map_does_what_it_says():
    W, H, ws, hs = 64, 16, 102, 38
    mx, my = _synthetic_map(W, H, ws, hs)
    outside, xi, ax, yi, ay = RR.quantise(mx, my)
    ok = ~outside
    assert outside.sum() >= 5 and np.isnan(mx).any() and np.isposinf(mx).any() and np.isneginf(my).any()
    for lo, hi, n, a in ((xi, xi, ws, ax), (yi, yi, hs, ay)):
        assert (ok & (lo < 0) & (a == 0)).any() and (ok & (lo < 0) & (a != 0)).any()          # out by whole and by fractional pixels
        assert (ok & (hi >= n) & (a == 0)).any() and (ok & (hi == n - 1) & (a != 0)).any()
        assert (ok & (hi == n - 1) & (a == 0)).any()                                          # exactly the last row / column
        assert (ok & (hi == n - 2) & (a != 0)).any() and (ok & (lo == 0) & (a != 0)).any()    # reflecting taps with nonzero weights


@pytest.mark.parametrize("size", [(333, 41), (130, 33), (64, 16), (1, 70), (200, 1), (1242, 375)])
def test_remap_against_the_reference(hip, size):
    """Every new layout under rectify_ref.example_model's maps and under the synthetic map: image and valid map equal rawfmt_ref.remap."""
    A = hip
    W, H = size
    big = W * H > 200000
    rng = np.random.default_rng(W * 37 + H)
    st, dev = _handle(A, W, H, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    ws, hs = (W + 38) & ~1, (H + 22) & ~1  # (even: legal for every layout)
    try:
        k = 0
        for code in RF.NEW_FORMATS:
            k += 1
            vs = _variants(code)
            for fmt in ([vs[k % len(vs)]] if big else vs):
                pad = [0, 6, 3, 16][(k + (fmt >> 8)) % 4]
                side = k % 2
                pitch = _pitch(fmt, ws, pad)
                raw_fmt = A.RawFormat(ws, hs, pitch, fmt)
                raw = RF.random_frame(rng, ws, hs, pitch, fmt)
                what = "%dx%d <- %dx%d %s bits %d pitch %d" % (W, H, ws, hs, RF.NAMES[code], fmt >> 8, pitch)
                m = RR.example_model(ws, hs, W, H)
                cases_ = [("example model", RR.model_maps(m, W, H), lambda: st.set_rectify_model(side, raw_fmt, A.CameraModel(**m)))]
                if not big:
                    sm = _synthetic_map(W, H, ws, hs)
                    cases_.append(("synthetic map", sm, lambda: st.set_rectify_maps(side, raw_fmt, *sm)))
                for name, (mx, my), setter in cases_:
                    setter()
                    want_img, want_valid = RF.remap(raw, ws, hs, pitch, fmt, 0, mx, my)
                    got = _on_device(A, st, dev, side, raw)
                    assert np.array_equal(got, want_img), "%s, %s: image differs on %d pixels" % (what, name, int((got != want_img).any(axis=2).sum()))
                    gv = st.rectify_maps(side)[2]
                    assert np.array_equal(gv, want_valid), "%s, %s: valid map differs on %d pixels" % (what, name, int((gv != want_valid).sum()))
    finally:
        dev.free()
        st.Release()


# ---------------------------------------------------------------------------------------------- end to end
def _cone():
    """Cone without its last row: 450 x 374, even in both directions (NV12)"""
    left, right, opt = cases.make_case("cone")
    return np.ascontiguousarray(left[:374]), np.ascontiguousarray(right[:374]), opt


PAIRS = {"grbg8_nv12": ((RF.BAYER_GRBG8, RF.NV12), (3, 0)), "yuyv_rggb16": ((RF.YUYV, RF.pix_bits(RF.BAYER_RGGB16, 12)), (0, 6))}


def _frames(left, right, name):
    """-> per side (frame bytes, (ws, hs, pitch, fmt))"""
    fmts, pads = PAIRS[name]
    H, W = left.shape[:2]
    out = []
    for img, fmt, pad in zip((left, right), fmts, pads):
        pitch = _pitch(fmt, W, pad)
        out.append((RF.pack(img, fmt, pitch), (W, H, pitch, fmt)))
    return out


def _set_both(A, obj, frames, W, H, mode):
    """`mode` "format": conversion only; "model": rectify_ref.second_model on both sides -> the pair the numpy definition expects"""
    want = []
    for side, (raw, (ws, hs, pitch, fmt)) in enumerate(frames):
        rf = A.RawFormat(ws, hs, pitch, fmt)
        if mode == "format":
            obj.set_input_format(side, rf)
            want.append(RF.decode(raw, ws, hs, pitch, fmt).astype(np.uint8))
        else:
            m = RR.second_model(ws, hs, W, H)
            obj.set_rectify_model(side, rf, A.CameraModel(**m))
            want.append(RF.remap(raw, ws, hs, pitch, fmt, 0, *RR.model_maps(m, W, H))[0])
    return want


@pytest.mark.parametrize("mode", ["format", "model"])
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_end_to_end_equals_the_oracle_on_the_decoded_images(hip, oracle, name, mode):
    A = hip
    left, right, opt = _cone()
    H, W = left.shape[:2]
    n = W * H
    frames = _frames(left, right, name)
    raw_l, raw_r = frames[0][0], frames[1][0]
    st, dev = _handle(A, W, H, opt), DeviceBuffers(A)
    try:
        rl, rr = _set_both(A, st, frames, W, H, mode)
        want = _final(oracle, rl, rr, opt)
        assert np.isfinite(want).mean() > 0.5
        assert np.array_equal(st.rectify(raw_l, 0), rl) and np.array_equal(st.rectify(raw_r, 1), rr)
        assert _same(st.match(raw_l, raw_r), want), "match"
        d = np.full((H, W), 7, F)
        assert st.match_async(raw_l, raw_r, d) and st.wait() and _same(d, want), "match_async"
        dl, dr, dd = dev.new(raw_l), dev.new(raw_r), dev.alloc(4 * n + GUARD, POISON)
        assert st.match_device(dl, dr, dd) and st.wait(), A.last_error()
        got = dev.get(dd, 4 * n + GUARD, np.uint8)
        assert _same(got[:4 * n].view(F).reshape(H, W), want) and np.all(got[4 * n:] == POISON), "match_device"
        assert np.array_equal(dev.get(dl, raw_l.shape, np.uint8), raw_l), "the caller's frame was written"
        # the cloud's colours are those of the decoded left image
        d, z, pts, g = st.match_out(raw_l, raw_r, CONE_CALIB, depth=True, cloud=True, disp8=True)
        assert _same(d, want), "match_out"
        _check_outputs(name + " match_out", want, rl, CONE_CALIB, z, pts, st.cloud_count(), g)
        farm = A.PairFarm(W, H, cases.to_product_option(opt), device=0, pipelines=2)
        try:
            _set_both(A, farm, frames, W, H, mode)
            outs = [np.zeros((H, W), F) for _ in range(3)]
            for o in outs:
                farm.submit(raw_l, raw_r, o)
            with pytest.raises(RuntimeError):  # refused while a pair is in flight
                farm.set_input_format(0, A.RawFormat(W, H, 0, A.PIX_BGR8))
            assert "in flight" in A.last_error()
            farm.drain()
            assert all(_same(o, want) for o in outs), "farm"
            farm.clear_rectify()
            farm.submit(rl, rr, outs[0])
            farm.drain()
            assert _same(outs[0], want), "farm, off again"
        finally:
            farm.close()
        st.clear_rectify()
        assert _same(st.match(rl, rr), want), "after clear_rectify"
    finally:
        dev.free()
        st.Release()


def test_bgr8_through_set_input_format_equals_a_plain_match(hip):
    """BGR8 (left, padded pitch) and RGB8 (right) through the conversion: the plain Match of the same pixels; and one side converting,
    the other one through maps."""
    A = hip
    left, right, opt = _cone()
    H, W = left.shape[:2]
    st, dev = _handle(A, W, H, opt), DeviceBuffers(A)
    try:
        want = st.match(left, right)
        fl, fr = A.RawFormat(W, H, W * 3 + 5, A.PIX_BGR8), A.RawFormat(W, H, 0, A.PIX_RGB8)
        raw_l, raw_r = RR.pack_source(left, RR.BGR8, W * 3 + 5), RR.pack_source(right, RR.RGB8)
        st.set_input_format(0, fl)
        st.set_input_format(1, fr)
        assert _same(st.match(raw_l, raw_r), want)
        dl, dr, dd = dev.new(raw_l), dev.new(raw_r), dev.alloc(4 * W * H, POISON)
        assert st.match_device(dl, dr, dd) and st.wait() and _same(dev.get(dd, (H, W), F), want)
        m = RR.identity_model(cx=W / 2.0, cy=H / 2.0)  # the right side through the identity maps instead: the same image
        st.set_rectify_model(1, fr, A.CameraModel(**m))
        assert st.rectify_maps(1)[2].all() and _same(st.match(raw_l, raw_r), want)
        st.clear_rectify()
        assert _same(st.match(left, right), want)
    finally:
        dev.free()
        st.Release()


# ---------------------------------------------------------------------------------------------- redo paths
def _match_all(st, left, right):
    d, z, pts, g = st.match_out(left, right, CONE_CALIB, depth=True, cloud=True, disp8=True)
    return d, z, pts, st.cloud_count(), g


def _check_all(what, got, want, rect_left):
    d, z, pts, count, g = got
    assert _same(d, want), what + ": the map differs"
    _check_outputs(what, want, rect_left, CONE_CALIB, z, pts, count, g)


def _warped(left, right, fmts, pads, grow):
    """The pair warped under second_model into frames of another (even) size, packed into the given layouts"""
    H, W = left.shape[:2]
    out = []
    for img, fmt, pad, (gw, gh) in zip((left, right), fmts, pads, grow):
        ws, hs = W + gw, H + gh
        mx, my = RR.model_maps(RR.second_model(W, H, ws, hs), ws, hs)
        frame = RR.remap(img, W, H, W * 3, RR.BGR8, mx, my)[0]
        pitch = _pitch(fmt, ws, pad)
        out.append((RF.pack(frame, fmt, pitch), (ws, hs, pitch, fmt)))
    return out


def _set_example(A, st, raws, W, H):
    want = []
    for side, (raw, (ws, hs, pitch, fmt)) in enumerate(raws):
        m = RR.example_model(ws, hs, W, H)
        st.set_rectify_model(side, A.RawFormat(ws, hs, pitch, fmt), A.CameraModel(**m))
        want.append(RF.remap(raw, ws, hs, pitch, fmt, 0, *RR.model_maps(m, W, H))[0])
    return want


def test_redo_paths_with_a_bayer_side(hip, monkeypatch):
    """The sequence of tests/test_gpu_rectify.py::test_redo_paths_with_rectification_on with a Bayer left side (and the noise pair
    through the conversion alone): the aggregation ring redo (counter 2) or the scanline seam redo (counter 4), the continued voting
    chain (counter 1), the median fallback in both forms (counter 0).  The counters show each path was taken."""
    A = hip
    w, h, d = 256, 160, 64
    opt = pyoracle.Option(max_disparity=d)
    s_pair = workloads.structured_pair(w, h, d, seed=41)
    n_pair = workloads.noise_pair(w, h, seed=42)
    monkeypatch.setenv("ADC_AGG_DUAL", "0")
    plain = _handle(A, w, h, opt)
    s_raw = _warped(*s_pair, (RF.BAYER_GRBG8, RF.GRAY8), (3, 0), ((20, 12), (20, 12)))
    st = _handle(A, w, h, opt)

    def noise_on():  # raw == rectified: keeps the short arms that make the next pair's ring too shallow
        for side in (0, 1):
            st.set_input_format(side, A.RawFormat(w, h, 0, A.PIX_BGR8))

    try:
        s_rect = _set_example(A, st, s_raw, w, h)
        want_s, want_n = plain.match(*s_rect), plain.match(*n_pair)
        s_in = (s_raw[0][0], s_raw[1][0])
        _check_all("structured, first", _match_all(st, *s_in), want_s, s_rect[0])
        noise_on()
        _check_all("noise", _match_all(st, *n_pair), want_n, n_pair[0])
        _check_all("noise, small ring assumed", _match_all(st, *n_pair), want_n, n_pair[0])
        _set_example(A, st, s_raw, w, h)
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
    raws = _warped(*pair, (RF.pix_bits(RF.BAYER_BGGR16, 12), RF.NV12), (0, 7), ((-16, 10), (24, -8)))
    plain, st, dev = _handle(A, w, h, opt), _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        rect = _set_example(A, st, raws, w, h)
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


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_on_a_real_handle(hip):
    """One side set alone; a geometry other than the handle's; an odd device address with a 16-bit layout; a set call while a Match is
    pending; the argument rules with their messages.  The handle stays exact."""
    A = hip
    L = A.lib()
    w, h, d = 96, 40, 16
    left, right = workloads.structured_pair(w, h, d, seed=3)
    n = w * h
    st, dev = _handle(A, w, h, pyoracle.Option(max_disparity=d)), DeviceBuffers(A)
    try:
        want = st.match(left, right)
        bgr = A.RawFormat(w, h, 0, A.PIX_BGR8)
        out = np.full((h, w), 7, F)
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n, POISON)
        lp, rp, op = np.ascontiguousarray(left).ctypes.data, np.ascontiguousarray(right).ctypes.data, out.ctypes.data
        # one side alone
        st.set_input_format(A.SIDE_LEFT, A.RawFormat(w, h, 0, A.PIX_BAYER_RGGB8))
        for rc in (L.adc_match(st._h, lp, rp, op), L.adc_match_async(st._h, lp, rp, op), L.adc_match_device(st._h, dl, dr, dd)):
            assert rc == 1 and "one side only" in A.last_error(), (rc, A.last_error())
        assert (out == 7).all() and np.all(dev.get(dd, 4 * n, np.uint8) == POISON) and st.wait()
        st.clear_rectify()
        assert _same(st.match(left, right), want)
        # another geometry, and the argument rules, with their messages; the state is untouched
        for bad, word in ((A.RawFormat(w + 2, h, 0, A.PIX_BGR8), "handle"), (A.RawFormat(w, h - 2, 0, A.PIX_NV12), "handle"),
                          (A.RawFormat(w, h, 0, 9), "format"), (A.RawFormat(w, h, 0, 0x24), "format"), (A.RawFormat(w, h, w * 3, A.pix_bits(A.PIX_BGR8, 10)), "bits"),
                          (A.RawFormat(w, h, 2 * w, A.pix_bits(A.PIX_GRAY16, 8)), "bits"), (A.RawFormat(w, h, 2 * w + 1, A.PIX_GRAY16), "even"),
                          (A.RawFormat(w, h, w - 1, A.PIX_NV12), "pitch"), (A.RawFormat(w, h, 2 * w - 1, A.PIX_YUYV), "pitch")):
            assert L.adc_set_input_format(st._h, 0, C.byref(bad)) == 1 and word in A.last_error(), (word, A.last_error())
        assert L.adc_set_input_format(st._h, 2, C.byref(bgr)) == 1 and "side" in A.last_error()
        assert _same(st.match(left, right), want)
        # an odd device address with a 16-bit layout: refused at the call that receives it
        g16 = A.RawFormat(w, h, 0, A.pix_bits(A.PIX_GRAY16, 12))
        st.set_input_format(0, g16)
        st.set_input_format(1, bgr)
        raw = RF.pack(left, g16.format)
        want16 = st.match(raw, right)
        assert not _same(want16, want)
        p16 = dev.alloc(raw.nbytes + 2)
        dev.put(p16, raw)
        assert L.adc_match_device(st._h, p16 + 1, dr, dd) == 1 and "even" in A.last_error()
        assert L.adc_rectify_device(st._h, 0, p16 + 1, dd) == 1 and "even" in A.last_error()
        assert np.all(dev.get(dd, 4 * n, np.uint8) == POISON)
        assert st.match_device(p16, dr, dd) and st.wait() and _same(dev.get(dd, (h, w), F), want16)
        # while a Match is pending
        assert st.match_device(p16, dr, dd)
        assert L.adc_set_input_format(st._h, 0, C.byref(bgr)) == 1 and "pending" in A.last_error()
        assert st.wait() and _same(dev.get(dd, (h, w), F), want16)
        st.clear_rectify()
        assert _same(st.match(left, right), want)
    finally:
        dev.free()
        st.Release()


# ---------------------------------------------------------------------------------------------- the CLI
def test_cli_raw_nv12(hip, oracle, tmp_path):
    """adcensus_cli --raw NV12,450,374,PITCH on Cone written as NV12 frames: <out>.pfm is the oracle's Match on the decoded images."""
    from PIL import Image
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    left, right, opt = _cone()
    H, W = left.shape[:2]
    pitch = W + 14
    frames = [RF.pack(img, RF.NV12, pitch) for img in (left, right)]
    dec = [RF.decode(f, W, H, pitch, RF.NV12).astype(np.uint8) for f in frames]
    want = _final(oracle, dec[0], dec[1], opt)
    for name, f in zip(("l.nv12", "r.nv12"), frames):
        f.tofile(tmp_path / name)
    r = subprocess.run([cli, str(tmp_path / "l.nv12"), str(tmp_path / "r.nv12"), "0", "64", str(tmp_path / "out"), "--raw", "NV12,%d,%d,%d" % (W, H, pitch)],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, ADC_VERBOSE="0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert _same(read_pfm(str(tmp_path / "out") + ".pfm"), want)
    assert np.array_equal(np.array(Image.open(str(tmp_path / "out") + "-rect-left.png"))[:, :, ::-1], dec[0])


# ---------------------------------------------------------------------------------------------- failing HIP calls
def test_hip_failures_on_the_rawfmt_paths(hip):
    """The fault-injection build (the n-th HIP call returns an error on the host, nothing on the device misbehaves): every HIP call of
    the two adc_set_input_format calls' first use + a converting adc_match, of a converting adc_match_device + adc_wait and of
    adc_rectify_device + adc_wait on such a side fails once -- the call reports it, the same handle is exact afterwards, nothing
    leaks.  tests/rawfmt_fault_probe.py runs in its own interpreter."""
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rawfmt_fault_probe.py")], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([l for l in r.stdout.splitlines() if l.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])
    print(o)
    # first use of a side: its raw buffer and the raw staging; the other side: its raw buffer, and the staging again (it was sized for two
    # frames of the first side, and an NV12 frame is larger than a Bayer one); a side again: none.  A converting Match: two launches on
    # top of the plain one
    assert (o["set_first_calls"], o["set_other_calls"], o["set_again_calls"]) == (2, 2, 0), o
    assert o["conv_calls"] == o["plain_calls"] + 2 and o["device_calls"] == o["device_plain_calls"] + 2 and o["convert_calls"] >= 2, o
    for name in ("host", "device", "convert"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert abs(o["host_leak_bytes"]) <= (2 << 20) and abs(o["final_leak_bytes"]) <= (2 << 20), o
