"""GPU tier: the left-view winner of the last scanline pass (SO_WTA, k_scanline.hip) -- the production form of the stage
(ADC_RUN_SCANLINE with +100) on volumes written with adc_debug_write: DISP_LEFT and VOLUME_A, bit for bit.

The oracle has no entry that starts at a cost volume (oracle/oracle_abi.h: it runs from images, or from a disparity map on), so the
expected values come from the sequential CPU restatements of the reference's scanline pass and of ADCensusStereo::ComputeDisparity
in tests/emul/emul.cpp (emul_scanline_pass, per disparity and without lanes, and emul_wta), which tests/test_emul.py pins to the
oracle's own dumps bit for bit.

Shapes: column paths of 1, 2, 63, 64, 65 and 129 elements at W = 8 (the winners are parked 64 to a flush); D = 33 and 64 (one
disparity per lane, with and without padding lanes), 100 and 128 (two per lane), 200 (four: the wide kernel); [-6, 58) and
[5, 105) with min_disparity != 0; 1030 x 20 for the kernel of passes with at least 1024 paths.  Volumes: two equal minima per
pixel under zero penalties (every final cost is (cost + path minimum) / 2, so the ties survive all four passes) -- inside one lane
and across lanes; the minimum at d = 0 and at d = D - 1; Large_Float everywhere (nothing below it: best stays 0)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from tests import cases

pytestmark = pytest.mark.gpu

F = np.float32
LARGE = F(99999.0)
PATHS = (1, 2, 63, 64, 65, 129)


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def lanes_of(d):
    """disparities per lane of the scanline kernels"""
    return 1 if d <= 64 else (2 if d <= 128 else 4)


def images(w, h, seed):
    rng = np.random.default_rng(seed)
    return ((rng.integers(0, 6, (h, w, 3)) * 40).astype(np.uint8) for _ in range(2))


def tie_volume(w, h, d, seed):
    """random costs in [20, 60) (multiples of 1/8), and per pixel the value 3 + k / 8 at two disparities: even pixels inside one lane
    where a lane holds more than one disparity, odd pixels in two different lanes"""
    rng = np.random.default_rng(seed)
    vpl = lanes_of(d)
    vol = (F(20) + rng.integers(0, 320, (h, w, d)).astype(F) / F(8)).astype(F)
    for y in range(h):
        for x in range(w):
            v = F(3) + F(rng.integers(0, 8)) / F(8)
            if vpl > 1 and (x + y) % 2 == 0:
                lane = int(rng.integers(0, (d - 1) // vpl))  # (a lane that is full: lane * vpl + vpl - 1 < d)
                a, b = sorted(int(k) for k in rng.choice(vpl, 2, replace=False))
                d1, d2 = lane * vpl + a, lane * vpl + b
            else:
                l1, l2 = sorted(int(k) for k in rng.choice((d + vpl - 1) // vpl, 2, replace=False))
                d1, d2 = l1 * vpl + int(rng.integers(0, vpl)), min(d - 1, l2 * vpl + int(rng.integers(0, vpl)))
            vol[y, x, d1] = vol[y, x, d2] = v
    return vol


def edge_volume(w, h, d, seed):
    """the minimum (0.0 against costs of at least 20) at d = 0 on even pixels, at d = D - 1 on odd ones"""
    rng = np.random.default_rng(seed)
    vol = (F(20) + rng.integers(0, 320, (h, w, d)).astype(F) / F(8)).astype(F)
    even = (np.add.outer(np.arange(h), np.arange(w)) % 2) == 0
    vol[even, 0] = 0
    vol[~even, d - 1] = 0
    return vol


def expected(emul, vol, left, right, opt):
    h, w, d = vol.shape
    lh, lv, rh, rv = (np.zeros((h, w), np.uint8) for _ in range(4))
    emul.emul_color_diffs(P(left), P(lh), P(lv), w, h)
    emul.emul_color_diffs(P(right), P(rh), P(rv), w, h)
    a, b = vol.copy(), np.empty_like(vol)
    for vert, direction in ((0, 1), (0, -1), (1, 1), (1, -1)):
        emul.emul_scanline_pass(P(a), P(b), P(lv if vert else lh), P(rv if vert else rh), w, h, opt.min_disparity, d, vert, direction,
                                opt.so_tso, C.c_float(opt.so_p1), C.c_float(opt.so_p2))
        a, b = b, a
    disp = np.empty((h, w), F)
    emul.emul_wta(P(a), P(disp), w, h, opt.min_disparity, d, 0)
    return a, disp


def tie_counts(final):
    """(pixels whose two lowest equal minima share a lane, pixels whose two lowest lie in different lanes)"""
    vpl = lanes_of(final.shape[2])
    inside = across = 0
    for row in final.reshape(-1, final.shape[2]):
        at = np.flatnonzero(row == row.min())
        if len(at) >= 2:
            if at[0] // vpl == at[1] // vpl:
                inside += 1
            else:
                across += 1
    return inside, across


class Stage:
    def __init__(self, A, w, h, opt, left, right):
        self.A, self.st = A, A.ADCensusStereo(device=0)
        if not self.st.Initialize(w, h, cases.to_product_option(opt)):
            raise RuntimeError("Initialize failed: " + A.last_error())
        self.st.debug_set_images(left, right)
        self.st.debug_run(A.RUN_GRAY_CENSUS)
        self.st.debug_run(A.RUN_ARMS)  # (the colour-step maps of the penalties)

    def run(self, vol):
        A, st = self.A, self.st
        for attempt in range(2):
            st.debug_write(A.BUF_VOLUME_A, vol)
            st.debug_write(A.BUF_DISP_LEFT, np.full(vol.shape[:2], -7.0, F))
            try:
                st.debug_run(A.RUN_SCANLINE, 104)
                break
            except RuntimeError as exc:  # a failed seam of speculative row segments: the handle runs whole rows from here on
                if "seam check" not in str(exc) or attempt:
                    raise
        return st.debug_read(A.BUF_VOLUME_A), st.debug_read(A.BUF_DISP_LEFT)


def compare(A, emul, w, h, opt, volumes, seed):
    left, right = images(w, h, seed)
    bad = []
    stage = Stage(A, w, h, opt, left, right)
    try:
        for name, vol in volumes:
            want_vol, want_disp = expected(emul, vol, left, right, opt)
            got_vol, got_disp = stage.run(vol)
            nv = int((got_vol.view(np.uint32) != want_vol.view(np.uint32)).sum())
            nd = int((got_disp.view(np.uint32) != want_disp.view(np.uint32)).sum())
            if nv or nd:
                bad.append("%dx%d [%d, %d) %s: %d costs, %d disparities differ" % (w, h, opt.min_disparity, opt.max_disparity, name, nv, nd))
    finally:
        stage.st.Release()
    return bad


@pytest.mark.parametrize("d", (33, 64, 100, 128, 200))
def test_ties_under_zero_penalties(hip, emul, d):
    opt = pyoracle.Option(max_disparity=d, so_p1=0.0, so_p2=0.0)
    bad, inside, across = [], 0, 0
    for h in PATHS:
        vol = tie_volume(8, h, d, seed=d * 1000 + h)
        left, right = images(8, h, seed=h)
        final, _ = expected(emul, vol, left, right, opt)
        i, a = tie_counts(final)
        inside, across = inside + i, across + a
        bad += compare(hip, emul, 8, h, opt, [("ties", vol)], seed=h)
    # the condition of the inputs, on the expected final volumes themselves: otherwise the comparison proves nothing
    assert across >= 100 and (lanes_of(d) == 1 or inside >= 100), (inside, across)
    assert not bad, bad


@pytest.mark.parametrize("d", (33, 64, 100, 128, 200))
def test_minima_at_the_ends_and_nothing_below_large_float(hip, emul, d):
    opt = pyoracle.Option(max_disparity=d)
    bad = []
    for h in PATHS:
        vols = [("ends", edge_volume(8, h, d, seed=d + h)), ("large", np.full((h, 8, d), LARGE, F))]
        bad += compare(hip, emul, 8, h, opt, vols, seed=100 + h)
    assert not bad, bad


@pytest.mark.parametrize("dmin,dmax", ((-6, 58), (5, 105)))
def test_ranges_that_do_not_start_at_zero(hip, emul, dmin, dmax):
    d = dmax - dmin
    bad = []
    for h in (2, 65, 129):
        zero = pyoracle.Option(min_disparity=dmin, max_disparity=dmax, so_p1=0.0, so_p2=0.0)
        bad += compare(hip, emul, 8, h, zero, [("ties", tie_volume(8, h, d, seed=7 * h + d))], seed=200 + h)
        opt = pyoracle.Option(min_disparity=dmin, max_disparity=dmax)
        vols = [("ends", edge_volume(8, h, d, seed=d + h)), ("large", np.full((h, 8, d), LARGE, F)), ("ties", tie_volume(8, h, d, seed=9 * h + d))]
        bad += compare(hip, emul, 8, h, opt, vols, seed=300 + h)
    assert not bad, bad


def test_more_than_1024_column_paths(hip, emul):
    """1030 columns: the last pass runs the kernel of passes that fill the chip (compiler-allocated prefetch slots)"""
    w, h, d = 1030, 20, 128
    zero = pyoracle.Option(max_disparity=d, so_p1=0.0, so_p2=0.0)
    vol = tie_volume(w, h, d, seed=5)
    left, right = images(w, h, seed=400)
    inside, across = tie_counts(expected(emul, vol, left, right, zero)[0])
    assert inside >= 100 and across >= 100
    bad = compare(hip, emul, w, h, zero, [("ties", vol)], seed=400)
    bad += compare(hip, emul, w, h, pyoracle.Option(max_disparity=d), [("ends", edge_volume(w, h, d, seed=6)), ("ties", vol)], seed=401)
    assert not bad, bad
