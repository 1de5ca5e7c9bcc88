"""GPU tier: the provenance and confidence maps of adc_match_ex / adc_match_device_ex against tests/extras_ref.py on the oracle's
stage dumps, bit for bit (uint32 view for floats, equality for codes) -- on every disparity-per-lane width, with and without LR
check / filling / discontinuity adjustment, through every redo adc_wait can take, at KITTI size and at 1080p, and from the CLI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases, extras_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["s2_96x64_d32", "cone", "cone_neg", "cone_pos", "cone_nolr", "cone_nofill", "cone_dda", "q_9x20_d8", "q_3x3_d2",
         "noise_160x90_d128", "s2_200x120_d200", "noise_80x40_d520", "s2_80x20_d2047"]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_u32(a), _u32(b))


def _expect(oracle, left, right, opt):
    o = oracle.run(left, right, opt, stages=extras_ref.STAGES)
    prov, conf = extras_ref.extras(o, opt)
    return o["disp_final"], prov, conf


def _check(got, want, what):
    d, p, c = got
    wd, wp, wc = want
    assert _same(d, wd), "%s: disparity differs on %d pixels" % (what, int((_u32(d) != _u32(wd)).sum()))
    assert np.array_equal(p, wp), "%s: provenance differs on %d pixels" % (what, int((p != wp).sum()))
    assert _same(c, wc), "%s: confidence differs on %d pixels" % (what, int((_u32(c) != _u32(wc)).sum()))


def _handle(A, w, h, opt):
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt)), A.last_error()
    return st


def _d3_pair():
    left, right = workloads.structured_pair(64, 40, 3, seed=61)
    return left, right, pyoracle.Option(max_disparity=3)


@pytest.mark.parametrize("name", CASES + ["d3_64x40"])
def test_match_ex_equals_reference(hip, oracle, name):
    """disparity == disp_final, provenance and confidence == extras_ref; each map alone equals its part of the pair; a plain Match
    on the same handle afterwards is undisturbed."""
    A = hip
    left, right, opt = _d3_pair() if name == "d3_64x40" else cases.make_case(name)
    h, w = left.shape[:2]
    want = _expect(oracle, left, right, opt)
    st = _handle(A, w, h, opt)
    try:
        _check(st.match_ex(left, right), want, name)
        d, p = np.empty((h, w), np.float32), np.empty((h, w), np.uint8)
        assert st.MatchEx(left, right, d, p, None)
        assert _same(d, want[0]) and np.array_equal(p, want[1]), name + ": provenance alone"
        d, c = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
        assert st.MatchEx(left, right, d, None, c)
        assert _same(d, want[0]) and _same(c, want[2]), name + ": confidence alone"
        assert _same(st.match(left, right), want[0]), name + ": plain Match after MatchEx"
        # the codes are what the definition allows: lr in 0..2, fill 0 only with lr 0, confidence in [0, 1]
        p = want[1]
        assert np.all((p & A.PROV_LR_MASK) <= 2) and not np.any(((p >> A.PROV_FILL_SHIFT) == A.FILL_WTA) & ((p & A.PROV_LR_MASK) != 0))
        assert np.all((want[2] >= 0) & (want[2] <= 1))
    finally:
        st.Release()


def test_reset_and_device_entry_point(hip, oracle):
    """Reset to another geometry and back (the lazily allocated scratch follows the handle), then match_device_ex into
    adc_device_malloc buffers + wait: the same maps."""
    A = hip
    L = A.lib()
    l1, r1, o1 = cases.make_case("s2_96x64_d32")
    l2, r2, o2 = cases.make_case("noise_160x90_d128")
    want1, want2 = _expect(oracle, l1, r1, o1), _expect(oracle, l2, r2, o2)
    st = _handle(A, 96, 64, o1)
    bufs = []
    try:
        _check(st.match_ex(l1, r1), want1, "first geometry")
        assert st.Reset(160, 90, cases.to_product_option(o2))
        _check(st.match_ex(l2, r2), want2, "after Reset")
        assert st.Reset(96, 64, cases.to_product_option(o1))
        _check(st.match_ex(l1, r1), want1, "back again")
        assert st.Reset(160, 90, cases.to_product_option(o2))
        h, w = l2.shape[:2]
        n = w * h
        for size in (3 * n, 3 * n, 4 * n, n, 4 * n):
            bufs.append(L.adc_device_malloc(size))
            assert bufs[-1]
        dl, dr, dd, dp, dc = bufs
        assert L.adc_memcpy_h2d(dl, np.ascontiguousarray(l2).ctypes.data, 3 * n) == 0
        assert L.adc_memcpy_h2d(dr, np.ascontiguousarray(r2).ctypes.data, 3 * n) == 0
        for rep in range(2):
            assert st.match_device_ex(dl, dr, dd, dp, dc) and st.wait(), A.last_error()
            d, p, c = np.empty((h, w), np.float32), np.empty((h, w), np.uint8), np.empty((h, w), np.float32)
            assert L.adc_memcpy_d2h(d.ctypes.data, dd, 4 * n) == 0 and L.adc_memcpy_d2h(p.ctypes.data, dp, n) == 0
            assert L.adc_memcpy_d2h(c.ctypes.data, dc, 4 * n) == 0
            _check((d, p, c), want2, "match_device_ex %d" % rep)
        # only the confidence, into the same buffers; then a plain match_device
        assert st.match_device_ex(dl, dr, dd, None, dc) and st.wait()
        c = np.empty((h, w), np.float32)
        assert L.adc_memcpy_d2h(c.ctypes.data, dc, 4 * n) == 0 and _same(c, want2[2])
        assert st.match_device(dl, dr, dd) and st.wait()
        d = np.empty((h, w), np.float32)
        assert L.adc_memcpy_d2h(d.ctypes.data, dd, 4 * n) == 0 and _same(d, want2[0])
    finally:
        st.Release()
        for b in bufs:
            L.adc_device_free(b)


def test_redo_paths_keep_the_maps_exact(hip, oracle, monkeypatch):
    """The sequence of test_gpu_api.test_async_pipeline_assumptions_and_budgets with match_ex: an aggregation redo (the small ring
    assumed for a long-arm image, debug counter 2) and a continued voting chain (budget of 4 kernels, counter 1) -- the maps come
    from the redone stages."""
    A = hip
    w, h, d = 256, 160, 64
    opt = pyoracle.Option(max_disparity=d)
    s_pair = workloads.structured_pair(w, h, d, seed=41)
    n_pair = workloads.noise_pair(w, h, seed=42)
    want_s, want_n = _expect(oracle, *s_pair, opt), _expect(oracle, *n_pair, opt)
    monkeypatch.setenv("ADC_AGG_DUAL", "0")
    st = _handle(A, w, h, opt)
    try:
        _check(st.match_ex(*s_pair), want_s, "structured, first")
        _check(st.match_ex(*n_pair), want_n, "noise")
        _check(st.match_ex(*n_pair), want_n, "noise, small ring assumed")
        redo0 = st.debug_counter(2)
        _check(st.match_ex(*s_pair), want_s, "structured, aggregation redo")
        assert st.debug_counter(2) == redo0 + 1, "the aggregation redo path was not taken"
    finally:
        st.Release()
    st = _handle(A, w, h, opt)
    try:
        _check(st.match_ex(*s_pair), want_s, "structured, new handle")
        st.debug_set_budget(4)
        over = st.debug_counter(1)
        _check(st.match_ex(*s_pair), want_s, "structured, voting chain continued")
        assert st.debug_counter(1) == over + 1, "the voting continuation path was not taken"
    finally:
        st.Release()


def test_scanline_seam_redo_keeps_the_maps_exact(hip):
    """A forced scanline seam failure (3 segments per row with a 16-step warm-up): adc_wait redoes the Match with whole rows
    (counter 4) and the maps follow.  The switches are read once per process: own interpreter."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "import adcensus_amd as A\n"
            "from tests import cases, extras_ref\n"
            "from oracle import pyoracle\n"
            "l, r, opt = cases.make_case('s2_320x180_d128')\n"
            "o = pyoracle.load('auto').run(l, r, opt, stages=extras_ref.STAGES)\n"
            "wp, wc = extras_ref.extras(o, opt)\n"
            "st = A.ADCensusStereo(device=0)\n"
            "assert st.Initialize(l.shape[1], l.shape[0], cases.to_product_option(opt))\n"
            "bad = []\n"
            "for rep in range(3):\n"
            "    d, p, c = st.match_ex(l, r)\n"
            "    if not np.array_equal(d.view(np.uint32), o['disp_final'].view(np.uint32)): bad.append('disp%%d' %% rep)\n"
            "    if not np.array_equal(p, wp): bad.append('prov%%d' %% rep)\n"
            "    if not np.array_equal(c.view(np.uint32), wc.view(np.uint32)): bad.append('conf%%d' %% rep)\n"
            "redos = st.debug_counter(4)\n"
            "st.Release()\n"
            "print('BAD', bad, 'REDOS', redos)\n"
            "sys.exit(1 if bad else (2 if redos == 0 else 0))\n") % ROOT
    env = dict(os.environ, ADC_SO_SEG="3", ADC_SO_WARM="16")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]


def test_paper_modes_refuse_the_maps(hip):
    """With paper modes set the maps are not defined: MatchEx / match_device_ex return 1 with a message, the handle still matches."""
    A = hip
    left, right, opt = cases.make_case("s2_96x64_d32")
    h, w = left.shape[:2]
    st = _handle(A, w, h, opt)
    try:
        st.set_paper_modes(A.PAPER_SO_SUM)
        before = st.match(left, right)
        d, p, c = np.empty((h, w), np.float32), np.empty((h, w), np.uint8), np.empty((h, w), np.float32)
        L = A.lib()
        assert L.adc_match_ex(st._h, left.ctypes.data, right.ctypes.data, d.ctypes.data, p.ctypes.data, c.ctypes.data) == 1
        assert "paper" in A.last_error()
        assert L.adc_match_ex(st._h, left.ctypes.data, right.ctypes.data, d.ctypes.data, None, c.ctypes.data) == 1
        assert L.adc_match_device_ex(st._h, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), None) == 1
        assert _same(st.match(left, right), before)
        assert st.MatchEx(left, right, d, None, None) and _same(d, before)  # (no maps asked for: exactly Match)
    finally:
        st.Release()


@pytest.mark.parametrize("size", ["kitti_structured", "full_noise"])
def test_large_sizes(hip, oracle, size):
    """A KITTI-size structured pair (1242x375, D = 128) and the headline noise pair (1920x1080, D = 128, seed 12345)."""
    A = hip
    if size == "kitti_structured":
        w, h = 1242, 375
        left, right = workloads.structured_pair(w, h, 128, seed=4243)
    else:
        w, h = 1920, 1080
        left, right = workloads.noise_pair(w, h, 12345)
    opt = pyoracle.Option(max_disparity=128)
    want = _expect(oracle, left, right, opt)
    st = _handle(A, w, h, opt)
    try:
        _check(st.match_ex(left, right), want, size)
    finally:
        st.Release()


def test_cli_extras(hip, oracle, tmp_path):
    """adcensus_cli ... --extras on cone: <out>-prov.png (raw codes), <out>-conf.png (uchar(conf * 255)), <out>-conf.pfm."""
    from PIL import Image
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    left, right, opt = cases.make_case("cone")
    h, w = left.shape[:2]
    _, wp, wc = _expect(oracle, left, right, opt)
    Image.fromarray(np.ascontiguousarray(left[:, :, ::-1])).save(tmp_path / "left.png")
    Image.fromarray(np.ascontiguousarray(right[:, :, ::-1])).save(tmp_path / "right.png")
    out = subprocess.run([cli, str(tmp_path / "left.png"), str(tmp_path / "right.png"), "0", "64", str(tmp_path / "out"), "--extras"],
                         capture_output=True, text=True, timeout=300, env=dict(os.environ, ADC_VERBOSE="0"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.array(Image.open(tmp_path / "out-prov.png")), wp)
    assert np.array_equal(np.array(Image.open(tmp_path / "out-conf.png")), (wc * np.float32(255)).astype(np.uint8))
    with open(tmp_path / "out-conf.pfm", "rb") as f:
        assert f.readline().strip() == b"Pf"
        assert f.readline().split() == [str(w).encode(), str(h).encode()]
        f.readline()
        got = np.ascontiguousarray(np.frombuffer(f.read(), dtype="<f4").reshape(h, w)[::-1])
    assert _same(got, wc)
