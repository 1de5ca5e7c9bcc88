"""GPU tier: the speckle filter (k_speckle.hip) against tests/speckle_ref.py, bit for bit -- maps through their uint32 view, labels
and statistics exactly: the kernels alone on the oracle's final maps and on the shapes that break naive connected-component
labelling (up to 1920x1080), the whole calls through every entry point, every redo adc_wait can take, refusals, large sizes, the
CLI, and every HIP call failing once."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases, outputs_ref
from tests.speckle_patterns import patterns
from tests.speckle_ref import largest, speckle_ref
from tests.test_gpu_outputs import CONE_CALIB, POISON, DeviceBuffers, _check_outputs, _final, _handle, _same, _u32
from tests.test_outputs_api import read_pfm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["cone", "cone_nofill", "cone_neg", "cone_pos", "piano", "q_3x3_d2", "q_9x20_d8", "q_1x40_d8", "q_40x1_d8", "noise_160x90_d128",
         "s2_80x20_d2047"]
CALL_CASES = ["cone", "cone_nofill", "cone_neg", "q_9x20_d8", "noise_160x90_d128", "s2_80x20_d2047"]
GUARD = 256  # poisoned bytes behind every buffer the kernels write
SIZE, DIFF = 100, 1.0


def _filter(A, st, dev, disp, max_size, max_diff, labels=True):
    """adc_filter_speckles_device on a host map: (filtered map, labels or None, stats); the label buffer is poisoned first, and the
    bytes behind both buffers must still be poison afterwards"""
    h, w = disp.shape
    n = w * h
    pd = dev.alloc(4 * n + GUARD, POISON)
    dev.put(pd, np.ascontiguousarray(disp, np.float32))
    pl = dev.alloc(4 * n + GUARD, POISON) if labels else None
    assert st.filter_speckles_device(pd, max_size, max_diff, pl), A.last_error()
    assert st.wait(), A.last_error()
    raw = dev.get(pd, 4 * n + GUARD, np.uint8)
    assert np.all(raw[4 * n:] == POISON), "written behind the map"
    got = raw[:4 * n].view(np.float32).reshape(h, w).copy()
    lab = None
    if labels:
        rawl = dev.get(pl, 4 * n + GUARD, np.uint8)
        assert np.all(rawl[4 * n:] == POISON), "written behind the labels"
        lab = rawl[:4 * n].view(np.int32).reshape(h, w).copy()
    stats = st.speckle_stats()
    dev.free()
    return got, lab, stats


def _check_filter(A, st, dev, what, disp, max_size, max_diff, labels=True):
    want = speckle_ref(disp, max_size, max_diff)
    got, lab, stats = _filter(A, st, dev, disp, max_size, max_diff, labels)
    assert _same(got, want[0]), "%s: map differs on %d pixels" % (what, int((_u32(got) != _u32(want[0])).sum()))
    if labels:
        assert np.array_equal(lab, want[1]), "%s: labels differ on %d pixels" % (what, int((lab != want[1]).sum()))
    assert stats == want[2], (what, stats, want[2])
    return want


@pytest.mark.parametrize("name", CASES)
def test_kernels_on_the_reference_maps(hip, oracle, name):
    """Stage-isolated: adc_filter_speckles_device on the ORACLE's disp_final."""
    A = hip
    left, right, opt = cases.make_case(name)
    h, w = left.shape[:2]
    disp = _final(oracle, left, right, opt)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        for max_size, max_diff in ((100, 1.0), (400, 1.0), (50, 0.5), (1, 0.0), (w * h, 1.0)):
            want = _check_filter(A, st, dev, "%s (%d, %g)" % (name, max_size, max_diff), disp, max_size, max_diff)
            if max_size == w * h:
                assert not np.isfinite(want[0]).any()  # everything removed
            _check_filter(A, st, dev, "%s (%d, %g) without labels" % (name, max_size, max_diff), disp, max_size, max_diff, labels=False)
        # labels only: the map keeps its bits
        got, lab, stats = _filter(A, st, dev, disp, 0, 1.0)
        want = speckle_ref(disp, 0, 1.0)
        assert _same(got, disp) and np.array_equal(lab, want[1]) and stats == want[2] and stats[1:] == (0, 0)
        if name == "cone":  # the figures of the numpy definition on Cone's reference map
            a, b, c = speckle_ref(disp, 100, 1.0), speckle_ref(disp, 400, 1.0), speckle_ref(disp, 50, 0.5)
            print("cone: valid", int(np.isfinite(disp).sum()), "(100, 1.0)", a[2], "largest", largest(a[1]), "(400, 1.0) removed px", b[2][2],
                  "(50, 0.5)", c[2])
            assert int(np.isfinite(disp).sum()) == 168750 and a[2] == (125, 91, 930) and largest(a[1]) == 54940
            assert b[2][2] == 6081 and (c[2][0], c[2][2]) == (302, 963)
        # the host convenience
        f, l = st.filter_speckles(disp, 100, 1.0, labels=True)
        want = speckle_ref(disp, 100, 1.0)
        assert _same(f, want[0]) and np.array_equal(l, want[1]) and st.speckle_stats() == want[2]
        assert _same(st.filter_speckles(disp, 100, 1.0), want[0])
    finally:
        dev.free()
        st.Release()


@pytest.mark.parametrize("size", [(333, 41), (130, 33), (64, 16), (1030, 5), (7, 300), (1, 70), (200, 1), (1920, 1080)])
def test_kernels_on_synthetic_maps(hip, size):
    """The shapes that break naive labelling (tests/speckle_patterns.py), at widths that are not multiples of 64 and at 1080p."""
    A = hip
    w, h = size
    st, dev = _handle(A, w, h, pyoracle.Option(max_disparity=16)), DeviceBuffers(A)
    try:
        for name, (disp, max_size, max_diff) in patterns(w, h).items():
            want = _check_filter(A, st, dev, "%s %dx%d" % (name, w, h), disp, max_size, max_diff)
            print("%s %dx%d (%d, %g): %s" % (name, w, h, max_size, max_diff, want[2]))
    finally:
        dev.free()
        st.Release()


@pytest.mark.parametrize("name", CALL_CASES)
def test_whole_calls_equal_reference(hip, oracle, name):
    """set_speckle_filter, then every entry point delivers speckle_ref(disp_final) and what follows from it; filter off again on
    the same handle: disp_final; a handle that never had the filter set: disp_final."""
    A = hip
    left, right, opt = cases.make_case(name)
    h, w = left.shape[:2]
    n = w * h
    want = _final(oracle, left, right, opt)
    want_f, _, want_stats = speckle_ref(want, SIZE, DIFF)
    removed = np.isfinite(want) & ~np.isfinite(want_f)
    assert int(removed.sum()) == want_stats[2]
    print(name, "stats", want_stats)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        d0, p0, c0 = st.match_ex(left, right)  # the parent's maps
        assert _same(d0, want)
        st.set_speckle_filter(SIZE, DIFF)
        assert _same(st.match(left, right), want_f), name + ": match"
        assert st.speckle_stats() == want_stats
        d = np.full((h, w), 7, np.float32)
        assert st.match_async(left, right, d) and st.wait() and _same(d, want_f), name + ": match_async"
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n, POISON)
        assert st.match_device(dl, dr, dd) and st.wait(), A.last_error()
        assert _same(dev.get(dd, (h, w), np.float32), want_f), name + ": match_device"
        assert st.speckle_stats() == want_stats
        # provenance: the parent's code | PROV_SPECKLE exactly on the removed pixels; confidence as computed
        d, p, c = st.match_ex(left, right)
        assert _same(d, want_f), name + ": match_ex"
        assert np.array_equal(p, np.where(removed, p0 | A.PROV_SPECKLE, p0)), name + ": provenance"
        assert _same(c, c0), name + ": confidence"
        pp, pc = dev.alloc(n, POISON), dev.alloc(4 * n, POISON)
        assert st.match_device_ex(dl, dr, dd, pp, pc) and st.wait(), A.last_error()
        assert _same(dev.get(dd, (h, w), np.float32), want_f)
        assert np.array_equal(dev.get(pp, (h, w), np.uint8), np.where(removed, p0 | A.PROV_SPECKLE, p0)) and _same(dev.get(pc, (h, w), np.float32), c0)
        # the outputs come from the filtered map
        for calib in (None, CONE_CALIB):
            d, z, pts, g = st.match_out(left, right, calib, depth=calib is not None, cloud=True, disp8=True)
            assert _same(d, want_f), name + ": match_out"
            _check_outputs("%s match_out calib=%s" % (name, calib), want_f, left, calib, z, pts, st.cloud_count(), g)
            if calib is None:
                assert st.cloud_count() == int(np.isfinite(want).sum()) - want_stats[2]
        pz, pcl, pn, pg = dev.alloc(4 * n), dev.alloc(16 * n), dev.alloc(16), dev.alloc(n)
        assert st.match_device_out(dl, dr, dd, CONE_CALIB, pz, pcl, n, pn, pg) and st.wait(), A.last_error()
        count = st.cloud_count()
        assert _same(dev.get(dd, (h, w), np.float32), want_f)
        _check_outputs(name + " match_device_out", want_f, left, CONE_CALIB, dev.get(pz, (h, w), np.float32), dev.get(pcl, count, A.POINT_DTYPE),
                       count, dev.get(pg, (h, w), np.uint8))
        # other parameters on the same handle, then off again
        st.set_speckle_filter(50, 0.5)
        assert _same(st.match(left, right), speckle_ref(want, 50, 0.5)[0])
        st.set_speckle_filter(0, 0.0)
        assert _same(st.match(left, right), want), name + ": filter off again"
        d, p, c = st.match_ex(left, right)
        assert _same(d, want) and np.array_equal(p, p0) and _same(c, c0)
        assert st.match_device(dl, dr, dd) and st.wait() and _same(dev.get(dd, (h, w), np.float32), want)
    finally:
        dev.free()
        st.Release()
    st = _handle(A, w, h, opt)
    try:
        assert _same(st.match(left, right), want), name + ": a handle that never had the filter set"
    finally:
        st.Release()
    # the farm
    farm = A.PairFarm(w, h, cases.to_product_option(opt), device=0, pipelines=2)
    try:
        farm.set_speckle_filter(SIZE, DIFF)
        outs = [np.zeros((h, w), np.float32) for _ in range(3)]
        for o in outs:
            farm.submit(left, right, o)
        with pytest.raises(RuntimeError):  # refused while a pair is in flight
            farm.set_speckle_filter(0, 0.0)
        assert "in flight" in A.last_error()
        farm.drain()
        assert all(_same(o, want_f) for o in outs), name + ": farm"
        farm.set_speckle_filter(0, 0.0)
        farm.submit(left, right, outs[0])
        farm.drain()
        assert _same(outs[0], want), name + ": farm, filter off again"
    finally:
        farm.close()


def _match_all(st, left, right, calib=CONE_CALIB):
    d, z, pts, g = st.match_out(left, right, calib, depth=True, cloud=True, disp8=True)
    return d, z, pts, st.cloud_count(), g, st.speckle_stats()


def _check_all(what, got, want_disp, left, calib=CONE_CALIB):
    d, z, pts, count, g, stats = got
    want_f, _, want_stats = speckle_ref(want_disp, SIZE, DIFF)
    assert _same(d, want_f), what + ": the filtered disparity differs on %d pixels" % int((_u32(d) != _u32(want_f)).sum())
    assert stats == want_stats, (what, stats, want_stats)
    _check_outputs(what, want_f, left, calib, z, pts, count, g)


def test_redo_paths_deliver_the_filtered_recomputed_map(hip, oracle, monkeypatch):
    """The sequence of tests/test_gpu_outputs.py::test_redo_paths_keep_the_outputs_exact with the filter on: the aggregation ring
    redo (counter 2), the continued voting chain (counter 1), the median fallback in both forms (counter 0).  The counters show
    the path was taken; the delivered map, its statistics and its outputs are those of the filtered recomputed map."""
    A = hip
    w, h, d = 256, 160, 64
    opt = pyoracle.Option(max_disparity=d)
    s_pair = workloads.structured_pair(w, h, d, seed=41)
    n_pair = workloads.noise_pair(w, h, seed=42)
    want_s, want_n = _final(oracle, *s_pair, opt), _final(oracle, *n_pair, opt)
    monkeypatch.setenv("ADC_AGG_DUAL", "0")
    st = _handle(A, w, h, opt)
    try:
        st.set_speckle_filter(SIZE, DIFF)
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
        st.set_speckle_filter(SIZE, DIFF)
        _check_all("structured, new handle", _match_all(st, *s_pair), want_s, s_pair[0])
        st.debug_set_budget(4)
        over = st.debug_counter(1)
        _check_all("structured, voting chain continued", _match_all(st, *s_pair), want_s, s_pair[0])
        assert st.debug_counter(1) == over + 1, "the voting continuation path was not taken"
        # ... and with the provenance map: the bit sits on the pixels removed from the RECOMPUTED map
        st.set_speckle_filter(0, 0.0)
        _, p0, c0 = st.match_ex(*s_pair)
        st.set_speckle_filter(SIZE, DIFF)
        st.debug_set_budget(4)
        over = st.debug_counter(1)
        dd, p, c = st.match_ex(*s_pair)
        assert st.debug_counter(1) == over + 1
        want_f = speckle_ref(want_s, SIZE, DIFF)[0]
        removed = np.isfinite(want_s) & ~np.isfinite(want_f)
        assert _same(dd, want_f) and np.array_equal(p, np.where(removed, p0 | A.PROV_SPECKLE, p0)) and _same(c, c0)
    finally:
        st.Release()
    # the median fallback: 330 rows = the banded filter with speculative bands; without filling, so that the map has holes
    w, h, d = 240, 330, 32
    left, right = workloads.structured_pair(w, h, d, seed=11)
    opt = pyoracle.Option(max_disparity=d, do_filling=0)
    want = _final(oracle, left, right, opt)
    assert np.isinf(want).any() and speckle_ref(want, SIZE, DIFF)[2][2] > 0
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        st.set_speckle_filter(SIZE, DIFF)
        _check_all("median, first", _match_all(st, left, right), want, left)
        for arg in (100, 101):
            fall = st.debug_counter(0)
            st.debug_run(A.RUN_MEDIAN, arg)
            _check_all("median fallback %d" % arg, _match_all(st, left, right), want, left)
            assert st.debug_counter(0) == fall + 1, "the median fallback path was not taken"
            fall = st.debug_counter(0)
            st.debug_run(A.RUN_MEDIAN, arg)
            dd, p, c = st.match_ex(left, right)
            assert st.debug_counter(0) == fall + 1 and _same(dd, speckle_ref(want, SIZE, DIFF)[0])
            assert np.array_equal((p & A.PROV_SPECKLE) != 0, np.isfinite(want) & ~np.isfinite(dd))
        n = w * h
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n, POISON)
        fall = st.debug_counter(0)
        st.debug_run(A.RUN_MEDIAN, 100)
        assert st.match_device(dl, dr, dd) and st.wait(), A.last_error()
        assert st.debug_counter(0) == fall + 1
        assert _same(dev.get(dd, (h, w), np.float32), speckle_ref(want, SIZE, DIFF)[0])
        st.set_speckle_filter(0, 0.0)
        assert _same(st.match(left, right), want)
    finally:
        dev.free()
        st.Release()


def test_refusals(hip, oracle):
    """NaN / negative / infinite max_diff, the setter with a Match pending, a NULL map: 1 with a message, nothing enqueued, the
    poisoned buffers untouched, a plain Match afterwards exact."""
    A = hip
    L = A.lib()
    left, right, opt = cases.make_case("q_9x20_d8")
    h, w = left.shape[:2]
    n = w * h
    want = _final(oracle, left, right, opt)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    farm = A.PairFarm(w, h, cases.to_product_option(opt), device=0, pipelines=1)
    try:
        pd, pl = dev.alloc(4 * n, POISON), dev.alloc(4 * n, POISON)
        for bad in (float("nan"), -1.0, -0.5, float("inf"), float("-inf")):
            assert L.adc_set_speckle_filter(st._h, 100, bad) == 1 and "max_diff" in A.last_error(), bad
            assert L.adc_filter_speckles_device(st._h, pd, 100, bad, pl) == 1 and "max_diff" in A.last_error(), bad
            assert L.adc_farm_set_speckle_filter(farm._f, 100, bad) == 1 and "max_diff" in A.last_error(), bad
            with pytest.raises(RuntimeError):
                st.set_speckle_filter(100, bad)
        assert L.adc_filter_speckles_device(st._h, None, 100, 1.0, pl) == 1 and "null map" in A.last_error()
        assert L.adc_filter_speckles_device(st._h, pd, 0, 1.0, None) == 0  # (nothing to do)
        assert st.wait()
        for p in (pd, pl):
            assert np.all(dev.get(p, 4 * n, np.uint8) == POISON)
        assert _same(st.match(left, right), want)  # the refused setters left the filter off
        # the setter while a Match is pending
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n, POISON)
        assert st.match_device(dl, dr, dd)
        assert L.adc_set_speckle_filter(st._h, 100, 1.0) == 1 and "pending" in A.last_error()
        assert st.wait() and _same(dev.get(dd, (h, w), np.float32), want)
        d = np.zeros((h, w), np.float32)
        assert st.match_async(left, right, d)
        assert L.adc_set_speckle_filter(st._h, 100, 1.0) == 1 and "pending" in A.last_error()
        assert st.wait() and _same(d, want)
        st.set_speckle_filter(100, 1.0)  # (accepted between Matches)
        assert st.match_device(dl, dr, dd)
        assert L.adc_set_speckle_filter(st._h, 0, 0.0) == 1  # switching it off is refused as well
        assert st.wait() and _same(dev.get(dd, (h, w), np.float32), speckle_ref(want, 100, 1.0)[0])
        st.set_speckle_filter(0, 0.0)
        assert _same(st.match(left, right), want)
    finally:
        farm.close()
        dev.free()
        st.Release()


@pytest.mark.parametrize("size", ["kitti_structured", "full_noise", "full_structured_nofill"])
def test_large_sizes(hip, oracle, size):
    """A KITTI-size structured pair (1242x375), the headline noise pair (1920x1080, seed 12345) and a 1080p structured pair without
    filling (holes), D = 128, parameters (200, 1.0): the filtered Match, its statistics, and the kernels alone with labels."""
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
    want_f, _, want_stats = speckle_ref(want, 200, 1.0)
    print(size, "valid", int(np.isfinite(want).sum()), "stats", want_stats)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        st.set_speckle_filter(200, 1.0)
        assert _same(st.match(left, right), want_f)
        assert st.speckle_stats() == want_stats
        d, _, pts, _ = st.match_out(left, right, None, cloud=True)
        assert _same(d, want_f)
        _check_outputs(size + ", cloud of the filtered map", want_f, left, None, None, pts, st.cloud_count(), None)
        _check_filter(A, st, dev, size + ", kernels alone", want, 200, 1.0)
        st.set_speckle_filter(0, 0.0)
        assert _same(st.match(left, right), want)
    finally:
        dev.free()
        st.Release()


def test_cli_speckle(hip, oracle, tmp_path):
    """adcensus_cli ... --speckle 100,1.0 on Cone: every file comes from the filtered map (.pfm equals speckle_ref, the cloud has
    valid - removed rows, the image is that of the filtered map); a run without the flag writes the unfiltered map."""
    from PIL import Image
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    left, right, opt = cases.make_case("cone")
    want = _final(oracle, left, right, opt)
    want_f, _, stats = speckle_ref(want, 100, 1.0)
    Image.fromarray(np.ascontiguousarray(left[:, :, ::-1])).save(tmp_path / "left.png")
    Image.fromarray(np.ascontiguousarray(right[:, :, ::-1])).save(tmp_path / "right.png")
    env = dict(os.environ, ADC_VERBOSE="0")
    for pref, extra in (("plain", []), ("spk", ["--speckle", "100,1.0"]), ("spkcal", ["--speckle", "100,1.0", "--calib", "3740,0.16,225,187.5,0"])):
        out = subprocess.run([cli, str(tmp_path / "left.png"), str(tmp_path / "right.png"), "0", "64", str(tmp_path / pref)] + extra,
                             capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
    assert _same(read_pfm(str(tmp_path / "plain") + ".pfm"), want)
    assert _same(read_pfm(str(tmp_path / "spk") + ".pfm"), want_f) and _same(read_pfm(str(tmp_path / "spkcal") + ".pfm"), want_f)
    rows = lambda p: sum(1 for _ in open(str(tmp_path / p) + "-cloud.txt"))  # noqa: E731
    assert rows("plain") == int(np.isfinite(want).sum()) and rows("spk") == rows("plain") - stats[2] == int(np.isfinite(want_f).sum())
    assert np.array_equal(np.array(Image.open(str(tmp_path / "spk") + "-d.png")), outputs_ref.disp8(want_f))
    assert np.array_equal(np.array(Image.open(str(tmp_path / "plain") + "-d.png")), outputs_ref.disp8(want))
    assert _same(read_pfm(str(tmp_path / "spkcal") + "-depth.pfm"), outputs_ref.outputs(want_f, left, CONE_CALIB)[0])


def test_hip_failures_on_the_speckle_paths(hip):
    """The fault-injection build: every HIP call of the setter's first use + a filtered adc_match, of a filtered adc_match_device +
    adc_wait and of adc_filter_speckles_device + adc_wait fails once -- the call reports it, the same handle is exact afterwards,
    nothing leaks.  tests/speckle_fault_probe.py runs in its own interpreter; only the existing injection hook is used."""
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "speckle_fault_probe.py")], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([l for l in r.stdout.splitlines() if l.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])
    print(o)
    # the hook sits on the new calls: two first-use allocations; four launches and the stats read-back per filtered Match
    assert o["setter_first_calls"] == 2 and o["setter_again_calls"] == 0, o
    assert o["filtered_calls"] >= o["plain_calls"] + 5 and o["device_calls"] >= o["device_plain_calls"] + 5 and o["filter_calls"] >= 5, o
    for name in ("host", "device", "filter"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert abs(o["host_leak_bytes"]) <= (2 << 20) and abs(o["final_leak_bytes"]) <= (2 << 20), o
