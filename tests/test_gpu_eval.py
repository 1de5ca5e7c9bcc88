"""GPU tier of the ground-truth evaluation (adc_set_ground_truth / adc_evaluate_device / adc_evaluate, k_eval.hip) against
tests/eval_ref.py, bit for bit: report words, echo, error map (uint32 view) and class map -- the kernels on the oracle's final maps of
Cone, Cloth3 and Wood2 with the committed ground truth in every format and occlusion source, with the provenance and confidence of
match_ex, on synthetic maps at the kernel's edges, the whole calls (device and host entry points, the CLI), every redo adc_wait can
take, the refusals on a real handle, "off means untouched", and the fault-injection build."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from adcensus_amd import evaluation, workloads
from oracle import pyoracle
from tests import cases, extras_ref
from tests import eval_ref as E
from tests.speckle_ref import speckle_ref
from tests.test_eval_api import load_gt, read_pfm
from tests.test_gpu_outputs import DeviceBuffers, _handle
from tests.test_gpu_rectify import PARENT_CALLS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
TS = [0.5, 1.0, 2.0, 4.0]
POISON = 0xA5


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(what, got, want, n_thresholds=None, echo=None):
    """got: (EvalReport, err, class) of a call; want: (report dict, err, class) of eval_ref.evaluate"""
    rep, err, cls = got
    wrep, werr, wcls = want
    words, wwords = rep.words(), E.to_words(wrep)
    diff = np.nonzero(words != wwords)[0]
    assert diff.size == 0, "%s: report words differ at %s: %s vs %s" % (what, diff[:8], words[diff[:8]], wwords[diff[:8]])
    if err is not None:
        assert np.array_equal(_u32(err), _u32(werr)), "%s: err differs on %d pixels" % (what, int((_u32(err) != _u32(werr)).sum()))
    if cls is not None:
        assert np.array_equal(cls, wcls), "%s: class differs on %d pixels" % (what, int((cls != wcls).sum()))
    if n_thresholds is not None:
        assert rep.n_thresholds == n_thresholds, what
    if echo is not None:
        assert (rep.has_right_gt, rep.has_nonocc_mask, rep.has_provenance, rep.has_confidence) == echo, what


_MAPS = {}


def _oracle_maps(oracle, name, **kw):
    """(final map, provenance, confidence) of the oracle for a named pair, computed once per session (Cloth3 and Wood2 take the CPU
    oracle half a minute each)"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _MAPS:
        left, right, opt = cases.make_case(name)
        for k, v in kw.items():
            setattr(opt, k, v)
        dump = oracle.run(left, right, opt, stages=extras_ref.STAGES)
        prov, conf = extras_ref.extras(dump, opt)
        _MAPS[key] = (dump["disp_final"], prov, conf)
    return _MAPS[key]


def _formats(A, raw8, scale):
    """the U8 fixture as the three formats, each with a row pitch of its own: (GroundTruth, decoded g)"""
    h, w = raw8.shape
    pad8 = np.full((h, w + 13), 77, np.uint8)
    pad8[:, :w] = raw8
    u16 = np.full((h, w + 3), 999, np.uint16)
    u16[:, :w] = raw8.astype(np.uint16) * 256  # (value * 256) / (scale * 256): the same quotient
    f32 = np.where(raw8 == 0, F(np.nan), raw8.astype(F)).astype(F)  # PFM style: unknown is not finite
    g = E.decode_gt(raw8, E.GT_U8, scale)
    assert np.array_equal(_u32(E.decode_gt(u16[:, :w], E.GT_U16, scale * 256)), _u32(g)) and np.array_equal(_u32(E.decode_gt(f32, E.GT_F32, scale)), _u32(g))
    return {"u8": A.GroundTruth(pad8[:, :w], scale), "u16": A.GroundTruth(u16[:, :w], scale * 256), "f32": A.GroundTruth(f32, scale)}, g


@pytest.mark.parametrize("name", ["cone", "cloth3", "wood2"])
def test_kernels_on_the_oracle_maps(hip, oracle, name):
    """The oracle's final map scored through the host entry point: three ground-truth formats x (right view, caller mask, neither)."""
    A = hip
    left, right, opt = cases.make_case(name)
    d = _oracle_maps(oracle, name)[0]
    raw_l, raw_r, scale = load_gt(name)
    h, w = d.shape
    st = _handle(A, w, h, opt)
    try:
        fl, g = _formats(A, raw_l, scale)
        fr, g_right = _formats(A, raw_r, scale)
        non = E.nonocc_from_right(g, g_right, 1.0)
        mask = (np.random.default_rng(3).random((h, w)) < 0.7).astype(np.uint8) * 200
        wants = {"right": E.evaluate(d, g, non, TS), "mask": E.evaluate(d, g, E.nonocc_from_mask(g, mask), TS), "none": E.evaluate(d, g, None, TS)}
        s = evaluation.summarize(_as_report(A, wants["right"][0], TS))
        print(name, "all", ["%.2f" % (100 * r) for r in s["all"]["bad_rate"]], "%.4f" % s["all"]["mean"], "nonocc", ["%.2f" % (100 * r) for r in s["nonocc"]["bad_rate"]],
              "%.4f" % s["nonocc"]["mean"])
        for fmt in ("u8", "u16", "f32"):
            for occ, echo in (("right", (1, 0, 0, 0)), ("mask", (0, 1, 0, 0)), ("none", (0, 0, 0, 0))):
                st.set_ground_truth(fl[fmt], fr[fmt] if occ == "right" else None, mask if occ == "mask" else None, 1.0)
                _check("%s %s %s" % (name, fmt, occ), st.evaluate(d, thresholds=TS), wants[occ], 4, echo)
        # right view AND a mask: the right view wins; another occ_thres; fewer thresholds (the unused ones report 0)
        st.set_ground_truth(fl["u8"], fr["f32"], mask, 0.25)
        _check(name + " occ_thres", st.evaluate(d, thresholds=[1.0]), E.evaluate(d, g, E.nonocc_from_right(g, g_right, 0.25), [1.0]), 1, (1, 0, 0, 0))
        assert st.eval_report().occ_thres == 0.25 and list(st.eval_report().thresholds) == [1.0, 0, 0, 0]
        _check(name + " no thresholds", st.evaluate(d, thresholds=[], err=False, cls=False), E.evaluate(d, g, E.nonocc_from_right(g, g_right, 0.25), []), 0)
    finally:
        st.Release()


def _as_report(A, rep, ts, prov=False, conf=False):
    r = A.EvalReport()
    words = E.to_words(rep)
    C.memmove(C.byref(r), words.ctypes.data, words.nbytes)
    r.n_thresholds, r.has_right_gt, r.has_provenance, r.has_confidence = len(ts), 1, int(prov), int(conf)
    for k, t in enumerate(ts):
        r.thresholds[k] = t
    return r


# case -> (option changes, speckle filter, the fill classes the case claims to cover, needs invalid pixels)
EXTRAS_CASES = {
    "cone": (dict(), None, (E.FILL_WTA, 1, 2), False),
    "cloth3": (dict(), None, (E.FILL_WTA, 1, 2), False),
    "wood2": (dict(), None, (E.FILL_WTA, 1), False),
    "cone_nofill_speckle": (dict(do_filling=0), (1000, 1.0), (E.FILL_WTA, 3), True),
    "cloth3_nofill": (dict(do_filling=0), None, (E.FILL_WTA, 3), True),
}


@pytest.mark.parametrize("case", list(EXTRAS_CASES))
def test_with_provenance_and_confidence(hip, oracle, case):
    """adc_match_device_ex, adc_wait, adc_evaluate_device, adc_wait on device buffers: the report, err and class equal eval_ref fed with
    the oracle's final map and tests/extras_ref.py's maps.  Each case has at least 1 % of its known pixels in every fill class it
    claims, and at least 1 % invalid where it claims invalid pixels (asserted: the case cannot pass vacuously)."""
    A = hip
    kw, speckle, fills, needs_invalid = EXTRAS_CASES[case]
    name = case.split("_")[0]
    left, right, opt = cases.make_case(name)
    for k, v in kw.items():
        setattr(opt, k, v)
    d, prov, conf = _oracle_maps(oracle, name, **kw)
    if speckle:
        filtered = speckle_ref(d, *speckle)[0]
        prov = np.where(np.isfinite(d) & ~np.isfinite(filtered), prov | A.PROV_SPECKLE, prov).astype(np.uint8)
        d = filtered
    raw_l, raw_r, scale = load_gt(name)
    g, g_right = E.decode_gt(raw_l, E.GT_U8, scale), E.decode_gt(raw_r, E.GT_U8, scale)
    want = E.evaluate(d, g, E.nonocc_from_right(g, g_right, 1.0), TS, prov, conf)
    known = want[0]["all"]["pixels"]
    for f in fills:
        assert want[0]["by_fill"][f]["pixels"] >= 0.01 * known, (case, f, want[0]["by_fill"][f]["pixels"], known)
    if needs_invalid:
        assert want[0]["all"]["invalid"] >= 0.01 * known, (case, want[0]["all"]["invalid"], known)
    if speckle:
        assert want[0]["speckle_removed_known"] >= 0.01 * known, (case, want[0]["speckle_removed_known"])
    assert want[0]["conf_pixels"].sum() > 0.5 * known and want[0]["conf_bad"].sum() > 0
    h, w = d.shape
    n = w * h
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        if speckle:
            st.set_speckle_filter(*speckle)
        st.set_ground_truth(raw_l, raw_r, scale=scale)
        dl, dr, dd, dp, dc = dev.new(left), dev.new(right), dev.alloc(4 * n), dev.alloc(n), dev.alloc(4 * n)
        de, dk = dev.alloc(4 * n, POISON), dev.alloc(n, POISON)
        assert st.match_device_ex(dl, dr, dd, dp, dc) and st.wait(), A.last_error()
        assert np.array_equal(_u32(dev.get(dd, (h, w), F)), _u32(d)) and np.array_equal(dev.get(dp, (h, w), np.uint8), prov)
        assert st.evaluate_device(dd, dp, dc, TS, de, dk) and st.wait(), A.last_error()
        _check(case + " device", (st.eval_report(), dev.get(de, (h, w), F), dev.get(dk, (h, w), np.uint8)), want, 4, (1, 0, 1, 1))
        # the report only; provenance without confidence (the confidence bins stay zero)
        assert st.evaluate_device(dd, dp, dc, TS) and st.wait(), A.last_error()
        _check(case + " report only", (st.eval_report(), None, None), want)
        assert st.evaluate_device(dd, dp, None, TS) and st.wait(), A.last_error()
        _check(case + " provenance only", (st.eval_report(), None, None), E.evaluate(d, g, E.nonocc_from_right(g, g_right, 1.0), TS, prov), 4, (1, 0, 1, 0))
        # the host entry point on the same maps
        _check(case + " host", st.evaluate(d, prov, conf, TS), want, 4, (1, 0, 1, 1))
        s = evaluation.summarize(st.eval_report())
        print(case, {k: (v["pixels"], ["%.2f" % (100 * r) for r in v["bad_rate"]]) for k, v in s["by_fill"].items()}, "confidence area %.4f, best %.4f, random %.4f"
              % (s["confidence"]["area"], s["confidence"]["oracle_area"], s["confidence"]["random_area"]))
    finally:
        dev.free()
        st.Release()


def _synthetic(rng, h, w, kind="mixed"):
    """(raw float32 ground truth, map, provenance, confidence) with every special value the definition names"""
    n = h * w
    g = (rng.random((h, w)) * 200).astype(F)
    g[rng.random((h, w)) < 0.07] = np.nan  # unknown
    d = (np.nan_to_num(g) + rng.normal(0, 1.5, (h, w))).astype(F)
    pick = rng.random((h, w))
    d[pick < 0.05] = INF
    d[(pick >= 0.05) & (pick < 0.06)] = np.nan
    d[(pick >= 0.06) & (pick < 0.07)] = -INF
    d[(pick >= 0.07) & (pick < 0.08)] += F(2048)      # at and beyond the clamp
    d[(pick >= 0.08) & (pick < 0.09)] = F(-3e38)
    d[(pick >= 0.09) & (pick < 0.12)] = np.nan_to_num(g)[(pick >= 0.09) & (pick < 0.12)] + F(1.0)  # e == t exactly (not bad)
    flat = d.reshape(-1)
    flat[: min(n, 3)] = [F(2048.0), F(4096.5), INF][: min(n, 3)]
    prov = rng.integers(0, 32, (h, w)).astype(np.uint8)
    conf = rng.random((h, w)).astype(F)
    cp = rng.random((h, w))
    conf[cp < 0.1] = 0.0
    conf[(cp >= 0.1) & (cp < 0.2)] = 1.0
    conf[(cp >= 0.2) & (cp < 0.21)] = np.nan
    conf[(cp >= 0.21) & (cp < 0.22)] = -0.5
    conf[(cp >= 0.22) & (cp < 0.23)] = 7.0
    if kind == "all_inf":
        d[:] = INF
    if kind == "all_unknown":
        g[:] = np.nan
    if kind == "exact":
        d = np.nan_to_num(g).astype(F)
    return g, d, prov, conf


@pytest.mark.parametrize("w,h", [(333, 77), (4099, 1), (1, 2053), (1024, 1), (1025, 3), (1242, 375), (1920, 1080)])
def test_synthetic_maps_at_the_kernel_edges(hip, w, h):
    """Sizes around the tile of 1024 pixels and the grid-stride loop, a single row, a single column, KITTI size and 1080p; maps with
    +inf, NaN, -inf, errors at and beyond the clamp, confidence exactly 0 and 1 (and outside [0, 1]); a map of all +inf; ground truth
    all unknown; an exact map.  Buffers behind the per-pixel outputs must stay untouched."""
    A = hip
    rng = np.random.default_rng(w * 7 + h)
    n = w * h
    st, dev = _handle(A, w, h, pyoracle.Option(max_disparity=8)), DeviceBuffers(A)
    try:
        for kind in ("mixed", "all_inf", "all_unknown", "exact"):
            g_raw, d, prov, conf = _synthetic(rng, h, w, kind)
            g_right = np.roll(g_raw, -3, axis=1)
            g = E.decode_gt(g_raw, E.GT_F32, 1.0)
            non = E.nonocc_from_right(g, E.decode_gt(g_right, E.GT_F32, 1.0), 1.0)
            want = E.evaluate(d, g, non, [1.0, 2048.0, 0.0], prov, conf)
            if kind == "mixed" and n > 1000:
                a = want[0]["all"]
                assert a["invalid"] > 0 and a["bad"][1] > 0 and a["err_hist"][255] > 0 and want[0]["conf_pixels"][[0, 255]].all() and a["bad"][2] > a["bad"][0] > 0
            st.set_ground_truth(g_raw, g_right)
            dd, dp, dc = dev.new(d), dev.new(prov), dev.new(conf)
            de, dk = dev.alloc(4 * n + 64, POISON), dev.alloc(n + 64, POISON)
            assert st.evaluate_device(dd, dp, dc, [1.0, 2048.0, 0.0], de, dk) and st.wait(), A.last_error()
            err, cls = dev.get(de, n + 16, F), dev.get(dk, n + 64, np.uint8)
            assert err[n:].tobytes() == bytes([POISON]) * 64 and cls[n:].tobytes() == bytes([POISON]) * 64, "written behind the maps"
            _check("%dx%d %s" % (w, h, kind), (st.eval_report(), err[:n].reshape(h, w), cls[:n].reshape(h, w)), want, 3, (1, 0, 1, 1))
            if kind == "all_unknown":
                assert not st.eval_report().words().any()
            dev.free()
    finally:
        dev.free()
        st.Release()


def test_refusals_on_a_real_handle(hip):
    A = hip
    w, h, d = 256, 160, 64
    left, right = workloads.structured_pair(w, h, d, seed=41)
    n = w * h
    st, dev = _handle(A, w, h, pyoracle.Option(max_disparity=d)), DeviceBuffers(A)
    try:
        dl, dr, dd, dp = dev.new(left), dev.new(right), dev.alloc(4 * n), dev.alloc(n)
        gt = np.full((h, w), 40, np.uint8)
        assert not st.evaluate_device(dd) and "no ground truth" in A.last_error()
        with pytest.raises(RuntimeError, match="no evaluation"):
            st.eval_report()
        with pytest.raises(RuntimeError, match="pitch"):
            st.set_ground_truth(A.GroundTruth(gt, 4.0, pitch_bytes=w - 1))
        with pytest.raises(RuntimeError, match="2 GiB"):
            st.set_ground_truth(A.GroundTruth(gt, 4.0, pitch_bytes=1 << 30))
        assert not st.evaluate_device(dd) and "no ground truth" in A.last_error()
        st.set_ground_truth(gt, scale=4.0)
        assert st.match_device(dl, dr, dd), A.last_error()
        # REFUSED while the Match is pending: a redo in adc_wait would rewrite the map behind the evaluation
        assert not st.evaluate_device(dd) and "Match is pending" in A.last_error()
        with pytest.raises(RuntimeError, match="Match is pending"):
            st.set_ground_truth(gt, scale=4.0)
        with pytest.raises(RuntimeError, match="Match is pending"):
            st.clear_ground_truth()
        assert st.wait(), A.last_error()
        want_d = dev.get(dd, (h, w), F)
        assert not st.evaluate_device(dd, None, dp) and "provenance" in A.last_error()
        assert not st.evaluate_device(dd, thresholds=[1, 2, 3, 4, 5]) and "at most 4" in A.last_error()
        assert not st.evaluate_device(dd, thresholds=[-1.0]) and "threshold" in A.last_error()
        assert st.evaluate_device(dd) and st.wait(), A.last_error()
        g = E.decode_gt(gt, E.GT_U8, 4.0)
        _check("after the refusals", (st.eval_report(), None, None), E.evaluate(want_d, g, None, [1.0]), 1, (0, 0, 0, 0))
        assert st.eval_report().all.pixels == n
        st.clear_ground_truth()
        assert not st.evaluate_device(dd) and "no ground truth" in A.last_error()
        assert st.eval_report().all.pixels == n  # (the last completed report stays)
        assert np.array_equal(_u32(st.match(left, right)), _u32(want_d))
    finally:
        dev.free()
        st.Release()


def test_redo_paths_are_followed_by_an_exact_evaluation(hip, oracle, monkeypatch):
    """The redo paths of adc_wait, forced as in tests/test_gpu_outputs.py::test_redo_paths_keep_the_outputs_exact (aggregation ring
    redo, continued voting chain, median fallback in both forms), each followed by an evaluation: it scores the delivered map."""
    A = hip
    w, h, d = 256, 160, 64
    opt = pyoracle.Option(max_disparity=d)
    rng = np.random.default_rng(9)
    gt = rng.integers(0, 4 * d, (h, w)).astype(np.uint8)
    gt[rng.random((h, w)) < 0.1] = 0
    gt_r = np.roll(gt, -5, axis=1)
    g = E.decode_gt(gt, E.GT_U8, 4.0)
    non = E.nonocc_from_right(g, E.decode_gt(gt_r, E.GT_U8, 4.0), 1.0)
    n = w * h

    def want_of(pair, o):
        dump = oracle.run(*pair, o, stages=extras_ref.STAGES)
        prov, conf = extras_ref.extras(dump, o)
        return dump["disp_final"], E.evaluate(dump["disp_final"], g, non, TS, prov, conf)

    def run(st, dev, bufs, pair, what, want):
        dl, dr, dd, dp, dc, de, dk = bufs
        dev.put(dl, pair[0]), dev.put(dr, pair[1])
        assert st.match_device_ex(dl, dr, dd, dp, dc) and st.wait(), A.last_error()
        assert np.array_equal(_u32(dev.get(dd, (h, w), F)), _u32(want[0])), what
        assert st.evaluate_device(dd, dp, dc, TS, de, dk) and st.wait(), A.last_error()
        _check(what, (st.eval_report(), dev.get(de, (h, w), F), dev.get(dk, (h, w), np.uint8)), want[1], 4, (1, 0, 1, 1))

    s_pair = workloads.structured_pair(w, h, d, seed=41)
    n_pair = workloads.noise_pair(w, h, seed=42)
    want_s, want_n = want_of(s_pair, opt), want_of(n_pair, opt)
    monkeypatch.setenv("ADC_AGG_DUAL", "0")
    for phase in ("aggregation", "voting", "median"):
        st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
        try:
            st.set_ground_truth(gt, gt_r, scale=4.0)
            bufs = [dev.alloc(s) for s in (3 * n, 3 * n, 4 * n, n, 4 * n, 4 * n, n)]
            run(st, dev, bufs, s_pair, phase + ": structured, first", want_s)
            if phase == "aggregation":
                run(st, dev, bufs, n_pair, "noise", want_n)
                run(st, dev, bufs, n_pair, "noise, small ring assumed", want_n)
                redo0 = st.debug_counter(2)
                run(st, dev, bufs, s_pair, "structured, aggregation redo", want_s)
                assert st.debug_counter(2) == redo0 + 1, "the aggregation redo path was not taken"
            elif phase == "voting":
                st.debug_set_budget(4)
                over = st.debug_counter(1)
                run(st, dev, bufs, s_pair, "structured, voting chain continued", want_s)
                assert st.debug_counter(1) == over + 1, "the voting continuation path was not taken"
            else:
                for arg in (100, 101):
                    fall = st.debug_counter(0)
                    st.debug_run(A.RUN_MEDIAN, arg)
                    run(st, dev, bufs, s_pair, "median fallback %d" % arg, want_s)
                    assert st.debug_counter(0) == fall + 1, "the median fallback path was not taken"
        finally:
            dev.free()
            st.Release()


def test_cli_gt_on_cone(hip, oracle, tmp_path):
    """adcensus_cli ... --gt on Cone: the table carries the figures of the definition on the oracle's map, <out>-err.pfm equals it bit for
    bit, and the files of a run without the flag do not change."""
    from PIL import Image
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    left, right, opt = cases.make_case("cone")
    want_d, prov, conf = _oracle_maps(oracle, "cone")
    raw_l, raw_r, scale = load_gt("cone")
    Image.fromarray(np.ascontiguousarray(left[:, :, ::-1])).save(tmp_path / "left.png")
    Image.fromarray(np.ascontiguousarray(right[:, :, ::-1])).save(tmp_path / "right.png")
    Image.fromarray(raw_l).save(tmp_path / "disp2.png")
    Image.fromarray(raw_r).save(tmp_path / "disp6.png")
    env = dict(os.environ, ADC_VERBOSE="0")
    outs = {}
    for pref, extra in (("plain", []), ("gt", ["--gt", "%s,%s,%d" % (tmp_path / "disp2.png", tmp_path / "disp6.png", scale), "--bad", "0.5,1,2,4", "--extras"])):
        out = subprocess.run([cli, str(tmp_path / "left.png"), str(tmp_path / "right.png"), "0", "64", str(tmp_path / pref)] + extra,
                             capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[pref] = out.stdout
    print(outs["gt"])
    for suffix in ("-d.png", "-c.png", "-cloud.txt", ".pfm"):
        assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / "gt") + suffix, "rb").read(), suffix
    assert not os.path.exists(str(tmp_path / "plain") + "-err.pfm") and "Evaluation" not in outs["plain"]
    g, g_right = E.decode_gt(raw_l, E.GT_U8, scale), E.decode_gt(raw_r, E.GT_U8, scale)
    rep, err, cls = E.evaluate(want_d, g, E.nonocc_from_right(g, g_right, 1.0), TS, prov, conf)
    assert np.array_equal(_u32(read_pfm(str(tmp_path / "gt") + "-err.pfm")), _u32(err))
    assert Image.open(str(tmp_path / "gt") + "-bad.png").size == (want_d.shape[1], want_d.shape[0])
    rows = {ln.split()[0]: ln.split() for ln in outs["gt"].splitlines() if ln.split() and ln.split()[0] in ("all", "nonocc", "fill:wta", "fill:voting", "fill:interp")}
    for key, s in (("all", rep["all"]), ("nonocc", rep["nonocc"]), ("fill:wta", rep["by_fill"][0]), ("fill:voting", rep["by_fill"][1]), ("fill:interp", rep["by_fill"][2])):
        assert int(rows[key][1]) == s["pixels"] and rows[key][3:7] == ["%.2f" % (100.0 * b / s["pixels"]) for b in s["bad"]], (key, rows[key])
        assert rows[key][7] == "%.4f" % (s["sum_err_q"] / 1024.0 / (s["pixels"] - s["invalid"])), (key, rows[key])
    # the figures the project has quoted for this pair since its first survey: 10.0 % of the known pixels off by more than one pixel
    assert rows["all"][1] == "163321" and rows["all"][3:7] == ["15.00", "10.03", "7.37", "5.11"] and rows["nonocc"][3:7] == ["8.03", "3.67", "2.77", "1.76"]
    assert "sparsification area" in outs["gt"]


def _probe(*args):
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "eval_fault_probe.py"), *args], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FAULT_PROBE ")][-1][len("FAULT_PROBE "):])


def test_off_means_untouched(hip):
    """adc_create allocates nothing of the feature, and after adc_set_ground_truth followed by adc_clear_ground_truth a plain adc_match
    and a plain adc_match_device + adc_wait make exactly the hooked HIP calls of the parent revision."""
    o = _probe("--counts-only")
    print(o)
    assert {k: o[k] for k in PARENT_CALLS} == PARENT_CALLS, o
    # the hook sits on the new calls.  The first set call of a handle: CU count, 2 ground-truth maps, occlusion map, report words, pinned block, raw buffer (7), then 2 uploads,
    # 3 kernels, 2 waits; a later one only the second part
    assert o["set_first_calls"] >= o["set_calls"] + 7 and o["set_calls"] >= 7, o


def test_hip_failures_on_the_evaluation_paths(hip):
    """The fault-injection build: every HIP call of adc_set_ground_truth (first use included), of adc_evaluate (first use included) and
    of adc_evaluate_device + adc_wait fails once (an injected return code, never a device fault) -- the call reports it, nothing
    leaks, the same handle delivers the exact report and maps and an exact Match afterwards."""
    o = _probe()
    print(o)
    # adc_evaluate: 5 first-use allocations; 3 uploads, memset, kernel, read-back, the wait, 2 copy-outs; the device form: 3 + the wait
    assert o["eval_first_calls"] >= o["eval_calls"] + 5 and o["eval_calls"] >= 9 and o["device_calls"] >= 4, o
    assert o["known"] > 0
    for name in ("set", "eval", "device"):
        assert o[name + "_not_failed"] == [] and o[name + "_wrong_after"] == [], (name, o)
    assert abs(o["set_leak_bytes"]) <= (2 << 20) and abs(o["eval_leak_bytes"]) <= (2 << 20) and abs(o["final_leak_bytes"]) <= (2 << 20), o
