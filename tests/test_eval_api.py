"""CPU tier of the ground-truth evaluation: tests/eval_ref.py (the definition the GPU tests hold the kernels to) on hand-made maps whose
counts are written out here and against a scalar loop written from the header word for word; the pixel counts of the committed
ground-truth fixtures; the derived figures of adcensus_amd/evaluation.py; and the new surface of the C ABI, the Python mirror, the
facade and the CLI -- declared, exported, struct layouts, every refusal before a HIP call, malformed --gt / --bad, the sanitizer
build (whose stub of the C ABI is a third, plain-C statement of the definition)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from adcensus_amd import evaluation
from tests import cases
from tests import eval_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
ENTRY_POINTS = ["adc_set_ground_truth", "adc_clear_ground_truth", "adc_evaluate_device", "adc_evaluate", "adc_get_eval_report"]
F = np.float32
INF = F(np.inf)
NAN = F(np.nan)
# the issue's table: known and non-occluded pixels of the three pairs (occ_thres = 1.0), from the fixtures alone
FIXTURE_COUNTS = {"cone": (168750, 163321, 143397), "cloth3": (347430, 344585, 307552), "wood2": (362415, 355534, 309333)}


def load_gt(name):
    z = np.load(os.path.join(cases.GOLDEN_DIR, name + "_gt.npz"))
    return np.ascontiguousarray(z["left"]), np.ascontiguousarray(z["right"]), int(z["scale"])


def brute_evaluate(d, g, non, ts, prov=None, conf=None):
    """The header's definition, one pixel at a time (float32 scalars); non: bool map or None.  Returns (words, err, class)."""
    H, W = d.shape
    t = [F(x) for x in ts] + [INF] * (4 - len(ts))
    w = np.zeros(E.WORDS, np.uint64)
    err, cls = np.full((H, W), INF, F), np.zeros((H, W), np.uint8)
    M = (1 << 64) - 1

    def add(base, full, valid, bad, eq):
        w[base] += np.uint64(1)
        if not valid:
            w[base + 1] += np.uint64(1)
            return
        for k in range(4):
            w[base + 2 + k] += np.uint64(bad[k])
        w[base + 6] = np.uint64((int(w[base + 6]) + eq) & M)
        if full:
            w[base + 7] = np.uint64((int(w[base + 7]) + eq * eq) & M)
            w[base + 8 + min(eq >> 8, 255)] += np.uint64(1)

    for y in range(H):
        for x in range(W):
            known, valid = bool(np.isfinite(g[y, x])), bool(np.isfinite(d[y, x]))
            kv = known and valid
            e = abs(F(d[y, x] - g[y, x])) if kv else INF
            eq = int(np.rint(F(min(e, F(2048.0)) * F(1024.0)))) if kv else 0
            bad = [int(kv and e > t[k]) for k in range(4)]
            n = known and non is not None and bool(non[y, x])
            if known:
                add(0, True, valid, bad, eq)
            if n:
                add(264, True, valid, bad, eq)
            if prov is not None and known:
                fill = (int(prov[y, x]) >> 2) & 3
                add(528 + 7 * fill, False, valid, bad, eq)
                if int(prov[y, x]) & 0x10:
                    w[556] += np.uint64(1)
                if conf is not None and kv and fill == 0:
                    c = F(conf[y, x] * F(256.0))
                    b = 0 if not c >= 0 else (255 if c >= 255 else int(c))
                    w[557 + b] += np.uint64(1)
                    w[813 + b] += np.uint64(bad[0])
            err[y, x] = e
            cls[y, x] = (1 if known else 0) | (2 if valid else 0) | (4 if bad[0] else 0) | (8 if known and non is not None and not n else 0)
    return w, err, cls


def hand_made():
    """4 x 6: one unknown, two invalid (+inf, NaN), occluded pixels of every kind, errors exactly at both thresholds, g = 2.5 and 3.5."""
    raw = np.array([[8, 8, 8, 8, 0, 8], [10] * 6, [14] * 6, [4] * 6], np.uint8)  # scale 4: 2, 2.5, 3.5, 1
    gr = np.array([[2, 3, 2, 3.5, 2, 2], [2.5, 2.5, INF, 2.5, 9, 9], [3.5, 3.5, 0, 0, 0, 0], [1] * 6], F)
    d = np.array([[2, 2.5, 2, INF, 7, 3], [2.5, 2.5, 4, 2.5, 2.5, 2.5], [NAN, 3.5, 3.5, 3.5, 3.5, 3.5], [2, 1, 1, 1, 1, -1]], F)
    prov = np.tile(np.array([0, 0, 5, 5, 10, 13], np.uint8), (4, 1))
    prov[0, 4] |= 0x10  # (unknown: not counted)
    prov[0, 5] |= 0x10
    conf = np.zeros((4, 6), F)
    conf[:, 1] = [1.0, 1.0, 0.5, 0.999]
    return raw, gr, d, prov, conf


def test_hand_made_map_counts():
    raw, gr, d, prov, conf = hand_made()
    g = E.decode_gt(raw, E.GT_U8, 4)
    assert g.tolist() == [[2, 2, 2, 2, np.inf, 2], [2.5] * 6, [3.5] * 6, [1] * 6]
    non = E.nonocc_from_right(g, gr, 1.0)
    # row 0: x - 2; (0,3) sees gr = 3 (difference exactly 1: kept), (0,5) sees 3.5 (dropped).  row 1: rintf(2.5) = 2, ties to even: x = 2
    # looks at column 0 (round-half-up would leave the image); (1,4) meets an unknown.  row 2: rintf(3.5) = 4.  row 3: x - 1
    assert non.astype(int).tolist() == [[0, 0, 1, 1, 0, 0], [0, 0, 1, 1, 0, 1], [0, 0, 0, 0, 1, 1], [0, 1, 1, 1, 1, 1]]
    rep, err, cls = E.evaluate(d, g, non, [0.5, 1.0], prov, conf)
    a, n = rep["all"], rep["nonocc"]
    # errors: (0,1) 0.5 == t0 and (0,5) 1.0 == t1 are not above their threshold; (1,2) 1.5, (3,0) 1.0, (3,5) 2.0
    assert (a["pixels"], a["invalid"], a["bad"]) == (23, 2, [4, 2, 0, 0])
    assert (a["sum_err_q"], a["sum_sq_err_q"]) == (1024 * 6, 1024 * 1024 * (0.25 + 1 + 2.25 + 1 + 4))
    hist = np.zeros(256, np.uint64)
    hist[[0, 2, 4, 6, 8]] = [16, 1, 2, 1, 1]
    assert np.array_equal(a["err_hist"], hist)
    assert (n["pixels"], n["invalid"], n["bad"], n["sum_err_q"], n["sum_sq_err_q"]) == (12, 1, [2, 2, 0, 0], 1024 * 3.5, 1024 * 1024 * 6.25)
    fills = [(s["pixels"], s["invalid"], s["bad"], s["sum_err_q"]) for s in rep["by_fill"]]
    assert fills == [(8, 1, [1, 0, 0, 0], 1536), (8, 1, [1, 1, 0, 0], 1536), (3, 0, [0, 0, 0, 0], 0), (4, 0, [2, 1, 0, 0], 3072)]
    assert rep["speckle_removed_known"] == 1
    cp, cb = np.zeros(256, np.uint64), np.zeros(256, np.uint64)
    cp[[0, 128, 255]] = [3, 1, 3]  # (0.999 * 256 = 255.7: the last bin)
    cb[0] = 1
    assert np.array_equal(rep["conf_pixels"], cp) and np.array_equal(rep["conf_bad"], cb)
    assert err[0].tolist() == [0, 0.5, 0, np.inf, np.inf, 1] and err[2, 0] == INF and err[3, 5] == 2
    assert cls.tolist() == [[11, 11, 3, 1, 2, 15], [11, 11, 7, 3, 11, 3], [9, 11, 11, 11, 3, 3], [15, 3, 3, 3, 3, 7]]
    words, berr, bcls = brute_evaluate(d, g, non, [0.5, 1.0], prov, conf)
    assert np.array_equal(E.to_words(rep), words) and np.array_equal(err.view(np.uint32), berr.view(np.uint32)) and np.array_equal(cls, bcls)
    # without occlusion information: nonocc is empty and no pixel is marked occluded; without maps: the fill words stay zero
    rep0, _, cls0 = E.evaluate(d, g, None, [0.5])
    assert rep0["nonocc"]["pixels"] == 0 and not (cls0 & E.OCCLUDED).any() and not E.to_words(rep0)[264:].any()
    assert rep0["all"]["bad"] == [4, 0, 0, 0]
    # a caller mask instead of the right view
    mask = np.zeros((4, 6), np.uint8)
    mask[:, 3:] = 7
    assert E.nonocc_from_mask(g, mask).sum() == 11  # (the unknown pixel is never in a mask)


def test_ground_truth_formats_and_ties():
    raw8 = np.array([[0, 1, 5, 255]], np.uint8)
    assert E.decode_gt(raw8, E.GT_U8, 4).tolist() == [[np.inf, 0.25, 1.25, 63.75]]
    assert E.decode_gt(raw8.astype(np.uint16) * 257, E.GT_U16, 256).view(np.uint32).tolist() == (np.array([[np.inf, 257, 1285, 65535]], F) / F(256)).view(np.uint32).tolist()
    f = np.array([[0.0, -1.5, NAN, INF, -INF, 3e38]], F)
    assert E.decode_gt(f, E.GT_F32, 1).tolist() == [[0, -1.5, np.inf, np.inf, np.inf, F(3e38)]]  # (0 is a disparity in PFM ground truth)
    assert E.decode_gt(f, E.GT_F32, 0.5).tolist()[0][5] == np.inf  # (the quotient overflows: unknown)
    third = E.decode_gt(np.array([[1, 2]], np.uint8), E.GT_U8, 3)
    assert third.view(np.uint32).tolist() == [[F(F(1) / F(3)).view(np.uint32), F(F(2) / F(3)).view(np.uint32)]]
    # ties to even in the occlusion lookup: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4; a huge disparity is out of range, not an overflow
    g = np.array([[0.5, 1.5, 2.5, 3.5, 4.5, 3e9]], F)
    only0 = np.array([[1, INF, INF, INF, INF, INF]], F)  # x - rintf(g) = 0, -1, 0, -1, 0, far out: pixels 0, 2, 4 look at column 0
    assert E.nonocc_from_right(g, only0, 100.0).astype(int).tolist() == [[1, 0, 1, 0, 1, 0]]
    assert not E.nonocc_from_right(g, np.array([[INF, 1, 1, 1, 1, 1]], F), 100.0).any()
    assert E.nonocc_from_right(g, only0, 1.0).astype(int).tolist() == [[1, 0, 0, 0, 0, 0]]  # |1 - 0.5| <= 1 < |1 - 2.5|


def test_clamp_and_confidence_bins():
    g = np.zeros((1, 6), F)
    d = np.array([[2047.9999, 2048, 2049, 3e38, -3e38, 0.00048828125]], F)
    rep, err, _ = E.evaluate(d, g, None, [2048.0])
    assert rep["all"]["bad"][0] == 3 and rep["all"]["err_hist"][255] == 5 and rep["all"]["err_hist"][0] == 1
    # 2047.9999 * 1024 = 2097151.875 exactly, rintf: 2^21; 2^-11 px * 1024 = 0.5 -> rintf ties to even: 0
    assert rep["all"]["sum_err_q"] == 5 * 2048 * 1024 and rep["all"]["sum_sq_err_q"] == 5 * (2048 * 1024) ** 2
    big = np.full((1, 5000), 2048, F)  # the squares wrap modulo 2^64 (5000 * 2^42 does not, 2^22 * 2^42 would)
    assert E.evaluate(big, np.zeros_like(big), None, [])[0]["all"]["sum_sq_err_q"] == 5000 * (1 << 42)
    assert E.conf_bin(np.array([0.0, 1.0, 0.5, -0.0, -1.0, NAN, 2.0, 0.99609375, 0.996], F)).tolist() == [0, 255, 128, 0, 0, 0, 255, 255, 254]


def test_fixture_pixel_counts():
    for name, (pixels, known, nonocc) in FIXTURE_COUNTS.items():
        left, right, scale = load_gt(name)
        assert left.dtype == np.uint8 and left.shape == right.shape == cases.make_case(name)[0].shape[:2] and left.size == pixels
        g, gr = E.decode_gt(left, E.GT_U8, scale), E.decode_gt(right, E.GT_U8, scale)
        assert int(np.isfinite(g).sum()) == known, name
        assert int(E.nonocc_from_right(g, gr, 1.0).sum()) == nonocc, name
        assert os.path.getsize(os.path.join(cases.GOLDEN_DIR, name + "_gt.npz")) < 1 << 20


def _report_from_words(words, ts, prov, conf):
    rep = A.EvalReport()
    C.memmove(C.byref(rep), np.ascontiguousarray(words).ctypes.data, words.nbytes)
    rep.n_thresholds, rep.occ_thres, rep.has_right_gt, rep.has_provenance, rep.has_confidence = len(ts), 1.0, 1, int(prov), int(conf)
    for k, t in enumerate(ts):
        rep.thresholds[k] = t
    return rep


def test_summarize_reproduces_the_hand_made_rates():
    raw, gr, d, prov, conf = hand_made()
    g = E.decode_gt(raw, E.GT_U8, 4)
    rep, _, _ = E.evaluate(d, g, E.nonocc_from_right(g, gr, 1.0), [0.5, 1.0], prov, conf)
    ct = _report_from_words(E.to_words(rep), [0.5, 1.0], True, True)
    assert np.array_equal(ct.words(), E.to_words(rep)) and ct.all.err_hist[4] == 2 and ct.by_fill[3].sum_err_q == 3072 and ct.conf_pixels[255] == 3
    s = evaluation.summarize(ct)
    assert s["thresholds"] == [0.5, 1.0] and s["occlusion_defined"]
    assert s["all"]["bad_rate"] == [4 / 23, 2 / 23] and s["all"]["invalid_rate"] == 2 / 23 and s["all"]["mean"] == 6 / 21
    assert math.isclose(s["all"]["rms"], math.sqrt(8.5 / 21)) and s["nonocc"]["bad_rate"] == [2 / 12, 2 / 12] and s["nonocc"]["mean"] == 3.5 / 11
    assert s["by_fill"]["none"]["bad_rate"] == [0.5, 0.25] and s["by_fill"]["interpolation"]["mean"] == 0 and s["speckle_removed_known"] == 1
    c = s["confidence"]
    assert (c["pixels"], c["bad"]) == (7, 1) and c["curve"][0] == (0.0, 1 / 7) and c["curve"][1] == (3 / 7, 0.0) and c["curve"][-1] == (1.0, 0.0)
    assert math.isclose(c["area"], 0.5 * (3 / 7) * (1 / 7)) and c["oracle_area"] < c["area"] < c["random_area"] == 1 / 7
    # the best ranking removes the bad pixels first, a constant confidence is the random ranking
    assert math.isclose(evaluation.sparsification([10, 90], [10, 0])[1], 0.5 * 0.1 * 0.1)
    assert math.isclose(evaluation.sparsification([100], [10])[1], 0.5 * 0.1) and evaluation.oracle_area(100, 0) == 0


def test_port_oracle_crop_against_the_scalar_definition():
    """The port oracle's map of a Cone crop, scored by the numpy definition and by the scalar loop: the same words, maps and rates."""
    from oracle import pyoracle
    from tests import extras_ref
    left, right, scale = load_gt("cone")
    y0, y1, x0, x1 = 100, 164, 120, 300
    iml, imr, _ = cases.make_case("cone")
    opt = pyoracle.Option(max_disparity=64, do_filling=0)
    dump = pyoracle.load("port").run(np.ascontiguousarray(iml[y0:y1, x0 - 64:x1]), np.ascontiguousarray(imr[y0:y1, x0 - 64:x1]), opt, stages=extras_ref.STAGES)
    prov, conf = extras_ref.extras(dump, opt)
    d, prov, conf = (np.ascontiguousarray(a[:, 64:]) for a in (dump["disp_final"], prov, conf))
    g, gr = E.decode_gt(left, E.GT_U8, scale), E.decode_gt(right, E.GT_U8, scale)
    non = E.nonocc_from_right(g, gr, 1.0)[y0:y1, x0:x1]  # (cross-checked on the full rows, then cropped)
    g = np.ascontiguousarray(g[y0:y1, x0:x1])
    ts = [0.5, 1.0, 2.0, 4.0]
    rep, err, cls = E.evaluate(d, g, non, ts, prov, conf)
    words, berr, bcls = brute_evaluate(d, g, non, ts, prov, conf)
    assert np.array_equal(E.to_words(rep), words) and np.array_equal(err.view(np.uint32), berr.view(np.uint32)) and np.array_equal(cls, bcls)
    s = evaluation.summarize(_report_from_words(words, ts, True, True))
    print("crop: all", s["all"], "nonocc", s["nonocc"], "confidence area", s["confidence"]["area"], s["confidence"]["random_area"])
    assert s["all"]["pixels"] > 0.9 * d.size and 0.01 < s["all"]["invalid_rate"] < 0.5 and s["by_fill"]["none"]["pixels"] > 0
    assert s["nonocc"]["bad_rate"][1] < s["all"]["bad_rate"][0] and s["confidence"]["area"] < s["confidence"]["random_area"]


def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    for name, value in (("ADC_GT_U8", 0), ("ADC_GT_U16", 1), ("ADC_GT_F32", 2), ("ADC_EVAL_MAX_THRESHOLDS", 4), ("ADC_EVAL_ERR_BINS", 256),
                        ("ADC_EVAL_CONF_BINS", 256), ("ADC_EVAL_KNOWN", 1), ("ADC_EVAL_VALID", 2), ("ADC_EVAL_BAD", 4), ("ADC_EVAL_OCCLUDED", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert (A.GT_U8, A.GT_U16, A.GT_F32, A.EVAL_KNOWN, A.EVAL_VALID, A.EVAL_BAD, A.EVAL_OCCLUDED) == (0, 1, 2, E.KNOWN, E.VALID, E.BAD, E.OCCLUDED)
    for lib in (A.LIB_PATH, os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(ENTRY_POINTS) <= names, lib
    # the struct layouts, asked of a C compiler
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(adc_gt), offsetof(adc_gt, format), offsetof(adc_gt, scale),\n'
                   ' sizeof(adc_eval_params), offsetof(adc_eval_params, thresholds), sizeof(adc_eval_mask_stats), offsetof(adc_eval_mask_stats, err_hist),\n'
                   ' sizeof(adc_eval_fill_stats), sizeof(adc_eval_report), offsetof(adc_eval_report, nonocc), offsetof(adc_eval_report, by_fill),\n'
                   ' offsetof(adc_eval_report, conf_bad), offsetof(adc_eval_report, thresholds), offsetof(adc_eval_report, has_right_gt)); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    R = A.EvalReport
    assert got == [C.sizeof(A.GroundTruth), A.GroundTruth.format.offset, A.GroundTruth.scale.offset, C.sizeof(A.EvalParams), A.EvalParams.thresholds.offset,
                   C.sizeof(A.EvalMaskStats), A.EvalMaskStats.err_hist.offset, C.sizeof(A.EvalFillStats), C.sizeof(R), R.nonocc.offset, R.by_fill.offset,
                   R.conf_bad.offset, R.thresholds.offset, R.has_right_gt.offset]
    assert R.thresholds.offset == 8 * E.WORDS and got[0] == 24 and got[3] == 20


def test_every_refusal_comes_before_a_hip_call():
    """No device here: each of these returns 1 with a message without touching HIP.  A zeroed block stands in for an idle handle
    without ground truth; a block of ones for a handle with ground truth set and a Match pending (every flag nonzero)."""
    L = A.lib()
    vp = C.c_void_p
    assert L.adc_set_ground_truth.argtypes == [vp, C.POINTER(A.GroundTruth), C.POINTER(A.GroundTruth), vp, C.c_float]
    assert L.adc_evaluate_device.argtypes == [vp, vp, vp, vp, C.POINTER(A.EvalParams), vp, vp]
    assert L.adc_evaluate.argtypes == [vp, vp, vp, vp, C.POINTER(A.EvalParams), vp, vp, C.POINTER(A.EvalReport)]
    idle = C.cast(C.create_string_buffer(1 << 20), vp)
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), vp)
    img = np.zeros((4, 8), np.uint8)
    good = A.GroundTruth(img, 4.0)
    rep, p1 = A.EvalReport(), A.EvalParams([1.0])
    dev = vp(4096)

    def refused(rc, *words):
        msg = A.last_error()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    refused(L.adc_set_ground_truth(None, C.byref(good), None, None, 1.0), "adc_set_ground_truth", "null handle")
    refused(L.adc_set_ground_truth(idle, None, None, None, 1.0), "null left")
    refused(L.adc_set_ground_truth(idle, C.byref(A.GroundTruth()), None, None, 1.0), "null ground-truth array")
    for fmt in (-1, 3, 77):
        refused(L.adc_set_ground_truth(idle, C.byref(A.GroundTruth(img, 4.0, format=fmt)), None, None, 1.0), "format")
        refused(L.adc_set_ground_truth(idle, C.byref(good), C.byref(A.GroundTruth(img, 4.0, format=fmt)), None, 1.0), "format")
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        refused(L.adc_set_ground_truth(idle, C.byref(A.GroundTruth(img, scale)), None, None, 1.0), "scale")
    for thres in (-0.5, float("nan"), float("inf")):
        refused(L.adc_set_ground_truth(idle, C.byref(good), None, None, thres), "occ_thres")
    refused(L.adc_set_ground_truth(idle, C.byref(A.GroundTruth(img, 4.0, pitch_bytes=-8)), None, None, 1.0), "pitch")
    refused(L.adc_set_ground_truth(busy, C.byref(good), None, None, 1.0), "Match is pending")
    # (a handle of 16843009 x 16843009 pixels, as the block of ones reads: the pitch of an 8-pixel row is too small -- after the state check)
    refused(L.adc_clear_ground_truth(None), "null handle")
    refused(L.adc_clear_ground_truth(busy), "Match is pending")
    assert L.adc_clear_ground_truth(idle) == 0
    for call in (lambda h, d, p, c, par: L.adc_evaluate_device(h, d, p, c, par, None, None),
                 lambda h, d, p, c, par: L.adc_evaluate(h, d, p, c, par, None, None, C.byref(rep))):
        refused(call(None, dev, None, None, C.byref(p1)), "null handle")
        refused(call(idle, None, None, None, C.byref(p1)), "null map")
        refused(call(idle, dev, None, None, C.byref(p1)), "no ground truth")
        refused(call(idle, dev, None, None, None), "no ground truth")
        refused(call(busy, dev, None, dev, C.byref(p1)), "confidence map needs a provenance map")
        refused(call(busy, dev, dev, dev, C.byref(A.EvalParams([1, 2, 3, 4, 5]))), "at most 4")
        bad_n = A.EvalParams([1.0])
        bad_n.n_thresholds = -1
        refused(call(busy, dev, None, None, C.byref(bad_n)), "at most 4")
        for t in (-1.0, float("nan"), float("inf"), -float("inf")):
            refused(call(busy, dev, None, None, C.byref(A.EvalParams([0.5, t]))), "threshold")
        refused(call(busy, dev, dev, dev, C.byref(A.EvalParams([0.5, 1, 2, 4]))), "Match is pending")
        refused(call(busy, dev, None, None, C.byref(A.EvalParams([]))), "Match is pending")
    refused(L.adc_get_eval_report(None, C.byref(rep)), "null")
    refused(L.adc_get_eval_report(idle, None), "null")
    refused(L.adc_get_eval_report(idle, C.byref(rep)), "no evaluation")
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    st.width, st.height = 8, 4
    with pytest.raises(RuntimeError):
        st.set_ground_truth(img, scale=4)
    with pytest.raises(RuntimeError):
        st.clear_ground_truth()
    with pytest.raises(RuntimeError):
        st.evaluate(np.zeros((4, 8), F))
    with pytest.raises(RuntimeError):
        st.eval_report()
    assert st.evaluate_device(4096) is False
    # the mirror's helpers
    assert (good.format, good.pitch_bytes, good.scale) == (A.GT_U8, 8, 4.0)
    wide = np.zeros((4, 16), np.uint16)
    view = A.GroundTruth(wide[:, :8], 256)
    assert (view.format, view.pitch_bytes, view.data) == (A.GT_U16, 32, wide.ctypes.data)
    assert A.GroundTruth(np.zeros((4, 8), F)).format == A.GT_F32
    p = A.EvalParams([0.5, 2])
    assert (p.n_thresholds, list(p.thresholds)) == (2, [0.5, 2.0, 0.0, 0.0])


CALLER = r'''
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
int main() {
    ADCensusStereo s; ADCensusOption o;
    uint8 img[32] = {0};
    float32 d[32] = {0};
    adc_gt gt = {img, ADC_GT_U8, 0, 4.0f, 0};
    adc_eval_params p = {2, {0.5f, 1.0f, 0.f, 0.f}};
    adc_eval_report rep;
    // before Initialize there is no matcher underneath: everything is refused
    bool ok = !s.SetGroundTruth(&gt, nullptr, nullptr, 1.0f) && !s.ClearGroundTruth() && !s.Evaluate(d, nullptr, nullptr, &p, nullptr, nullptr, &rep) && !s.EvalReport(&rep);
    return (ok && !s.Match(img, img, d) && !s.Initialize(0, 0, o)) ? 0 : 1;
}
'''


def test_facade_compiles_and_exports_the_members(tmp_path):
    src = tmp_path / "caller.cpp"
    src.write_text(CALLER)
    libdir = os.path.join(ROOT, "adcensus_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libadcensus.so")):
        pytest.fail("libadcensus.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "caller"),
                    "-L", libdir, "-ladcensus", "-ladcensus_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(libdir, "libadcensus.so")], capture_output=True, text=True, check=True).stdout
    assert "ADCensusStereo::SetGroundTruth(adc_gt const*, adc_gt const*, unsigned char const*, float)" in out
    assert "ADCensusStereo::ClearGroundTruth()" in out and "ADCensusStereo::EvalReport(adc_eval_report*) const" in out
    assert "ADCensusStereo::Evaluate(float const*, unsigned char const*, float const*, adc_eval_params const*, float*, unsigned char*, adc_eval_report*)" in out
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def test_cli_rejects_malformed_gt_and_bad_flags(tmp_path):
    """Checked while the arguments are parsed: the images named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    base = [cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "0", "64", str(tmp_path / "out")]
    for bad in (["--gt"], ["--gt", "gt.png"], ["--gt", "gt.png,"], ["--gt", ",4"], ["--gt", "a.png,,4"], ["--gt", "a.png,b.png,c.png,4"], ["--gt", "gt.png,0"],
                ["--gt", "gt.png,-2"], ["--gt", "gt.png,nan"], ["--gt", "gt.png,inf"], ["--gt", "gt.png,4x"], ["--gt", "a.png,b.png,four"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--gt refused" in r.stdout and "Image Loading" not in r.stdout, (bad, r.stdout)
    for bad in (["--bad"], ["--bad", ""], ["--bad", "1,"], ["--bad", ",1"], ["--bad", "1,2,3,4,5"], ["--bad", "-1"], ["--bad", "nan"], ["--bad", "inf"],
                ["--bad", "1;2"], ["--bad", "one"]):
        r = subprocess.run(base + ["--gt", "gt.png,4"] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--bad refused" in r.stdout and "Image Loading" not in r.stdout, (bad, r.stdout)
    r = subprocess.run(base + ["--bad", "1"], capture_output=True, text=True, timeout=120)  # (--bad without --gt)
    assert r.returncode != 0 and "--bad refused" in r.stdout
    r = subprocess.run(base + ["--gt", "gt.png,4", "--calib", "1,1,0,0,0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "separate runs" in r.stdout
    r = subprocess.run(base + ["--gt", "a.png,b.png,4", "--bad", "0.5,1,2,4", "--extras", "--speckle", "50,1"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Image Loading" in r.stdout and "refused" not in r.stdout  # (well-formed: gets as far as the images)


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = (int(v) for v in f.readline().split())
        f.readline()
        return np.ascontiguousarray(np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1])


def write_pfm(path, a):
    with open(path, "wb") as f:
        f.write(b"Pf\n%d %d\n-1.0\n" % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a[::-1], "<f4").tobytes())


def test_cli_gt_under_sanitizers(tmp_path):
    """The flag's parsing, the PNG / PFM ground-truth loaders, the table and the two writers in the ASAN / UBSAN build on the stub C
    ABI, whose evaluation is the header's definition in plain C: <out>-err.pfm and the table's counts equal tests/eval_ref.py."""
    from PIL import Image
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "adcensus_amd", "host"), "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cli = os.path.join(ROOT, "adcensus_amd", "build", "asan", "adcensus_cli_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    rng = np.random.default_rng(5)
    w, h = 83, 57
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "l.png")
    Image.fromarray(rgb[:, ::-1].copy()).save(tmp_path / "r.png")
    gl = rng.integers(0, 120, (h, w)).astype(np.uint8)
    gl[rng.random((h, w)) < 0.1] = 0
    gr = np.roll(gl, -7, axis=1)
    Image.fromarray(gl).save(tmp_path / "gl.png")
    Image.fromarray(gr).save(tmp_path / "gr.png")
    Image.fromarray(rgb).save(tmp_path / "colour.png")
    gf = np.where(gl == 0, INF, gl.astype(F) / F(4)).astype(F)
    write_pfm(tmp_path / "gl.pfm", gf)

    def run(*extra):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "-3", "29", *extra], env=env, capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        return r

    assert run(str(tmp_path / "plain")).returncode == 0
    disp = read_pfm(str(tmp_path / "plain") + ".pfm")
    r = run(str(tmp_path / "both"), "--gt", "%s,%s,4" % (tmp_path / "gl.png", tmp_path / "gr.png"), "--bad", "0.5,1,2,4")
    assert r.returncode == 0, r.stdout
    g, g_right = E.decode_gt(gl, E.GT_U8, 4), E.decode_gt(gr, E.GT_U8, 4)
    rep, err, cls = E.evaluate(disp, g, E.nonocc_from_right(g, g_right, 1.0), [0.5, 1, 2, 4])
    assert np.array_equal(read_pfm(str(tmp_path / "both") + "-err.pfm").view(np.uint32), err.view(np.uint32))
    assert Image.open(str(tmp_path / "both") + "-bad.png").size == (w, h)
    rows = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("all", "nonocc")}
    for key in ("all", "nonocc"):
        s = rep[key]
        assert int(rows[key][1]) == s["pixels"] > 0 and rows[key][2] == "%.2f" % (100.0 * s["invalid"] / s["pixels"])
        assert rows[key][3:7] == ["%.2f" % (100.0 * b / s["pixels"]) for b in s["bad"]]
        assert rows[key][7] == "%.4f" % (s["sum_err_q"] / 1024.0 / (s["pixels"] - s["invalid"]))
    for name in ("plain", "both"):  # the existing files do not change with the flag
        assert open(str(tmp_path / "plain") + ".pfm", "rb").read() == open(str(tmp_path / name) + ".pfm", "rb").read()
    assert not os.path.exists(str(tmp_path / "plain") + "-err.pfm")
    # PFM ground truth (scale 1), left view only, with the maps of --extras and the speckle filter
    r = run(str(tmp_path / "pfm"), "--gt", "%s,1" % (tmp_path / "gl.pfm"), "--extras", "--speckle", "5,1")
    assert r.returncode == 0 and "fill:wta" in r.stdout and "nonocc" not in r.stdout and "sparsification" in r.stdout, r.stdout
    rep1, err1, _ = E.evaluate(read_pfm(str(tmp_path / "pfm") + ".pfm"), gf, None, [1.0])
    assert np.array_equal(read_pfm(str(tmp_path / "pfm") + "-err.pfm").view(np.uint32), err1.view(np.uint32))
    # refused behind the images: a ground truth of another size, a colour image, a missing file -- nothing is matched
    Image.fromarray(gl[:, :-1].copy()).save(tmp_path / "narrow.png")
    for bad in ("narrow.png", "colour.png", "absent.png"):
        r = run(str(tmp_path / "bad"), "--gt", "%s,4" % (tmp_path / bad))
        assert r.returncode != 0 and "--gt refused" in r.stdout and not os.path.exists(str(tmp_path / "bad") + ".pfm"), bad
