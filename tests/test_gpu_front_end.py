"""GPU tier: the pipeline's front end -- k_front (k_cost.hip: one pass over both images = gray, census, packed left image, colour steps,
cost records) and k_sup_records (k_arms.hip: support counts, region boxes and aggregation records from one kernel, transposed records
through an LDS tile).  Only whole Matches run these kernels (the debug stages keep the plain ones), so every test here runs adc_match
through the production path, reads the stage buffers back behind it and compares them -- and the map -- bit for bit with the CPU oracle.

Shapes (W x H, D): the smallest at which the new kernels can go wrong -- 1 x 1; census skipped (W <= 9, H <= 7); partial tiles both
ways and a transposed record tile that is not full; more than two tiles wide with a thin census interior; one pixel past a tile edge
with an odd cell grid."""
import numpy as np
import pytest

import adcensus_amd as A
from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (9, 20, 8), (30, 7, 8), (67, 35, 16), (130, 9, 16), (257, 66, 32)]
STAGES = ["gray_left", "gray_right", "census_left", "census_right", "arms", "sup_count_h", "sup_count_v", "outlier_label", "disp_final"]
BUFFERS = [("gray_left", A.BUF_GRAY_LEFT), ("gray_right", A.BUF_GRAY_RIGHT), ("census_left", A.BUF_CENSUS_LEFT),
           ("census_right", A.BUF_CENSUS_RIGHT), ("arms", A.BUF_ARMS), ("sup_count_h", A.BUF_SUPCOUNT_H),
           ("sup_count_v", A.BUF_SUPCOUNT_V), ("outlier_label", A.BUF_OUTLIER_LABEL)]


def _pair(kind, w, h, d, seed):
    if kind == "noise":
        return workloads.noise_pair(w, h, seed=seed)
    if kind == "structured":  # smooth regions: arms up to the limit, support counts in the hundreds
        return workloads.structured_pair(w, h, d, seed=seed)
    # "coarse": 8 colours instead of 64 -- arms of several pixels in both directions, support counts well above the arm lengths
    return workloads.quantized_noise_pair(w, h, d, seed=seed, levels=128 if kind == "coarse" else 64)


def _bad(got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (g.shape, w.shape, g.dtype, w.dtype)
    if g.dtype.kind == "f":
        g, w = g.view(np.uint32), w.view(np.uint32)
    return int((g != w).sum())


def _check_match(st, pair, want, what):
    """One Match through the production path; the map and every stage buffer behind it against the oracle's."""
    got = st.match(*pair)
    bad = {"disp_final": _bad(got, want["disp_final"])}
    bad["disp_left buffer"] = _bad(st.debug_read(A.BUF_DISP_LEFT), want["disp_final"])
    for name, buf in BUFFERS:
        bad[name] = _bad(st.debug_read(buf), want[name])
    print(what, bad)
    assert not any(bad.values()), (what, {k: v for k, v in bad.items() if v})


@pytest.fixture(scope="module")
def wanted(oracle):
    """Oracle outputs, computed once per (kind, shape, seed) and shared by the tests of this module."""
    cache = {}

    def get(kind, w, h, d, seed, port=None, paper_modes=0):
        key = (kind, w, h, d, seed, paper_modes)
        if key not in cache:
            pair = _pair(kind, w, h, d, seed)
            opt = pyoracle.Option(max_disparity=d)
            if paper_modes:
                out = port.run(pair[0], pair[1], opt, stages=STAGES, paper_modes=paper_modes)
            else:
                out = oracle.run(pair[0], pair[1], opt, stages=STAGES)
            cache[key] = (pair, out)
        return cache[key]

    return get


def _handle(w, h, d):
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(pyoracle.Option(max_disparity=d))), A.last_error()
    return st


@pytest.mark.parametrize("kind", ["noise", "quantized", "coarse"])
@pytest.mark.parametrize("w,h,d", SHAPES)
def test_whole_match_stage_buffers(hip, wanted, kind, w, h, d):
    pair, want = wanted(kind, w, h, d, 4100)
    if kind != "noise" and w * h > 2000:
        assert want["arms"].max() >= (4 if kind == "coarse" else 2) and want["sup_count_h"].max() > 2  # non-trivial records and region boxes
    st = _handle(w, h, d)
    try:
        _check_match(st, pair, want, "%s %dx%d D=%d" % (kind, w, h, d))
        assert st.debug_counter(2) == 0  # (first Match of a handle: full ring, nothing to redo)
    finally:
        st.Release()


@pytest.mark.parametrize("w,h,d", [(67, 35, 16), (257, 66, 32)])
def test_whole_match_long_arms(hip, wanted, w, h, d):
    """Arms far beyond a tile of k_sup_records, in both directions; then a noise pair on the same handle (the redo path behind a
    wrong depth assumption runs the plain kernels) and the long arms again."""
    pair, want = wanted("structured", w, h, d, 4100)
    assert want["arms"][..., :2].max() >= 30 and want["arms"][..., 2:].max() >= 15 and want["sup_count_h"].max() > 300
    st = _handle(w, h, d)
    try:
        _check_match(st, pair, want, "structured %dx%d" % (w, h))
        _check_match(st, *wanted("noise", w, h, d, 4100), "noise behind it")
        _check_match(st, pair, want, "structured again")
    finally:
        st.Release()


@pytest.mark.parametrize("w,h,d", [(67, 35, 16), (257, 66, 32)])
def test_two_pairs_back_to_back(hip, wanted, w, h, d):
    """Different pairs on one handle: a control word that is not cleared (arm maxima, record densities, flags) would carry over."""
    seq = [wanted("quantized", w, h, d, 4100), wanted("noise", w, h, d, 4100), wanted("quantized", w, h, d, 4101), wanted("noise", w, h, d, 4100)]
    st = _handle(w, h, d)
    try:
        for n, (pair, want) in enumerate(seq):
            _check_match(st, pair, want, "Match %d" % n)
    finally:
        st.Release()


def test_match_behind_a_voting_budget_of_one(hip, wanted):
    """A budget of one kernel: the voting chain is continued by adc_wait and the stages behind it are redone."""
    w, h, d = 257, 66, 32
    st = _handle(w, h, d)
    try:
        for n, seed in enumerate((4100, 4101)):
            pair, want = wanted("quantized", w, h, d, seed)
            before = st.debug_counter(1)
            st.debug_set_budget(1)
            _check_match(st, pair, want, "budget 1, Match %d" % n)
            print("continuations:", st.debug_counter(1) - before, "voting (rounds, evaluations):", st.voting_stats())
            if st.voting_stats()[0] > 1:
                assert st.debug_counter(1) == before + 1, "the continuation path was not taken"
    finally:
        st.Release()


def test_match_behind_a_forced_median_fallback(hip, wanted):
    w, h, d = 257, 66, 32
    st = _handle(w, h, d)
    try:
        for n, kind in enumerate(("noise", "quantized")):
            pair, want = wanted(kind, w, h, d, 4100)
            before = st.debug_counter(0)
            st.debug_run(A.RUN_MEDIAN, 100)
            _check_match(st, pair, want, "median fallback, Match %d" % n)
            assert st.debug_counter(0) == before + 1, "the fallback path was not taken"
    finally:
        st.Release()


def test_paper_mode_takes_the_plain_kernels(hip, wanted, port_oracle):
    """Paper mode on (plain kernels), off (fused), on again: each Match against the oracle run with the same modes."""
    w, h, d = 67, 35, 16
    st = _handle(w, h, d)
    try:
        for n, modes in enumerate((A.PAPER_CENSUS5X5, 0, A.PAPER_RIGHT_ARMS, 0)):
            st.set_paper_modes(modes)
            pair, want = wanted("quantized", w, h, d, 4100 + (n & 1), port=port_oracle, paper_modes=modes)
            _check_match(st, pair, want, "paper modes %d, Match %d" % (modes, n))
    finally:
        st.Release()
