"""GPU tier: the gather form of the sparse small-ring aggregation launches (k_agg_gather + k_agg_apply).  Where the record density
the handle last saw is low enough, a sparse launch no longer marches over the whole volume: it computes only the pixels whose own
record makes the pass change them, each from the input vectors of its span.  Every form gives the same bits, so every case here
matches several times on one handle, compares every map bit for bit with the CPU oracle, and asserts through debug counter 20
(gather launches; they also count as sparse launches, counter 16) that the form really ran, and through counters 2 and 4 that
nothing was redone unless the case is about the redo."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adcensus_amd as A
from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases, gather_patterns
from tests.test_gpu_sparse_agg import planted_pair, dense_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the shapes of the sparse tests (odd width + tall + negative dmin; padding lanes) + one with two 128-float chunks per pixel (Dp = 256)
SHAPES = [(320, 200, 0, 128), (203, 333, -10, 128), (640, 120, 0, 100), (160, 96, 0, 200)]
GATHER, SPARSE = 20, 16


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _ndiff(a, b):
    return int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).sum())


def _run_alternating(oracle, pairs, w, h, dmin, d, order=(0, 0, 1, 0, 1)):
    opt = pyoracle.Option(min_disparity=dmin, max_disparity=dmin + d)
    want = [oracle.run(l, r, opt, stages=["disp_final", "cost_aggr"]) for l, r in pairs]
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        for n, k in enumerate(order):
            g0, s0 = st.debug_counter(GATHER), st.debug_counter(SPARSE)
            got = st.match(*pairs[k])
            ran, sparse = st.debug_counter(GATHER) - g0, st.debug_counter(SPARSE) - s0
            print("Match %d: %d gather of %d sparse launches, densities %d / %d of %d pixels, threshold %d ppm" % (
                n, ran, sparse, st.debug_counter(18), st.debug_counter(19), w * h, st.debug_counter(21)))
            assert _same(got, want[k]["disp_final"]), "%dx%d [%d, %d): Match %d (pair %d) differs in %d pixels" % (
                w, h, dmin, dmin + d, n, k, _ndiff(got, want[k]["disp_final"]))
            # the first Match of a handle is dense (full ring); from the second on the three pass pairs gather
            assert ran == 0 if n == 0 else ran >= 3, "Match %d: %d gather launches (%s)" % (n, ran, st.aggregate_kernel())
            assert sparse >= ran
        assert "SPARSE" in st.aggregate_kernel() and "k_agg_gather" in st.aggregate_kernel(), st.aggregate_kernel()
        assert st.debug_counter(2) == 0 and st.debug_counter(4) == 0  # no redo
        # the aggregation stage alone with the pipeline's plan: the last pass is not moved into the scanline stage here, so a single
        # dividing gather launch (the non-pair DIVIDE form) runs behind the three pairs; the aggregated volume itself
        for k, (l, r) in enumerate(pairs):
            g0 = st.debug_counter(GATHER)
            st.debug_set_images(l, r)
            st.debug_run(A.RUN_GRAY_CENSUS)
            st.debug_run(A.RUN_ARMS)
            st.debug_run(A.RUN_AGGREGATE, 304)
            vol = st.debug_read(A.BUF_VOLUME_A)
            assert st.debug_counter(GATHER) - g0 >= 4, st.debug_counter(GATHER) - g0
            assert _same(vol, want[k]["cost_aggr"]), "cost_aggr of pair %d differs in %d elements" % (k, _ndiff(vol, want[k]["cost_aggr"]))
    finally:
        st.Release()


@pytest.mark.parametrize("w,h,dmin,d", SHAPES)
def test_gather_noise_pairs(hip, oracle, w, h, dmin, d):
    """Case 1: uniform-noise pairs (1-2 % of the records change a pixel), two pairs alternating on one handle, compiled-in thresholds."""
    _run_alternating(oracle, [workloads.noise_pair(w, h, seed=9800 + k) for k in range(2)], w, h, dmin, d)


@pytest.mark.parametrize("w,h,dmin,d", SHAPES)
def test_gather_planted_runs(hip, oracle, monkeypatch, w, h, dmin, d):
    """Case 2: noise with ~3 % + ~3 % planted copies, runs of 2..4 across the former segment boundaries and along the image border
    (tests/test_gpu_sparse_agg.py: planted_pair): 13-14 % of the pixels have a pass-changing record, spans overlap each other, so
    neighbouring changed pixels read the same input vectors.  Both forms are asked for up to a density of 0.2."""
    monkeypatch.setenv("ADC_AGG_SPARSE_DENSITY", "0.2")
    monkeypatch.setenv("ADC_AGG_GATHER_DENSITY", "0.2")
    _run_alternating(oracle, [planted_pair(w, h, seed=9810 + k) for k in range(2)], w, h, dmin, d)


def test_gather_switched_off_is_identical(hip):
    """Case 2, second half: the same planted pairs with ADC_AGG_GATHER=0 in an interpreter of their own give the same maps pair by
    pair, run sparse launches, and the gather counter stays 0."""
    code = ("import sys, hashlib; sys.path.insert(0, %r)\n"
            "import adcensus_amd as A\n"
            "from tests import test_gpu_sparse_agg as T\n"
            "st = A.ADCensusStereo(device=0); assert st.Initialize(320, 200, A.ADCensusOption(max_disparity=128))\n"
            "out = []\n"
            "for k in (0, 1, 2, 1):\n"
            "    out.append(hashlib.sha256(st.match(*T.planted_pair(320, 200, seed=9810 + k)).tobytes()).hexdigest()[:16])\n"
            "print('DIGESTS', ' '.join(out), 'COUNTERS', st.debug_counter(16), st.debug_counter(20))\n") % ROOT
    res = {}
    for flag in ("1", "0"):
        env = dict(os.environ, ADC_AGG_GATHER=flag, ADC_AGG_SPARSE_DENSITY="0.2", ADC_AGG_GATHER_DENSITY="0.2")
        o = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert o.returncode == 0, o.stdout[-1500:] + o.stderr[-1500:]
        line = [l for l in o.stdout.splitlines() if l.startswith("DIGESTS")][-1].split()
        res[flag] = (line[1:5], int(line[-2]), int(line[-1]))
    assert res["1"][0] == res["0"][0], res
    assert res["1"][1] >= 9 and res["1"][2] >= 9, res
    assert res["0"][1] >= 9 and res["0"][2] == 0, res


def test_gather_arms_up_to_the_small_ring_limit(hip, oracle, monkeypatch):
    """Case 3: runs of 6..9 equal pixels in both directions: arms reach 8 = the small-ring limit, spans of up to 17 vectors whose
    pixels' own spans reach 16 places away.  The last pass does not move into the scanline stage (depth > 4), so a Match itself runs
    a single dividing gather launch behind the three pairs.  The second Match assumes the depth the first one saw: no redo.  (These
    images have 8-9 % of pass-changing records; the forms are asked for up to 0.2 so that the case does not depend on the thresholds.)"""
    monkeypatch.setenv("ADC_AGG_SPARSE_DENSITY", "0.2")
    monkeypatch.setenv("ADC_AGG_GATHER_DENSITY", "0.2")
    w, h = 320, 200
    opt = pyoracle.Option(max_disparity=128)
    pairs = [gather_patterns.run_pair(w, h, seed=9820 + k) for k in range(2)]
    want = [oracle.run(l, r, opt, stages=["disp_final", "arms"]) for l, r in pairs]
    for o in want:
        ah, av = gather_patterns.arm_maxima(o["arms"])
        assert 5 <= ah <= 8 and 5 <= av <= 8 and max(ah, av) == 8, (ah, av)  # the images are what the case is about
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        for n in range(2):
            g0 = st.debug_counter(GATHER)
            got = st.match(*pairs[n])
            assert _same(got, want[n]["disp_final"]), "Match %d differs in %d pixels" % (n, _ndiff(got, want[n]["disp_final"]))
            ran = st.debug_counter(GATHER) - g0
            print("Match %d: %d gather launches, densities %d / %d of %d (%s)" % (n, ran, st.debug_counter(18), st.debug_counter(19), w * h, st.aggregate_kernel()))
            assert ran == 0 if n == 0 else ran >= 4, ran
        assert st.debug_counter(2) == 0 and st.debug_counter(4) == 0 and st.debug_counter(13) == 0  # no redo, no fused tail
    finally:
        st.Release()


def test_gather_launch_keeps_the_depth_gate(hip, oracle):
    """Case 4: noise, then a pair whose only long arms are vertical (runs of 6 equal pixels down a column: arms of 5 against an
    assumed depth of 2), then noise again.  In the short-arm plan the vertical pair launches are the only kernels that verify the
    assumed vertical depth -- the gather kernel must skip and flag exactly like the march it replaces, so the middle Match is redone
    once (debug counter 2) and comes out exact; the Matches around it are not redone."""
    w, h = 320, 200
    opt = pyoracle.Option(max_disparity=128)
    pairs = [workloads.noise_pair(w, h, seed=9830), gather_patterns.run_pair(w, h, seed=9831, horizontal=False, lengths=(6,)),
             workloads.noise_pair(w, h, seed=9832)]
    want = [oracle.run(l, r, opt, stages=["disp_final", "arms"]) for l, r in pairs]
    arms = [gather_patterns.arm_maxima(o["arms"]) for o in want]
    assert arms[1][1] >= 5 and arms[0][1] <= 2, arms                      # a vertical arm beyond the depth the noise pair lets assume
    assert arms[1][0] <= arms[0][0] + 1, arms                              # ... while the horizontal arms stay within theirs
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        redos = []
        for n in range(3):
            r0, g0 = st.debug_counter(2), st.debug_counter(GATHER)
            got = st.match(*pairs[n])
            assert _same(got, want[n]["disp_final"]), "Match %d differs in %d pixels" % (n, _ndiff(got, want[n]["disp_final"]))
            redos.append(st.debug_counter(2) - r0)
            print("Match %d: arms %s, %d redos, %d gather launches" % (n, arms[n], redos[-1], st.debug_counter(GATHER) - g0))
            if n == 1:
                assert st.debug_counter(GATHER) - g0 >= 3  # the skipped plan was the gather one (a redo itself never gathers)
        assert redos == [0, 1, 0], redos
        assert st.debug_counter(4) == 0
    finally:
        st.Release()


def test_gather_follows_the_density(hip, oracle):
    """Case 5a: a sparse image, a denser one (above both thresholds), sparse again: the Match AFTER the dense image runs no gather
    launch (and no sparse one), the one after that gathers again."""
    w, h = 320, 200
    opt = pyoracle.Option(max_disparity=128)
    imgs = {"s": workloads.noise_pair(w, h, seed=9300), "d": dense_pair(w, h, seed=9501)}
    want = {k: oracle.run(l, r, opt, stages=["disp_final"])["disp_final"] for k, (l, r) in imgs.items()}
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        thr = st.debug_counter(21) * 1e-6 * w * h
        assert st.debug_counter(21) <= st.debug_counter(17)
        ran = []
        for n, k in enumerate("ssdss"):
            g0 = st.debug_counter(GATHER)
            got = st.match(*imgs[k])
            assert _same(got, want[k]), "Match %d (%s) differs" % (n, k)
            ran.append(st.debug_counter(GATHER) - g0)
            nz = (st.debug_counter(18), st.debug_counter(19))
            assert (max(nz) > thr) == (k == "d"), (k, nz, thr)
        assert ran[0] == 0 and ran[1] >= 3 and ran[2] >= 3 and ran[3] == 0 and ran[4] >= 3, ran
        assert st.debug_counter(2) == 0 and st.debug_counter(4) == 0
    finally:
        st.Release()


def test_gather_not_in_the_two_plan_mode(hip, oracle):
    """Case 5b: a stream that alternates between a noise pair and a long-arm pair enters the two-plan mode (debug counter 10); no
    Match that enqueued both plans runs a gather launch, and every map is exact."""
    w, h = 320, 200
    opt = pyoracle.Option(max_disparity=128)
    pairs = [workloads.noise_pair(w, h, seed=9600), workloads.structured_pair(w, h, 128, seed=9601)]
    want = [oracle.run(l, r, opt, stages=["disp_final"])["disp_final"] for l, r in pairs]
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        for n in range(8):
            k = n % 2
            dual, g0 = st.debug_counter(10), st.debug_counter(GATHER)
            got = st.match(*pairs[k])
            assert _same(got, want[k]), "Match %d (pair %d) differs" % (n, k)
            if st.debug_counter(10) > dual:
                assert st.debug_counter(GATHER) == g0, "a two-plan Match ran a gather launch"
        assert st.debug_counter(10) >= 4, st.debug_counter(10)
    finally:
        st.Release()
