"""GPU tier: the sparse form of the regular small-ring aggregation launches (k_agg_march<.., SPARSE> + k_agg_apply).  A launch of
that form stores only the outputs whose own record makes a pass change the pixel, and a small kernel behind it copies those back
into the volume the launch read.  The form is chosen per direction from the record density of the PREVIOUS Match of the handle, in
the plain short-arm plan only -- so every case here matches several times on one handle, compares every map bit for bit with the
CPU oracle, and asserts through debug counter 16 that the sparse form really ran (and through counters 2 and 4 that nothing was
redone).  Segments are forced (ADC_AGG_HSEG / ADC_AGG_VSEG = 3) so that the halos between neighbouring waves are exercised."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adcensus_amd as A
from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSEG = 3
SHAPES = [(320, 200, 0, 128), (203, 333, -10, 128), (640, 120, 0, 100)]  # odd width + tall + negative dmin; padding lanes (100 of 128)


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _boundaries(n):
    seg = (n + NSEG - 1) // NSEG
    return [k * seg for k in range(1, NSEG) if k * seg < n]


def planted_pair(w, h, seed, frac=0.03):
    """Noise pair whose left image has `frac` of its pixels copy their left neighbour and another `frac` their upper neighbour, plus
    runs of 2..4 equal pixels across every forced segment boundary (both directions), in the first and last two rows and in the first
    and last two columns: overlapping non-trivial spans, spans that reach into the neighbouring segment's halo, and -- a pixel with a
    vertical arm only -- horizontal records with a support count != 1 but zero arms (and vice versa)."""
    left, right = (a.copy() for a in workloads.noise_pair(w, h, seed=seed))
    rng = np.random.default_rng(seed + 1)
    src = left.copy()
    mh = rng.random((h, w)) < frac
    mh[:, 0] = False
    left[mh] = np.roll(src, 1, axis=1)[mh]
    mv = (rng.random((h, w)) < frac) & ~mh
    mv[0, :] = False
    left[mv] = np.roll(src, 1, axis=0)[mv]
    for b in _boundaries(w):  # horizontal runs across the column boundaries of the row passes' segments
        for y in range(0, h, 5):
            n = 2 + (y // 5) % 3
            x0 = b - 1 - (y // 5) % 2
            left[y, x0:x0 + n] = left[y, x0]
    for b in _boundaries(h):  # vertical runs across the row boundaries of the column passes' segments
        for x in range(0, w, 5):
            n = 2 + (x // 5) % 3
            y0 = b - 1 - (x // 5) % 2
            left[y0:y0 + n, x] = left[y0, x]
    for x in range(3, w - 4, 11):  # first / last two rows: vertical pairs, and horizontal runs inside the border rows
        left[0:2, x] = left[0, x]
        left[h - 2:h, x + 1] = left[h - 1, x + 1]
        left[0, x + 3:x + 6] = left[0, x + 3]
        left[h - 1, x + 3:x + 7] = left[h - 1, x + 3]
    for y in range(3, h - 4, 11):  # first / last two columns
        left[y, 0:2] = left[y, 0]
        left[y + 1, w - 2:w] = left[y + 1, w - 1]
        left[y + 3:y + 6, 0] = left[y + 3, 0]
        left[y + 3:y + 7, w - 1] = left[y + 3, w - 1]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def dense_pair(w, h, seed, p=0.6):
    """Short-arm pair with MANY non-trivial records: every third column's pixel copies its left neighbour with probability p (runs
    of two, so no arm grows beyond what a noise image has) -- about 2 * p / 3 of the pixels then have a horizontal arm, and as many a
    vertical record with a support count != 1."""
    left, right = (a.copy() for a in workloads.noise_pair(w, h, seed=seed))
    rng = np.random.default_rng(seed + 2)
    m = rng.random((h, w)) < p
    m[:, np.arange(w) % 3 != 1] = False
    left[m] = np.roll(left, 1, axis=1)[m]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def _force_segments(monkeypatch):
    monkeypatch.setenv("ADC_AGG_HSEG", str(NSEG))
    monkeypatch.setenv("ADC_AGG_VSEG", str(NSEG))


def _run_alternating(oracle, pairs, w, h, dmin, d, order=(0, 0, 1, 0, 1)):
    opt = pyoracle.Option(min_disparity=dmin, max_disparity=dmin + d)
    want = [oracle.run(l, r, opt, stages=["disp_final", "cost_aggr"]) for l, r in pairs]
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        for n, k in enumerate(order):
            before = st.debug_counter(16)
            got = st.match(*pairs[k])
            assert _same(got, want[k]["disp_final"]), "%dx%d [%d, %d): Match %d (pair %d) differs in %d pixels" % (
                w, h, dmin, dmin + d, n, k, int((got.view(np.uint32) != want[k]["disp_final"].view(np.uint32)).sum()))
            ran = st.debug_counter(16) - before
            print("Match %d: %d sparse launches, densities %d / %d of %d pixels" % (n, ran, st.debug_counter(18), st.debug_counter(19), w * h))
            # the first Match of a handle is dense (full ring); from the second on the three pass pairs run sparse
            assert ran == 0 if n == 0 else ran >= 3, "Match %d: %d sparse launches (%s)" % (n, ran, st.aggregate_kernel())
        assert "SPARSE" in st.aggregate_kernel(), st.aggregate_kernel()
        assert st.debug_counter(2) == 0 and st.debug_counter(4) == 0  # no redo
        # the aggregation stage alone with the pipeline's plan (arms and densities read back, fused cost, pass pairs, and -- the
        # last pass is not moved into the scanline stage here -- a single dividing sparse launch): the aggregated volume itself
        for k, (l, r) in enumerate(pairs):
            before = st.debug_counter(16)
            st.debug_set_images(l, r)
            st.debug_run(A.RUN_GRAY_CENSUS)
            st.debug_run(A.RUN_ARMS)
            st.debug_run(A.RUN_AGGREGATE, 304)
            vol = st.debug_read(A.BUF_VOLUME_A)
            assert st.debug_counter(16) - before >= 4, st.debug_counter(16) - before
            assert _same(vol, want[k]["cost_aggr"]), "cost_aggr of pair %d differs in %d elements" % (
                k, int((vol.view(np.uint32) != want[k]["cost_aggr"].view(np.uint32)).sum()))
    finally:
        st.Release()


@pytest.mark.parametrize("w,h,dmin,d", SHAPES)
def test_sparse_noise_pairs(hip, oracle, monkeypatch, w, h, dmin, d):
    """Case 1: uniform-noise pairs (almost every record trivial), two pairs alternating on one handle."""
    _force_segments(monkeypatch)
    _run_alternating(oracle, [workloads.noise_pair(w, h, seed=9300 + k) for k in range(2)], w, h, dmin, d)


@pytest.mark.parametrize("w,h,dmin,d", SHAPES)
def test_sparse_planted_runs(hip, oracle, monkeypatch, w, h, dmin, d):
    """Case 2: noise with ~3 % + ~3 % planted copies and runs across every segment boundary and along the image border.  These
    images have 13.4 ... 14.0 % of pixels with a non-trivial record (every planted copy makes two pixels non-trivial in its own
    direction and gives both a support count != 1 in the other direction's record): above the committed threshold (10.5 % = half
    of the measured break-even of 21.1 %), so the form is asked for with ADC_AGG_SPARSE_DENSITY, still below the break-even."""
    _force_segments(monkeypatch)
    monkeypatch.setenv("ADC_AGG_SPARSE_DENSITY", "0.2")
    _run_alternating(oracle, [planted_pair(w, h, seed=9400 + k) for k in range(2)], w, h, dmin, d)


def test_sparse_switched_off_is_identical(hip):
    """Case 3: ADC_AGG_SPARSE=0 (own interpreter) gives the same maps pair by pair, and the counter stays 0."""
    code = ("import sys, hashlib; sys.path.insert(0, %r)\n"
            "import adcensus_amd as A\n"
            "from tests import test_gpu_sparse_agg as T\n"
            "st = A.ADCensusStereo(device=0); assert st.Initialize(320, 200, A.ADCensusOption(max_disparity=128))\n"
            "out = []\n"
            "for k in (0, 1, 2, 1):\n"
            "    out.append(hashlib.sha256(st.match(*T.planted_pair(320, 200, seed=555 + k)).tobytes()).hexdigest()[:16])\n"
            "print('DIGESTS', ' '.join(out), 'SPARSE', st.debug_counter(16))\n") % ROOT
    res = {}
    for flag in ("1", "0"):
        env = dict(os.environ, ADC_AGG_SPARSE=flag, ADC_AGG_SPARSE_DENSITY="0.2", ADC_AGG_HSEG=str(NSEG), ADC_AGG_VSEG=str(NSEG))  # (planted pairs: see case 2)
        o = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert o.returncode == 0, o.stdout[-1500:] + o.stderr[-1500:]
        line = [l for l in o.stdout.splitlines() if l.startswith("DIGESTS")][-1].split()
        res[flag] = (line[1:5], int(line[-1]))
    assert res["1"][0] == res["0"][0], res
    assert res["1"][1] >= 9 and res["0"][1] == 0, res


def test_sparse_follows_the_density(hip, oracle, monkeypatch):
    """Case 4: a sparse image, a denser one (record density above the committed threshold, debug counter 17), sparse again.  The
    form of a Match follows the density of the Match BEFORE it: the denser image itself still runs sparse launches (and is exact --
    the choice is never a matter of correctness), its successor runs dense, the one after that sparse again."""
    _force_segments(monkeypatch)
    w, h = 320, 200
    opt = pyoracle.Option(max_disparity=128)
    # (the sparse image is plain noise: its longest arms (1 / 1) and the denser image's (2 / 1) stay within the margin of one entry
    # the ring depth is assumed with, so that no Match of this sequence is redone for its arms)
    imgs = {"s": workloads.noise_pair(w, h, seed=9300), "d": dense_pair(w, h, seed=9501)}
    want = {k: oracle.run(l, r, opt, stages=["disp_final"])["disp_final"] for k, (l, r) in imgs.items()}
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        thr = st.debug_counter(17) * 1e-6 * w * h
        ran = []
        for n, k in enumerate("ssdss"):
            before = st.debug_counter(16)
            got = st.match(*imgs[k])
            assert _same(got, want[k]), "Match %d (%s) differs" % (n, k)
            ran.append(st.debug_counter(16) - before)
            nz = (st.debug_counter(18), st.debug_counter(19))
            print("Match %d (%s): %d sparse launches, densities %s, threshold %.0f pixels" % (n, k, ran[-1], nz, thr))
            assert (max(nz) > thr) == (k == "d"), (k, nz, thr)  # the test's images are on the side of the threshold they are meant to be
        assert ran[0] == 0 and ran[1] >= 3 and ran[2] >= 3 and ran[3] == 0 and ran[4] >= 3, ran
        assert st.debug_counter(2) == 0 and st.debug_counter(4) == 0  # no redo
    finally:
        st.Release()


def test_sparse_not_in_the_two_plan_mode(hip, oracle):
    """Case 5: a stream that alternates between a noise pair and a long-arm pair enters the two-plan mode (debug counter 10); no
    Match that enqueued both plans runs a sparse launch, and every map is exact."""
    w, h = 320, 200
    opt = pyoracle.Option(max_disparity=128)
    pairs = [workloads.noise_pair(w, h, seed=9600), workloads.structured_pair(w, h, 128, seed=9601)]
    want = [oracle.run(l, r, opt, stages=["disp_final"])["disp_final"] for l, r in pairs]
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        for n in range(8):
            k = n % 2
            dual, sparse = st.debug_counter(10), st.debug_counter(16)
            got = st.match(*pairs[k])
            assert _same(got, want[k]), "Match %d (pair %d) differs" % (n, k)
            if st.debug_counter(10) > dual:
                assert st.debug_counter(16) == sparse, "a two-plan Match ran a sparse launch"
        assert st.debug_counter(10) >= 4, st.debug_counter(10)
    finally:
        st.Release()
