"""GPU tier: the two ends of the short-arm aggregation plan.

k_cost_agg_flat (k_cost.hip) -- the first launch (fused cost, horizontal, non-dividing) as an element-wise kernel in place of the
small-ring march, from the second Match of a handle on, where the horizontal record density the handle last saw is low.  Both forms
give the same bits, so every case matches several times on one handle, compares every map (and the aggregated volume, through the
debug surface with the pipeline's plan) bit for bit with the CPU oracle, and asserts through debug counter 22 (flat launches) that the
form really ran -- or did not -- and through counters 2 and 4 that nothing was redone unless the case is about the redo.

The fused tail (k_scanline_seg_agg): the last aggregation pass inside the L->R scanline pass evaluates the sum and the division only
where the record asks for them; images with runs at the row ends, across every segment start and its warm-up, and with records whose
arms are 0 but whose divisor is not 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adcensus_amd as A
from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases, gather_patterns
from tests.test_gpu_sparse_agg import planted_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# D = 128; negative dmin + padding lanes (100 of 128); positive dmin + two 128-float chunks; an odd width with a tile remainder of 65
GEOMETRIES = [(160, 48, 0, 128), (203, 40, -10, 100), (130, 33, 5, 256), (321, 37, 0, 128)]
FLAT, GATHER = 22, 20


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _ndiff(a, b):
    return int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).sum())


def _aggregate(st, pair):
    """The aggregation stage alone with the pipeline's plan (fused cost, arms and densities of THIS image read back): cost_aggr."""
    st.debug_set_images(*pair)
    st.debug_run(A.RUN_GRAY_CENSUS)
    st.debug_run(A.RUN_ARMS)
    st.debug_run(A.RUN_AGGREGATE, 304)
    return st.debug_read(A.BUF_VOLUME_A)


@pytest.mark.parametrize("w,h,dmin,d", GEOMETRIES)
def test_flat_first_launch(hip, oracle, monkeypatch, w, h, dmin, d):
    """Two noise pairs and a planted pair (runs of 2..4 at the row ends, ~13 % of the records change a pixel) alternate on one handle.
    The forms are asked for up to a density of 0.2 so that the Match after the planted pair runs flat too."""
    monkeypatch.setenv("ADC_AGG_SPARSE_DENSITY", "0.2")
    monkeypatch.setenv("ADC_AGG_GATHER_DENSITY", "0.2")
    monkeypatch.setenv("ADC_COST_FLAT_DENSITY", "0.2")
    # (the noise pairs have arms of 1, the planted one of up to 4: the depth assumed from a noise pair has to cover it -- no redo here)
    monkeypatch.setenv("ADC_AGG_ASSUME_MARGIN", "3")
    opt = pyoracle.Option(min_disparity=dmin, max_disparity=dmin + d)
    pairs = [workloads.noise_pair(w, h, seed=9900), workloads.noise_pair(w, h, seed=9901), planted_pair(w, h, seed=9902)]
    want = [oracle.run(l, r, opt, stages=["disp_final", "cost_aggr"]) for l, r in pairs]
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        for n, k in enumerate((0, 2, 1, 2)):
            f0 = st.debug_counter(FLAT)
            got = st.match(*pairs[k])
            ran = st.debug_counter(FLAT) - f0
            print("Match %d (pair %d): %d flat launches, horizontal density %d of %d pixels, threshold %d ppm" % (
                n, k, ran, st.debug_counter(18), w * h, st.debug_counter(23)))
            assert _same(got, want[k]["disp_final"]), "%dx%d [%d, %d): Match %d (pair %d) differs in %d pixels" % (
                w, h, dmin, dmin + d, n, k, _ndiff(got, want[k]["disp_final"]))
            assert ran == (0 if n == 0 else 1), (n, ran)  # never the first Match of a handle; one launch for one launch
        assert st.debug_counter(FLAT) >= 2
        assert st.debug_counter(2) == 0 and st.debug_counter(4) == 0  # no redo
        vols = []
        for k, pair in enumerate(pairs):
            f0 = st.debug_counter(FLAT)
            vols.append(_aggregate(st, pair))
            assert st.debug_counter(FLAT) - f0 == 1
            assert _same(vols[k], want[k]["cost_aggr"]), "cost_aggr of pair %d differs in %d elements" % (k, _ndiff(vols[k], want[k]["cost_aggr"]))
        # the march in the same process (the switch is read per call): identical volumes, no flat launch
        monkeypatch.setenv("ADC_COST_FLAT", "0")
        f0, g0 = st.debug_counter(FLAT), st.debug_counter(GATHER)
        for k, pair in enumerate(pairs):
            assert _same(_aggregate(st, pair), vols[k]), k
        assert st.debug_counter(FLAT) == f0 and st.debug_counter(GATHER) > g0
        monkeypatch.delenv("ADC_COST_FLAT")
        # a density above the flat threshold selects the march, whatever the other forms do
        monkeypatch.setenv("ADC_COST_FLAT_DENSITY", "0.000001")
        assert st.debug_counter(23) == 1
        g0 = st.debug_counter(GATHER)
        for k in (0, 1, 0):
            got = st.match(*pairs[k])
            assert _same(got, want[k]["disp_final"]), k
        assert st.debug_counter(FLAT) == f0 and st.debug_counter(GATHER) > g0 and st.debug_counter(18) > 1e-6 * w * h
        assert st.debug_counter(2) == 0 and st.debug_counter(4) == 0
    finally:
        st.Release()


def test_flat_launch_keeps_the_depth_gate(hip, oracle):
    """Noise, then a pair whose only long arms are horizontal (runs of 6 equal pixels along a row: arms of 5 against an assumed depth
    of 2), then noise again.  The flat launch must skip and raise the too-shallow flag exactly like the march it replaces, so the
    middle Match is redone once (debug counter 2) and comes out exact; the Matches around it are not redone."""
    w, h = 320, 64
    opt = pyoracle.Option(max_disparity=128)
    pairs = [workloads.noise_pair(w, h, seed=9930), gather_patterns.run_pair(w, h, seed=9931, vertical=False, lengths=(6,)),
             workloads.noise_pair(w, h, seed=9932)]
    want = [oracle.run(l, r, opt, stages=["disp_final", "arms"]) for l, r in pairs]
    arms = [gather_patterns.arm_maxima(o["arms"]) for o in want]
    assert arms[1][0] >= 5 and arms[0][0] <= 2, arms  # a horizontal arm beyond the depth the noise pair lets assume
    assert arms[1][1] <= arms[0][1] + 1, arms          # ... while the vertical arms stay within theirs
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        redos, flats = [], []
        for n in range(3):
            r0, f0 = st.debug_counter(2), st.debug_counter(FLAT)
            got = st.match(*pairs[n])
            assert _same(got, want[n]["disp_final"]), "Match %d differs in %d pixels" % (n, _ndiff(got, want[n]["disp_final"]))
            redos.append(st.debug_counter(2) - r0)
            flats.append(st.debug_counter(FLAT) - f0)
            print("Match %d: arms %s, %d redos, %d flat launches" % (n, arms[n], redos[-1], flats[-1]))
        assert redos == [0, 1, 0], redos
        assert flats[:2] == [0, 1], flats  # the skipped plan of the middle Match was the flat one; a redo itself never runs flat
        assert st.debug_counter(4) == 0
    finally:
        st.Release()


def test_flat_not_in_the_two_plan_mode(hip, oracle):
    """A stream that alternates between a noise pair and a long-arm pair enters the two-plan mode (debug counter 10); no Match that
    enqueued both plans runs a flat launch, and every map is exact."""
    w, h = 320, 64
    opt = pyoracle.Option(max_disparity=128)
    pairs = [workloads.noise_pair(w, h, seed=9940), workloads.structured_pair(w, h, 128, seed=9941)]
    want = [oracle.run(l, r, opt, stages=["disp_final"])["disp_final"] for l, r in pairs]
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        for n in range(8):
            k = n % 2
            dual, f0 = st.debug_counter(10), st.debug_counter(FLAT)
            got = st.match(*pairs[k])
            assert _same(got, want[k]), "Match %d (pair %d) differs" % (n, k)
            if n == 0 or st.debug_counter(10) > dual:
                assert st.debug_counter(FLAT) == f0, "Match %d ran a flat launch" % n
        assert st.debug_counter(10) >= 4, st.debug_counter(10)
    finally:
        st.Release()


# ------------------------------------------------------------------------------------------------------------------ fused tail
def _seg_start(plen, nseg, warm, s):  # adc_so_seg_start (adc_device_fn.h)
    if s <= 0:
        return 0
    if s >= nseg:
        return plen
    t = (plen + (nseg - 1) * (warm + 1) + nseg - 1) // nseg
    return ((t + (s - 1) * (t - warm - 1)) & ~3) + 1


def _segments(w, h, warm=64):  # adc_so_segments / adc_so_seg_ok (k_scanline.hip, adc_device_fn.h), automatic choice
    def ok(n):
        return all(_seg_start(w, n, warm, s) - _seg_start(w, n, warm, s - 1) >= 32 + (warm + 1 if s == 1 else 0) for s in range(1, n + 1))
    n = (2048 + h // 2) // h
    if n == 2 and 3 * h <= 4096:
        n = 3
    n = min(n, 8)
    while n >= 2 and not ok(n):
        n -= 1
    return n if n >= 2 else 1


def tail_pair(w, h, seed):
    """Noise pair for the fused tail: horizontal runs of 2..5 equal pixels that start at x = 0, end at x = W - 1 and straddle every
    segment start and the first element of its 65-element warm-up (at every offset of the run against the boundary), plus vertical runs
    of 2..3 (records with arms 0 / 0 and a divisor > 1)."""
    left, right = (a.copy() for a in workloads.noise_pair(w, h, seed=seed))
    nseg = _segments(w, h)
    marks = []
    for s in range(1, nseg):
        a = _seg_start(w, nseg, 64, s)
        marks += [a, a - 65]
    y = 1
    for n in (2, 3, 4, 5):
        left[y, 0:n] = left[y, 0]
        left[y + 1, w - n:w] = left[y + 1, w - 1]
        y += 2
    rows = iter(range(y, h - 4))
    for n in (2, 3, 4, 5):
        for off in range(1, n):  # the run covers mark - off .. mark - off + n - 1: elements on both sides of the mark
            yy = next(rows)
            for m in marks:
                left[yy, m - off:m - off + n] = left[yy, m - off]
    for x in range(7, w - 2, 9):  # vertical runs in the last rows
        n = 2 + (x // 9) % 2
        left[h - 1 - n:h - 1, x] = left[h - 2, x]
    return np.ascontiguousarray(left), np.ascontiguousarray(right), nseg


@pytest.mark.parametrize("w,h", [(160, 40), (320, 40)])
def test_fused_tail_runs_at_ends_seams_and_warmups(hip, oracle, w, h):
    """In an interpreter of its own with ADC_SO_FAST=0 (small images then take the fused form): maps and cost_so bit for bit.  The
    fused form takes assumed depths up to 4 and these pairs have arms of 4, so the depth is assumed without a margin."""
    opt = pyoracle.Option(max_disparity=128)
    pairs = [tail_pair(w, h, seed=9950 + k) for k in range(2)]
    nseg = pairs[0][2]
    assert nseg >= 2
    for l, r, _ in pairs:
        o = oracle.run(l, r, opt, stages=["arms", "sup_count_v"])
        ah = gather_patterns.arm_maxima(o["arms"])[0]
        assert ah == 4, ah
        assert o["arms"][:, 0, 1].max() == 4 and o["arms"][:, w - 1, 0].max() == 4
        for s in range(1, nseg):
            for m in (_seg_start(w, nseg, 64, s), _seg_start(w, nseg, 64, s) - 65):
                assert o["arms"][:, m, 0].max() >= 1 and o["arms"][:, m, 1].max() >= 1 and o["arms"][:, m - 1, 1].max() >= 1, (s, m)
        zero = (o["arms"][..., 0] == 0) & (o["arms"][..., 1] == 0)
        assert (zero & (o["sup_count_v"] > 1)).sum() >= 5  # arms 0 / 0, divisor > 1 (the count of the dividing H pass)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "import adcensus_amd as A\n"
            "from oracle import pyoracle\n"
            "from tests import cases, test_gpu_cost_flat as T\n"
            "orc = pyoracle.load('auto')\n"
            "w, h = %d, %d\n"
            "opt = pyoracle.Option(max_disparity=128)\n"
            "pairs = [T.tail_pair(w, h, seed=9950 + k)[:2] for k in range(2)]\n"
            "want = [orc.run(l, r, opt, stages=['disp_final', 'cost_so']) for l, r in pairs]\n"
            "st = A.ADCensusStereo(device=0)\n"
            "assert st.Initialize(w, h, cases.to_product_option(opt))\n"
            "bad = []\n"
            "for n, k in enumerate((0, 1, 0, 1)):\n"
            "    f0 = st.debug_counter(13)\n"
            "    d = st.match(*pairs[k])\n"
            "    vol = st.debug_read(A.BUF_VOLUME_A)\n"
            "    nd = int((d.view(np.uint32) != want[k]['disp_final'].view(np.uint32)).sum())\n"
            "    nv = int((vol.view(np.uint32) != want[k]['cost_so'].view(np.uint32)).sum())\n"
            "    print('MATCH', n, k, 'fused', st.debug_counter(13) - f0, 'segments', st.debug_counter(5), 'disp', nd, 'cost_so', nv)\n"
            "    if nd or nv: bad.append((n, k, nd, nv))\n"
            "print('BAD', bad, 'FUSED', st.debug_counter(13), 'SEAM_REDOS', st.debug_counter(4), 'REDOS', st.debug_counter(2), 'SEGMENTS', st.debug_counter(5))\n"
            "ok = not bad and st.debug_counter(13) >= 3 and st.debug_counter(4) == 0 and st.debug_counter(2) == 0 and st.debug_counter(5) == %d\n"
            "st.Release()\n"
            "sys.exit(0 if ok else 1)\n") % (ROOT, w, h, nseg)
    o = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ADC_SO_FAST="0", ADC_AGG_ASSUME_MARGIN="0"), capture_output=True, text=True, timeout=600)
    print(o.stdout[-3000:])
    assert o.returncode == 0, o.stdout[-3000:] + o.stderr[-3000:]
