"""GPU tier: arm limits far above the default cross_L1 = 34, on flat-patch images whose arms do reach the limit (tests/cases.py:
flat_patch_pair).  Every arm limit up to the reference's MAX_ARM_LENGTH = 255 runs on the LDS marching ring (up to 511 entries),
the voting chain runs without slack budgets above an arm limit of 48 (irv_plan.h: IRV_SLACK_MAX_ARM), and a handle whose
images alternate between short and long arms assumes, verifies and redoes the ring depth.  Bit for bit against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG_VOTING_CASES = ["flat_640x96_L48", "flat_640x96_L49", "flat_640x96_L64", "flat_640x96_L128", "flat_640x96_L255",
                     "flat_560x320_L255", "flat_200x64_L255"]


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("slack", ["0", "1"])
def test_long_arm_voting_stage_with_and_without_slack(hip, slack):
    """The voting stage in isolation (oracle's LR-checked map, labels, arms and support counts in) on the long-arm cases, with the
    slack budgets switched off (ADC_IRV_SLACK=0) and at the default.  The switch is read once per process: each setting runs in
    its own interpreter."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "import adcensus_amd as A\n"
            "from tests import cases\n"
            "from oracle import pyoracle\n"
            "bad = []\n"
            "for name in %r:\n"
            "    l, r, opt = cases.make_case(name)\n"
            "    o = pyoracle.load('auto').run(l, r, opt)\n"
            "    h, w = l.shape[:2]\n"
            "    st = A.ADCensusStereo(device=0)\n"
            "    assert st.Initialize(w, h, cases.to_product_option(opt)), name\n"
            "    st.debug_set_images(l, r)\n"
            "    st.debug_write(A.BUF_ARMS, o['arms'])\n"
            "    st.debug_write(A.BUF_SUPCOUNT_H, o['sup_count_h'])\n"
            "    st.debug_write(A.BUF_DISP_LEFT, o['disp_after_lr'])\n"
            "    st.debug_write(A.BUF_OUTLIER_LABEL, o['outlier_label'])\n"
            "    st.debug_run(A.RUN_REGION_VOTING)\n"
            "    got = np.asarray(st.debug_read(A.BUF_DISP_LEFT)).view(np.uint32)\n"
            "    n = int((got != o['disp_after_irv'].view(np.uint32)).sum())\n"
            "    changed = int((o['disp_after_irv'].view(np.uint32) != o['disp_after_lr'].view(np.uint32)).sum())\n"
            "    print(name, 'voting changes', changed, 'rounds/evals', st.voting_stats(), 'differing', n)\n"
            "    if n: bad.append((name, n))\n"
            "    st.Release()\n"
            "print('FAILING', bad)\n"
            "sys.exit(1 if bad else 0)\n") % (ROOT, LONG_VOTING_CASES)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ADC_IRV_SLACK=slack), capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]


@pytest.mark.parametrize("height", [1, 8])
def test_voting_slack_window_guard_on_a_constructed_region(hip, height):
    """The constructed input of tests/cases.py: slack_window_voting_input (the decisive fills of a vote lie past the 128 columns the
    slack count reads per row) through the voting stage of a handle with arm limit 255: the reference's region voting, bit for bit.
    With the budgets on above arm limit 48 (the kernel before irv_slack_mode) the uncounted fills leave pixel 0 unfilled whenever
    it is evaluated before them (the CPU emulation's fixed order: tests/test_emul.py); the device's schedule mostly lets it see
    them.  On hardware the budgets' undercount showed on flat_640x96_L128_L2zero (voting stage, STAGE_CASES)."""
    A = hip
    disp, label, arms, sup_h, opt = cases.slack_window_voting_input(height=height)
    want = cases.region_voting_reference(disp, label, arms, opt)
    h, w = disp.shape
    left = np.zeros((h, w, 3), np.uint8)
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        st.debug_set_images(left, left)
        st.debug_write(A.BUF_ARMS, arms)
        st.debug_write(A.BUF_SUPCOUNT_H, sup_h)
        st.debug_write(A.BUF_DISP_LEFT, disp)
        st.debug_write(A.BUF_OUTLIER_LABEL, label)
        st.debug_run(A.RUN_REGION_VOTING)
        got = np.asarray(st.debug_read(A.BUF_DISP_LEFT))
    finally:
        st.Release()
    assert _same(got, want), (got[:, :3], want[:, :3], int((got.view(np.uint32) != want.view(np.uint32)).sum()))


@pytest.mark.parametrize("dual", ["0", None])
def test_short_long_short_arms_on_one_handle(hip, oracle, monkeypatch, dual):
    """One handle with cross_L1 = cross_L2 = 255: short-arm pairs (uniform noise), long-arm pairs (flat patches: arms of 255),
    then short-arm pairs again.  A long-arm image while the small ring is assumed is detected on the device and redone
    (ADC_AGG_DUAL=0: one plan; default: the two plans of a mixed stream, chosen on the device).  Every Match bit-exact."""
    A = hip
    from oracle import pyoracle
    from adcensus_amd import workloads
    if dual is not None:
        monkeypatch.setenv("ADC_AGG_DUAL", dual)
    w, h, d = 640, 96, 32
    opt = pyoracle.Option(max_disparity=d, cross_L1=255, cross_L2=255)
    pairs = {"n": workloads.noise_pair(w, h, seed=61), "f": cases.flat_patch_pair(w, h, d, seed=62),
             "f2": cases.flat_patch_pair(w, h, d, seed=63)}
    want = {k: oracle.run(v[0], v[1], opt, stages=["disp_final"])["disp_final"] for k, v in pairs.items()}
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        assert _same(st.match(*pairs["n"]), want["n"])     # first Match: nothing known, full ring (511 entries)
        assert _same(st.match(*pairs["n"]), want["n"])     # short arms: the small ring is assumed from now on
        redo0 = st.debug_counter(2)
        assert _same(st.match(*pairs["n"]), want["n"])
        assert st.debug_counter(2) == redo0                # (the assumption holds)
        assert _same(st.match(*pairs["f"]), want["f"])     # arms of 255 while short arms are assumed: detected on the device, redone
        assert st.debug_counter(2) == redo0 + 1, (st.debug_counter(2), redo0)
        assert _same(st.match(*pairs["f2"]), want["f2"])
        assert _same(st.match(*pairs["f"]), want["f"])
        redo1 = st.debug_counter(2)
        assert redo1 == redo0 + 1, (redo1, redo0)          # (long arms after long arms: the full ring is assumed)
        assert _same(st.match(*pairs["n"]), want["n"])     # short arms after long arms: the full ring stays valid, no redo
        assert _same(st.match(*pairs["n"]), want["n"])
        assert st.debug_counter(2) == redo1, (st.debug_counter(2), redo1)
        assert _same(st.match(*pairs["f2"]), want["f2"])   # long again: one plan -> a second redo; two plans -> chosen on the device
        assert st.debug_counter(2) == redo1 + (1 if dual == "0" else 0), (st.debug_counter(2), redo1, dual)
        assert _same(st.match(*pairs["n"]), want["n"])
    finally:
        st.Release()


@pytest.mark.parametrize("name", ["wrap0_320x288_d16", "wrap_320x320_d8"])
def test_wrapped_support_counts_through_aggregation(hip, oracle, name):
    """Regions of more than 65535 pixels wrap the reference's 16-bit support counts (cross_aggregator.h:101); a count of 0 makes the
    aggregation divide give inf (x / 0) and NaN (0 / 0: 0xFFC00000 on the reference's x86 build).  Every stage up to the aggregated
    volume, all four aggregation launch forms, must match bit for bit, NaN encodings included.  (The scanline stage does not yet
    reproduce the reference's NaN / inf ordering of std::min on such volumes: not asserted here.)"""
    left, right, opt = cases.make_case(name)
    o = oracle.run(left, right, opt)
    assert np.isnan(o["cost_aggr"]).any() and np.isinf(o["cost_aggr"]).any()
    from tests import gpu_harness
    rep = gpu_harness.stage_report(left, right, opt, o)
    pinned = ("gray_", "census_", "cost_init", "arms", "sup_count_", "cost_aggr")
    bad = {k: v for k, v in gpu_harness.failing(rep).items() if k.startswith(pinned)}
    assert all(k in rep for k in ("cost_aggr", "cost_aggr(fused cost)", "cost_aggr(fused cost + pass pairs)", "cost_aggr(pass pairs)"))
    assert not bad, "%s (oracle=%s): %s" % (name, oracle.kind, bad)


@pytest.mark.xfail(strict=True, reason="the scanline minima (v_min_f32 / fminf) drop NaN operands where the reference's std::min(a, b) "
                   "keeps a NaN first operand (scanline_optimizer.cpp:150-154): cost_so differs on volumes with wrapped support counts")
@pytest.mark.parametrize("name", ["wrap0_320x288_d16", "wrap_320x320_d8"])
def test_wrapped_support_counts_scanline_and_match(hip, oracle, name):
    """Known gap, kept visible: on the wrap cases the optimised volume, the disparity maps behind it and the whole Match differ from
    the reference (wrap0_320x288_d16: 417297 of 1474560 cost_so values, first at (0, 0, 0)).  Strict: passes the day the scanline
    reproduces the reference's NaN order, and must then move into STAGE_CASES."""
    left, right, opt = cases.make_case(name)
    o = oracle.run(left, right, opt)
    from tests import gpu_harness
    rep = gpu_harness.stage_report(left, right, opt, o)
    bad = {k: v for k, v in gpu_harness.failing(rep).items() if k.startswith(("cost_so", "match_final"))}
    assert not bad, "%s (oracle=%s): %s" % (name, oracle.kind, bad)
