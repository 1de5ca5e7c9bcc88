"""GPU tier (T1/T2): every HIP stage against the oracle, stage-isolated, plus the whole Match.
Bit-exact for every buffer (integer maps, f32 volumes, f32 disparity maps)."""
import pytest

from tests import cases, gpu_harness

pytestmark = pytest.mark.gpu

STAGE_CASES = ["s2_96x64_d32", "q_257x131_d64", "q_20x40_d32", "q_9x20_d8", "q_30x7_d8", "q_1x40_d8", "q_40x1_d8",
               "q_3x3_d2", "noise_128x72_d64", "noise_160x90_d128", "noise_150x40_d256", "s2_150x100_neg", "s2_320x180_d128", "s2_200x120_d200", "cone_crop_d40", "cone_crop_L40",
               "cone", "cone_neg", "cone_d16", "cone_nolr", "cone_nofill", "cone_dda", "cone_params",
               # min_disparity > 0, 128 < D < 192 (all-padding chunk), D > 256 up to the maximum of 2047, discontinuity adjustment with dmin != 0
               "cone_pos", "q_40x30_pos_wltd", "noise_160x90_d128_pos", "s2_150x100_pos", "s2_200x120_d160",
               "noise_96x50_d160_neg", "s2_360x60_d300", "noise_80x40_d520", "s2_72x48_d1024", "noise_64x24_d1100", "s2_80x20_d2047",
               "cone_crop_dda_neg", "cone_crop_dda_pos",
               # long arm limits up to 255 (and the clamp above it), odd arm options and shapes.  (The cases whose 16-bit support
               # counts wrap, wrap0_320x288_d16 / wrap_320x320_d8, are pinned up to the aggregation: tests/test_gpu_long_arms.py)
               "flat_640x96_L48", "flat_640x96_L49", "flat_640x96_L64", "flat_640x96_L128", "flat_640x96_L255", "flat_640x96_L300",
               "flat_640x96_L1000", "flat_560x320_L255", "flat_640x96_L64_L2gt", "flat_640x96_L128_L2zero", "flat_640x96_L128_t2t1",
               "flat_200x64_L255", "flat_600x1_L255", "flat_1x300_L255"]
# the option space (tests/cases.py: OPT_SETS): extreme and in-between values of the twelve numeric option fields on small pairs
STAGE_CASES += cases.OPT_DEFAULT_CASES + cases.OPT_ALL_CASES


@pytest.mark.parametrize("name", STAGE_CASES)
def test_stage_parity(hip, oracle, name):
    left, right, opt = cases.make_case(name)
    o = oracle.run(left, right, opt)
    rep = gpu_harness.stage_report(left, right, opt, o, seams_may_fail=name in cases.OPT_SEAMS_MAY_FAIL)
    if name in cases.OPT_CASES["penalty"] or name in cases.OPT_SEAMS_MAY_FAIL:  # (which form ran: profiles/README.md keeps the table)
        print("%s: scanline segments per row %d, failed seams %d" % (name, rep["cost_so"]["segments"], rep["cost_so"]["seam_fails"]))
    bad = gpu_harness.failing(rep)
    assert not bad, "%s (oracle=%s): %s" % (name, oracle.kind, bad)


@pytest.mark.parametrize("name", ["cloth3", "piano", "wood2"])
def test_middlebury_pairs(hip, oracle, name):
    """The other pairs of the reference's Data/ directory (committed fixtures tests/golden/<name>_{left,right}.npz); the
    oracle's dumps are additionally checked against the committed SHA-256 table of the reference build."""
    import hashlib
    import json
    import os
    import numpy as np
    left, right, opt = cases.make_case(name)
    o = oracle.run(left, right, opt)
    with open(os.path.join(cases.GOLDEN_DIR, "golden.json")) as f:
        gold = json.load(f)["cases"][name]
    stale = [k for k, v in o.items() if hashlib.sha256(np.ascontiguousarray(cases.canonical(k, v, opt)).tobytes()).hexdigest() != gold[k]]
    assert not stale, "oracle (%s) differs from the committed reference golden: %s" % (oracle.kind, stale)
    rep = gpu_harness.stage_report(left, right, opt, o)
    assert not gpu_harness.failing(rep), gpu_harness.failing(rep)
