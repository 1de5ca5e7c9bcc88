"""GPU tier: the option space (tests/cases.py: OPT_SETS) through the scanline kernel families that the automatic choice does not
take at the small sizes of its cases.  At these sizes a Match runs k_scanline_pin; ADC_SO_FAST=0 forces the compiler-allocated
family (k_scanline / k_scanline_seg, and with it k_scanline_seg_agg: the last aggregation pass inside the first scanline pass, which
sees lambda, the penalties and so_tso at once), ADC_SO_FAST=1 the pinned family everywhere, ADC_SO_DPP=0 the ds_bpermute forms.
The switches are read once per process: one interpreter per family (tests/option_family_probe.py), all cases in it, three
Matches per handle against the oracle's disp_final."""
import json
import os
import subprocess
import sys

import pytest

from tests import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCANLINE_CASES = cases.OPT_CASES["cost"] + cases.OPT_CASES["penalty"] + cases.OPT_CASES["tso"]


def _probe(env, names):
    o = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "option_family_probe.py")] + names, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert o.returncode == 0, o.stdout[-2000:] + o.stderr[-2000:]
    res = json.loads([l for l in o.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert sorted(res) == sorted(names)
    for n in names:  # (which form each case ran: profiles/README.md keeps the table)
        print(env, n, res[n])
    return res


@pytest.mark.parametrize("fast", ["0", "1"])
def test_both_scanline_families_under_option_cases(hip, fast):
    """The cost, penalty and so_tso cases under ADC_SO_FAST=0 and ADC_SO_FAST=1.  Under ADC_SO_FAST=0 the last aggregation pass
    must have moved into the scanline pass (counter 13) on the pair it can move on: n2w -- two disparities per lane, rows cut into
    two segments, horizontal arms <= 3.  (s2w, the structured pair with D = 128, has arms of 20: its Matches keep that pass a launch
    of its own and are pinned through the plain segment kernels.)  A handle whose seams failed redoes with whole rows and keeps them
    (counter 4), so it does not fuse: that may happen under the cases of cases.OPT_SEAMS_MAY_FAIL (big or negative penalties, and
    lambda = (1, 1) on the noise pair, whose saturated cost leaves the paths nothing to forget their start by: its seams do fail,
    as tests/test_emul.py::test_scanline_kernel_segments shows on the CPU) and under no other."""
    res = _probe({"ADC_SO_FAST": fast}, SCANLINE_CASES)
    bad = {n: r for n, r in res.items() if any(r["bad"])}
    assert not bad, bad
    for n, r in res.items():
        if n not in cases.OPT_SEAMS_MAY_FAIL:
            assert r["seam_redos"] == 0, (n, r)
        if fast == "0" and n.endswith("_n2w"):
            assert r["segments"] >= 2 or r["seam_redos"] > 0, (n, r)
            assert r["fused"] > 0 or (n in cases.OPT_SEAMS_MAY_FAIL and r["seam_redos"] > 0), (n, r)
        if fast == "1":
            assert r["fused"] == 0, (n, r)
    if fast == "0":
        assert sum(1 for n, r in res.items() if n.endswith("_n2w") and r["fused"] > 0) >= 10


def test_non_dpp_scanline_family_under_option_cases(hip):
    """ADC_SO_DPP=0: the cross-lane steps of the scanline recurrence through ds_bpermute instead of DPP (kept as a cross-check of the
    DPP forms): the penalty and so_tso cases, whole Match."""
    res = _probe({"ADC_SO_DPP": "0"}, cases.OPT_CASES["penalty"] + cases.OPT_CASES["tso"])
    bad = {n: r for n, r in res.items() if any(r["bad"])}
    assert not bad, bad
    assert all(r["fused"] == 0 for r in res.values())  # (the fused form exists for the DPP family only: adc_so_can_fuse_agg)
