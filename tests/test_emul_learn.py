"""CPU tier: adcensus_amd/csrc/learn_plan.h -- what a handle learns from one Match for the next -- driven by tests/emul/emul_learn.cpp
the way adc_wait, run_heavy, the median fallback and the voting finish drive it.  The constants are pinned, hand-written streams walk
every hold to its end Match by Match (what the GPU tier does with 64 and more Matches per test), and the random mode checks the
invariants of DESIGN.md section 5 against bookkeeping of its own."""
import re
import subprocess

import pytest

from tests import stream_model as M


@pytest.fixture(scope="module")
def exe():
    return M.build_emul("emul_learn")


def _stream(exe, geometry, matches):
    text = "G %s\n" % geometry + "".join("M %s\n" % m for m in matches)
    out = subprocess.run([exe, "stream"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(matches)
    return [{k: v if k == "hist" else int(v) for k, v in (t.split("=", 1) for t in line.split() if "=" in t)} for line in out]


G160 = "W=160 H=48 VPL=2 L1=34 so_fast=0"  # two scanline segments per row, compiler-allocated family: the tail can move
NOISE = "ah=1 av=1 nzh=100 nzv=100"


def test_constants(exe):
    c = M.consts()
    assert (c["plan_switch"], c["so_seam"], c["med_band"], c["med_column"]) == (64, 64, 64, 64)
    assert (c["max_redos"], c["irv_first"], c["irv_floor"], c["irv_history"], c["irv_max"]) == (2, 256, 4, 8, 1 << 16)
    assert (c["so_warm"], c["so_max_seg"], c["small_L"], c["assume_margin"], c["cf_tx"], c["cf_lds_max"]) == (64, 8, 8, 1, 128, 48 * 1024)
    assert M.holds() == {"agg_dual": 64, "so_seg_off": 64, "med_seg_off": 64, "med_spec_off": 64}
    assert (M.SO_WARM, M.SO_MAX_SEG, M.SMALL_L_KNOB, M.ASSUME_MARGIN) == (64, 8, 8, 1)


def test_first_match_full_ring_then_assumed(exe):
    r = _stream(exe, G160, [NOISE, NOISE, "ah=1 av=1 nzh=100 nzv=100 pending=0"])
    assert (r[0]["arms"], r[0]["arm_known"], r[0]["nzk"], r[0]["budget"]) == (3, 1, 1, 256)
    assert (r[1]["arms"], r[1]["can"], r[1]["fits"], r[1]["nseg"], r[1]["redos"]) == (2, 1, 1, 2, 0)
    state = lambda x: {k: v for k, v in x.items() if k in ("ah", "av", "sh", "sv", "nzh", "nzv", "last_plan", "agg_dual", "so_seg_off", "so_seg_probe")}
    assert state(r[2]) == state(r[1])  # a commit without a pending Match


def test_seam_hold_and_probe(exe):
    hold = M.holds()["so_seg_off"]
    r = _stream(exe, G160, [NOISE, NOISE + " seam=1"] + [NOISE] * (hold + 2))
    bad = r[1]
    assert (bad["nseg"], bad["redos"], bad["partial"], bad["so_seam_redos"], bad["arm_redos"]) == (2, 1, 1, 1, 0)
    assert (bad["so_seg_off"], bad["so_seg_probe"], bad["arm_known"]) == (hold - 1, 1, 1)
    inside = r[2:1 + hold]
    assert len(inside) == hold - 1 and all(x["nseg"] == 1 and x["can"] == 0 and x["so_seg_probe"] == 1 for x in inside)
    assert [x["so_seg_off"] for x in inside] == list(range(hold - 2, -1, -1))
    back, after = r[1 + hold], r[2 + hold]
    assert (back["nseg"], back["can"], back["so_seg_probe"]) == (2, 0, 0)  # the segments come back alone, hold their seams
    assert (after["nseg"], after["can"]) == (2, 1)                         # ... and the tail moves again
    assert after["so_seam_redos"] == 1 and after["redo_partial"] == 1


def test_ring_failure_sets_no_seam_hold(exe):
    """a too-shallow ring: one redo from the aggregation on, full ring, whole rows -- also where the stale volume failed a seam"""
    for extra in ("", " seam=1"):
        r = _stream(exe, G160, [NOISE, "ah=6 av=1 nzh=100 nzv=100" + extra, NOISE])
        x = r[1]
        assert (x["arms"], x["redos"], x["redo_h"], x["redo_v"], x["partial"]) == (2, 1, 1, 0, 1)
        assert (x["arm_redos"], x["so_seam_redos"], x["so_seg_off"], x["so_seg_probe"], x["arm_known"], x["ah"]) == (1, 0, 0, 0, 1, 6)
        assert (r[2]["nseg"], r[2]["arms"]) == (2, 2)
    v = _stream(exe, G160, [NOISE, "ah=1 av=7 nzh=100 nzv=100"])[1]
    assert (v["redo_h"], v["redo_v"], v["redos"]) == (0, 1, 1)


def test_flags_that_never_clear(exe):
    x = _stream(exe, G160, [NOISE, NOISE + " seam=2"])[1]
    assert (x["redos"], x["stuck"]) == (M.consts()["max_redos"], 1)


def test_plan_switch_hold(exe):
    hold = M.holds()["agg_dual"]
    long_arms = "ah=20 av=3 nzh=5000 nzv=5000"
    r = _stream(exe, G160, [NOISE, long_arms] + [NOISE] * (hold + 2))
    assert (r[1]["redos"], r[1]["agg_switches"], r[1]["agg_dual"], r[1]["last_plan"], r[1]["sh"], r[1]["sv"]) == (1, 1, hold, 2, 1, 1)
    assert (r[2]["dual"], r[2]["agg_switches"], r[2]["agg_dual"]) == (1, 2, hold)  # back to short arms: a switch again, no redo
    assert [x["dual"] for x in r[3:3 + hold]] == [1] * hold and r[2 + hold]["agg_dual"] == 0
    assert (r[3 + hold]["dual"], r[3 + hold]["redos"], r[3 + hold]["agg_switches"]) == (0, 0, 2)
    zero = _stream(exe, G160, ["ah=0 av=0 nzh=0 nzv=0"])[0]
    assert (zero["sh"], zero["sv"], zero["last_plan"]) == (1, 1, 1)  # armmax_small: floor 1


def test_median_ladder_and_side_by_side_holds(exe):
    hs, hg = M.holds()["med_spec_off"], M.holds()["med_seg_off"]
    r = _stream(exe, G160, [NOISE + " mcol=1 mband=1"] + [NOISE] * max(hs, hg))
    x = r[0]
    assert (x["med_spec"], x["med_seg"], x["med_rungs"], x["med_last"]) == (2, 3, 2, 2)  # bands on whole rows, then chained
    assert (x["med_seg_off"], x["med_spec_off"], x["med_spec_fails"], x["median_fallbacks"]) == (hg - 1, hs - 1, 1, 1)
    assert all(y["med_spec"] == 0 and y["med_seg"] == 1 for y in r[1:min(hs, hg)])
    assert (r[hs]["med_spec"], r[hg]["med_seg"]) == (2, 3)  # both back together, not one hold after the other
    col = _stream(exe, G160, [NOISE + " mcol=1", NOISE])
    assert (col[0]["med_rungs"], col[0]["med_last"], col[0]["med_seg_off"], col[0]["med_spec_off"]) == (1, 1, hg - 1, 0)
    assert (col[1]["med_spec"], col[1]["med_seg"]) == (2, 1)
    band = _stream(exe, G160 + " med_nseg=1", [NOISE + " mband=1"])[0]
    assert (band["med_rungs"], band["med_last"], band["med_seg_off"], band["med_spec_off"]) == (1, 2, 0, hs - 1)
    timeout = _stream(exe, G160, [NOISE + " mtime=1"])[0]
    assert (timeout["med_rungs"], timeout["med_last"], timeout["med_spec_fails"], timeout["med_spec_off"], timeout["median_fallbacks"]) == (1, 3, 0, 0, 1)
    f1, f2 = _stream(exe, G160, [NOISE + " forced=1"])[0], _stream(exe, G160, [NOISE + " forced=2"])[0]
    assert (f1["med_last"], f1["med_spec_fails"], f1["med_spec_off"], f1["med_seg_off"]) == (3, 0, 0, 0)
    assert (f2["med_rungs"], f2["med_last"], f2["med_spec_fails"], f2["med_spec_off"], f2["med_seg_off"]) == (1, 2, 1, hs - 1, 0)


def test_voting_budget(exe):
    uses = [300, 1, 2, 60, 5, 5, 5, 5, 5, 5, 5, 2, 2, 2, 2, 2, 2, 2, 2]
    r = _stream(exe, G160, [NOISE + " used=%d" % u for u in uses])
    budget = 256
    for i, x in enumerate(r):
        assert x["budget"] == budget and x["continued"] == int(uses[i] > budget)
        longest = max(uses[max(0, i - 7):i + 1])
        budget = 4 if longest <= 2 else min(1 << 16, longest + max(2 * longest // 5, 2) + 2)
        assert x["irv_budget"] == budget >= 4
    assert r[0]["irv_overflows"] == 1 and r[-1]["irv_overflows"] == 1 and r[-1]["irv_budget"] == 4
    assert _stream(exe, G160 + " irv_fixed=9", [NOISE + " used=100"])[0]["irv_budget"] == 9


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_invariants(exe, seed):
    o = subprocess.run([exe, "random", str(seed), "20000"], capture_output=True, text=True)
    assert o.returncode == 0, o.stdout[-3000:]
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", o.stdout.splitlines()[-1])}
    assert got["matches"] == 20000 and got["violations"] == 0
    for k in ("seam_failures", "shallow_rings", "both_median_seams", "forced_fallbacks", "chains_le2", "chains_ge300", "plan_switches", "holds_ended"):
        assert got[k] >= 20, (k, got)
