"""CPU tier: the oracles' stage entry (oracle.refine_from, oracle_abi.h: adc_oracle_refine_from) and the constructed refinement
inputs of tests/refine_patterns.py.

  * port == reference through refine_from on every pattern, bit for bit (where the reference library exists);
  * refine_from entered at each stage with oracle.run's dump of the stage before reproduces the dumps of the later stages (the
    rebuild of the two pixel lists from the label map), and equals cases.region_voting_reference on the slack-window input;
  * tests/emul's restatements of the interpolation walk equal refine_from(INTERP) on every interpolation pattern: the emulation
    is tied to the reference, not to another emulation;
  * coverage: the patterns do reach the branches they were built for -- counted on the reference's outputs (`oracle`: the
    reference where it exists, else the port that the tests above pin to it);
  * every pattern family once through refine_from in the ASAN + UBSAN builds of both oracles (oracle/sanitize_main.c, a stand-alone
    program): the constructed inputs are defined behaviour of the reference."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from oracle import pyoracle
from oracle.pyoracle import DDA, INTERP, LR, MEDIAN, VOTING
from tests import cases
from tests import refine_patterns as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def run_stage(orc, p):
    """(map, label) of the pattern's own stage"""
    if p.family == "lr":
        return orc.refine_from(LR, LR, p.disp, p.opt, disp_right=p.disp_right)
    if p.family == "dda":
        return orc.refine_from(DDA, DDA, p.disp, p.opt, cost=p.cost, label=np.zeros(p.disp.shape, np.uint8))
    return orc.refine_from(INTERP, INTERP, p.disp, p.opt, left=p.img, label=p.label)


def all_small_patterns():
    out = rp.interpolation_small() + rp.many() + [rp.edge_2p24(4094), rp.edge_2p24(4095)] + rp.offset()
    for r in range(len(rp.RANGES)):
        out += rp.lr_set(r) + rp.dda_set(r)
    return out


@pytest.fixture(scope="module")
def oracle(ref_oracle, port_oracle):
    """the checker of this module: pyoracle.stage_entry_oracle (a reference build that has refine_from, else the port)"""
    return pyoracle.stage_entry_oracle(ref_oracle, port_oracle)


@pytest.fixture(scope="module")
def patterns():
    return all_small_patterns()


def test_port_equals_reference_on_every_pattern(port_oracle, ref_oracle, patterns):
    if ref_oracle is None or not ref_oracle.has_refine_from:
        pytest.skip("no reference build with the stage entry: oracle/_ref not built, or built before it, and the reference's sources absent")
    bad = []
    for p in patterns:
        a, b = run_stage(port_oracle, p), run_stage(ref_oracle, p)
        if not (same(a[0], b[0]) and same(a[1], b[1])):
            bad.append(repr(p))
    assert not bad, bad


STAGE_DUMPS = ["disp_left_wta", "disp_after_lr", "disp_after_irv", "disp_after_interp", "disp_after_dda", "disp_final"]


@pytest.mark.parametrize("name", ["s2_96x64_d32", "cone_crop_dda_neg"])
def test_entry_at_each_stage_reproduces_the_dumps(oracle, name):
    """Entered at stage k with the dump of stage k - 1 (and the label map for k > LR), refine_from gives the dumps of the stages k ..
    MEDIAN: the lists rebuilt from the labels are the lists OutlierDetection left behind."""
    left, right, opt = cases.make_case(name)
    assert opt.do_lr_check and opt.do_filling
    o = oracle.run(left, right, opt)
    stages = [LR, VOTING, INTERP, DDA, MEDIAN]
    for first in stages:
        for last in stages[first:]:
            if not opt.do_discontinuity_adjustment and first <= DDA <= last:
                continue  # (the pipeline did not run it: nothing to compare with)
            got, lab = oracle.refine_from(first, last, o[STAGE_DUMPS[first]], opt, left=left, cost=o["cost_so"], arms=o["arms"],
                                          disp_right=o["disp_right_wta"], label=None if first == LR else o["outlier_label"])
            assert same(got, o[STAGE_DUMPS[last + 1]]), (first, last)
            assert same(lab, o["outlier_label"]), (first, last)
    if not opt.do_discontinuity_adjustment:  # stage ranges that skip the adjustment, as the pipeline did
        got, _ = oracle.refine_from(MEDIAN, MEDIAN, o["disp_after_interp"], opt, label=o["outlier_label"])
        assert same(got, o["disp_final"])


def test_missing_inputs_are_refused(oracle):
    d = np.zeros((3, 4), np.float32)
    lab = np.zeros((3, 4), np.uint8)
    opt = pyoracle.Option(max_disparity=8)
    for first, last, kw in ((LR, LR, {}), (VOTING, VOTING, dict(label=lab)), (INTERP, INTERP, dict(label=lab)), (DDA, DDA, dict(label=lab)),
                            (LR, MEDIAN, dict(disp_right=d, arms=np.zeros((3, 4, 4), np.uint8), left=np.zeros((3, 4, 3), np.uint8)))):
        with pytest.raises(RuntimeError, match="rc=2"):
            oracle.refine_from(first, last, d, opt, **kw)
    with pytest.raises(RuntimeError, match="rc=3"):
        oracle.refine_from(INTERP, LR, d, opt, label=lab)
    got, _ = oracle.refine_from(MEDIAN, MEDIAN, d, opt, label=lab)  # needs nothing but the map
    assert same(got, d)


def test_region_voting_reference_equals_refine_from(oracle):
    for w, h in ((256, 1), (256, 3)):
        disp, label, arms, _, opt = cases.slack_window_voting_input(w, h)
        got, _ = oracle.refine_from(VOTING, VOTING, disp, opt, arms=arms, label=label)
        assert same(got, cases.region_voting_reference(disp, label, arms, opt))
        assert (got[:, 0] == 9.0).all()  # (the vote the input was built for)


def test_emulations_equal_the_reference_walk(emul, oracle):
    """emul_interpolate (the plain walk) and emul_interpolate_code (the walk of k_interpolate_tab on the padded code map, with the
    kernel's trip lengths) against refine_from(INTERP) on every interpolation pattern up to 203 x 61."""
    emul.emul_interpolate_code.restype = C.c_long
    pats = rp.interpolation_small() + rp.offset()
    for p in pats:
        want, _ = run_stage(oracle, p)
        h, w = p.disp.shape
        ms = rp.search_range(p.opt)
        a, b = p.disp.copy(), np.empty((h, w), np.float32)
        emul.emul_interpolate(P(a), P(b), P(p.label), P(p.img), w, h, 1, ms)
        emul.emul_interpolate(P(b), P(a), P(p.label), P(p.img), w, h, 2, ms)
        assert same(a, want), p
        if p.family != "offset":  # (no table walk there: itp_plan.h)
            a, b = p.disp.copy(), np.empty((h, w), np.float32)
            assert emul.emul_interpolate_code(P(a), P(b), P(p.label), P(p.img), w, h, 1, ms, 2, 4) >= 0, p
            assert emul.emul_interpolate_code(P(b), P(a), P(p.label), P(p.img), w, h, 2, ms, 2, 4) >= 0, p
            assert same(a, want), p


# ------------------------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("ms", rp.REACH_MS)
def test_reach_targets_are_filled_from_the_planted_pixel(oracle, ms):
    """... by the reference's own walk: the planted value where step m lies inside the search range (or an earlier step rounds to
    the same pixel), 0.0f at m = ms; and a range that ends one step earlier does not find a pixel that only step m reaches."""
    pats = rp.reach(ms)
    assert {p.name.split("_s")[1] for p in pats} == {str(s) for s in range(16)}
    earlier = {}
    for p in pats:
        got, _ = run_stage(oracle, p)
        ty, tx = p.info["target"]
        want = p.disp[p.info["planted"]] if p.info["found"] else np.float32(0.0)
        assert got[ty, tx] == want and not (want == 0 and np.signbit(got[ty, tx])), (p, got[ty, tx], want)
        m = int(p.name.split("_m")[1].split("_")[0])
        if m < ms:  # the same map under the range [0, m): steps 1 .. m - 1 only
            short, _ = oracle.refine_from(INTERP, INTERP, p.disp, pyoracle.Option(max_disparity=m), left=p.img, label=p.label)
            earlier[p.name] = short[ty, tx] != 0.0
    # a planted pixel is met before step m only where rounding puts two steps on one pixel: never at m = 1, and for fewer than a
    # third of the maps
    assert not any(v for k, v in earlier.items() if "_m1_" in k)
    assert sum(earlier.values()) * 3 < len(earlier), sum(earlier.values())
    assert any(not p.info["found"] for p in pats) and all(p.info["found"] for p in pats if "_m%d_" % ms not in p.name)


def test_tie_fills(oracle):
    pats = {p.name: p for p in rp.tie()}
    for name, p in pats.items():
        got, _ = run_stage(oracle, p)
        v, col = p.info["values"], p.info["colours"]
        if name.endswith("list2"):
            want = min(v)  # occlusion: the smallest value
        else:
            dist = [3 * abs(c - p.info["own_colour"]) for c in col]
            want = v[dist.index(min(dist))]  # mismatch: the first ray in order among the nearest colours
        assert got[p.info["target"]] == want, (name, got[p.info["target"]], want)
    assert pats["uniform_list1"].info["values"][0] != min(pats["uniform_list1"].info["values"])
    col = pats["levels_list1"].info["colours"]
    assert col.count(60) >= 3 and col[0] != 60  # several rays tie at distance 0, ray 0 is not among them


def _withheld(orc, p):
    """the interpolation with the mismatch labels cleared: the first pass fills nothing"""
    lab = np.where(p.label == 1, 0, p.label).astype(np.uint8)
    return orc.refine_from(INTERP, INTERP, p.disp, p.opt, left=p.img, label=lab)[0]


def dependent_fills(orc, p):
    """occlusion targets whose fill changes when the first pass's fills are withheld"""
    got, held = run_stage(orc, p)[0], _withheld(orc, p)
    occ = (p.label == 2) & np.isinf(p.disp)
    return int((occ & (got.view(np.uint32) != held.view(np.uint32))).sum())


def test_two_pass_fills(oracle):
    (p,) = rp.two_pass()
    got, held = run_stage(oracle, p)[0], _withheld(oracle, p)
    i = p.info
    assert got[i["a"]] == 5.0 and got[i["b"]] == 0.0 and not np.signbit(got[i["b"]])
    assert got[i["o1"]] == 5.0 and held[i["o1"]] == 0.0   # O1's only hit is the first pass's fill of A
    assert got[i["o2"]] == 0.0 and held[i["o2"]] == 7.0   # O2 takes B's no-hit 0.0f for a disparity, as the reference does
    assert dependent_fills(oracle, p) == 2


@pytest.mark.parametrize("shape_index", range(len(rp.RANDOM_SHAPES)))
def test_random_maps_hold_second_pass_dependencies(oracle, shape_index):
    """Every random map with a density in (0, 1) holds at least 10 occlusion fills that depend on a first-pass fill -- except
    where no fill can depend on anything: the 1 x 1 image and the search range 1 (no step is ever taken), which stay in as the
    degenerate cases they are."""
    for p in rp.random_maps(shape_index):
        n = dependent_fills(oracle, p)
        if 0.0 < p.info["density"] < 1.0 and rp.random_can_depend(p):
            assert n >= 10, (p, n)
        if not rp.random_can_depend(p):
            assert n == 0, (p, n)


@pytest.mark.parametrize("rng_index", range(len(rp.RANGES)))
def test_lr_sets_reach_every_branch(oracle, rng_index):
    total = {}
    for p in rp.lr_set(rng_index):
        got, lab = run_stage(oracle, p)
        n, cur = rp.lr_classes(p, lab)
        assert same(cur, got), p
        for k, v in n.items():
            total[k] = total.get(k, 0) + int(v)
    print("LR set %d: %s" % (rng_index, total))
    for k in ("consistent", "invalid_in", "col_right_out", "col_rl_out", "mismatch_le", "occlusion", "late_occlusion"):
        assert total[k] >= 20, (k, total)
    assert total["col_rl_zero"] >= 3, total


@pytest.mark.parametrize("rng_index", range(len(rp.RANGES)))
def test_dda_sets_change_pixels(oracle, rng_index):
    changed = near_inf = 0
    for p in rp.dda_set(rng_index):
        got, _ = run_stage(oracle, p)
        diff = got.view(np.uint32) != p.disp.view(np.uint32)
        assert not (diff & np.isinf(p.disp)).any() and not np.isinf(got[diff]).any()  # an invalid pixel is neither changed nor copied
        changed += int(diff.sum())
        near_inf += int((diff & rp.inf_in_window(p.disp)).sum())
    print("adjustment set %d: %d pixels changed, %d of them next to +inf" % (rng_index, changed, near_inf))
    assert changed >= 20 and near_inf >= 5, (changed, near_inf)


def test_many_targets_exceed_the_walks_slots(oracle):
    for p in rp.many():
        assert int(((p.label > 0) & np.isinf(p.disp)).sum()) > 32768


# ----------------------------------------------------------------------------------------------------- sanitizer builds
def write_pattern_file(path, p, first, last):
    """oracle/sanitize_main.c, mode `refine FILE`: int32 {w, h, first, last, has_left, has_cost, has_arms, has_right, has_label}, the
    option struct, then the arrays that are there: left u8, cost f32, arms u8, disp f32, right f32, label u8."""
    h, w = p.disp.shape
    parts = [p.img, p.cost, None, p.disp, p.disp_right, p.label if p.label is not None else (np.zeros((h, w), np.uint8) if first > LR else None)]
    with open(path, "wb") as f:
        f.write(struct.pack("<9i", w, h, first, last, *[int(parts[i] is not None) for i in (0, 1, 2, 4, 5)]))
        f.write(bytes(p.opt))
        for a in parts:
            if a is not None:
                f.write(np.ascontiguousarray(a).tobytes())


def test_pattern_families_under_sanitizers(tmp_path, oracle):
    from tests.test_sanitize import _make, _run
    _make(os.path.join(ROOT, "oracle"))
    exes = [os.path.join(ROOT, "oracle", "_port", "sanitize_port")]
    ref = os.path.join(ROOT, "oracle", "_ref", "sanitize_ref")
    # (built by `make asan` wherever the reference's sources are: tests/test_sanitize.py insists on it there; a program kept from
    # before the `refine` mode, where they are not, cannot serve)
    if os.path.exists(ref) and pyoracle.exports(ref, b"refine_from ok"):
        exes.append(ref)
    rnd = rp.random_maps(0)[2]
    picks = [rp.reach(7)[-1], rp.reach(3)[5], rp.tie()[1], rp.two_pass()[0], rnd, rp.random_maps(7)[1], rp.many()[1], rp.edge_2p24(4095),
             rp.offset()[0], rp.lr_set(1)[1], rp.lr_set(2)[12], rp.dda_set(1)[2], rp.dda_set(2)[1]]
    assert {p.family for p in picks} == {"reach", "tie", "two_pass", "random", "many", "edge_2p24", "offset", "lr", "dda"}
    for k, p in enumerate(picks):
        first = {"lr": LR, "dda": DDA}.get(p.family, INTERP)
        path = str(tmp_path / ("p%d.bin" % k))
        write_pattern_file(path, p, first, first)
        want, _ = run_stage(oracle, p)
        want_sum = int(want.view(np.uint32).astype(np.uint64).sum())
        for exe in exes:
            out = _run([exe, "refine", path]).stdout
            assert "refine_from ok, sum %d" % want_sum in out, (p, exe, out)
