"""CPU tier: the streams of tests/streams.py and the model of the host rules (tests/stream_model.py), with the port oracle.

The GPU tier (tests/test_gpu_streams.py) compares every Match of these streams with the model; here the streams themselves are
checked: the fixed order has every transition, every image class lies on the side of the small-ring limit and of the fused tail's
depth it is meant to lie on under every option set it runs with, and the model's predictions over the committed streams reach the
coverage floors -- conditions on the streams, not measurements: a missed floor means other streams, never another floor."""
import collections
import subprocess

import pytest

from tests import stream_model as M
from tests import streams

FLOOR = 3


@pytest.fixture(scope="module")
def exe():
    return M.build_emul()


@pytest.fixture(scope="module")
def tables(port_oracle):
    cache = {}

    def get(geometry, option_set):
        if (geometry, option_set) not in cache:
            cache[(geometry, option_set)] = streams.oracle_table(port_oracle, geometry, option_set)
        return cache[(geometry, option_set)]
    return get


def test_fixed_order_has_every_transition():
    order = streams.FIXED_ORDER
    assert len(order) == 17 and set(order) == set(streams.CLASSES)
    pairs = [order[i:i + 2] for i in range(len(order) - 1)]
    assert len(set(pairs)) == 16 and set(pairs) == {a + b for a in streams.CLASSES for b in streams.CLASSES}


def test_random_orders_and_combos():
    for g in streams.GEOMETRIES:
        short, mixed = streams.random_orders(g)
        assert len(short) + len(mixed) == 24 and set(short) <= set("ndr") and "s" in mixed
        assert (short, mixed) == streams.random_orders(g)  # seeded
    per_set = collections.Counter(s for _, s in streams.COMBOS)
    assert set(per_set) == set(streams.OPTION_SETS) and min(per_set.values()) >= 2
    assert {g for g, s in streams.COMBOS if s == "default"} == set(streams.GEOMETRIES)
    assert len(set(streams.COMBOS)) == len(streams.COMBOS)


def test_holds_are_read_from_the_code():
    h = M.holds()
    assert set(h) == {"agg_dual", "so_seg_off", "med_seg_off", "med_spec_off"} and all(v >= 2 for v in h.values())


def test_emul_one_mode(exe):
    """`emul_agg_plan one`: a first Match runs the full ring; the Match behind a noise image runs flat + gather and moves its tail when
    the scanline stage can take it; the same handle in the two-plan mode launches neither."""
    base = "W=160 H=48 Dp=128 L1=34 ah=1 av=1 sh=1 sv=1 nzk=1 nzh=100 nzv=100 fits=1".split()
    run = lambda *a: dict(t.split("=", 1) for t in subprocess.check_output([exe, "one", *base, *a], text=True).split())
    first = run("valid=3", "can=1")
    assert (first["sparse"], first["flat"], first["tail_moved"], first["first_fused"], first["dual"]) == ("0", "0", "0", "1", "0")
    assert first["forms"].split(",")[0] == "rr2_cost:34" and len(first["forms"].split(",")) == 8
    later = run("valid=2", "can=1")
    assert (later["sparse"], later["gather"], later["flat"], later["tail_moved"]) == ("3", "3", "1", "1")
    assert later["forms"] == "cost_flat:2,gather+pair:2,gather+pair:2,gather+pair:2"
    assert run("valid=2", "can=0")["tail_moved"] == "0" and run("valid=2", "can=0")["sparse"] == "4"
    two = run("valid=2", "can=1", "dual=1")
    assert (two["dual"], two["sparse"], two["flat"], two["tail_moved"]) == ("1", "0", "0", "0")


def test_restated_handle_facts():
    """adc_so_segments / adc_so_can_fuse_agg / adc_cost_agg_flat_fits as restated"""
    assert M.so_segments(160, 48, 2, 0) == 2 and M.so_segments(128, 48, 2, 0) == 1 and M.so_segments(203, 40, 2, 0) == 4
    assert M.so_segments(160, 48, 2, 1) == 1 and M.so_segments(321, 37, 4, 0) == 1
    assert not M.so_can_fuse(160, 48, 2, 0, None) and M.so_can_fuse(160, 48, 2, 0, 0) and not M.so_can_fuse(160, 48, 2, 1, 0)
    assert not M.so_can_fuse(160, 48, 1, 0, 0) and not M.so_can_fuse(321, 37, 4, 0, 0) and not M.so_can_fuse(160, 48, 2, 0, 0, so_seg_probe=1)
    assert M.cost_flat_fits(128, 8) and M.cost_flat_fits(256, 8) and not M.cost_flat_fits(64, 2)
    # ... and against the header (learn_plan.h through `emul_learn grid`): every geometry of the streams and the full sizes, widths
    # 64 .. 2048 in coarse steps plus the widths around which each segment count starts to fit
    limits = [next(w for w in range(64, 2049) if M.so_seg_ok(w, n, M.SO_WARM)) for n in range(2, M.SO_MAX_SEG + 1)]
    widths = sorted(set(range(64, 2049, 62)) | {w + d for w in limits for d in (-1, 0, 1)} | {g[0] for g in streams.GEOMETRIES.values()})
    heights = sorted({g[1] for g in streams.GEOMETRIES.values()} | {375, 1080})
    grid = [(w, h, vpl, off, probe, seg, fast, 64 * vpl * (1 + w % 2), w % 37)
            for w in widths for h in heights for vpl in (1, 2, 4) for off in (0, 1) for seg in (-1, 0, 1, 2, 5, 8)
            for fast, probe in ((-1, 0), (0, 0), (0, 1), (1, 0))]
    assert min(limits) > 64 and max(limits) < 2048 and len(grid) > 20000
    out = subprocess.run([M.build_emul("emul_learn"), "grid"], input="".join("%d %d %d %d %d %d %d %d %d\n" % g for g in grid),
                         capture_output=True, text=True, check=True).stdout.split("\n")
    seen = collections.Counter()
    for (w, h, vpl, off, probe, seg, fast, dp, cap), line in zip(grid, out):
        want = (M.so_segments(w, h, vpl, off, seg_env=seg), int(M.so_can_fuse(w, h, vpl, off, None if fast < 0 else fast, probe, seg_env=seg)),
                int(M.cost_flat_fits(dp, cap)))
        assert tuple(int(t) for t in line.split()) == want, (w, h, vpl, off, probe, seg, fast, dp, cap, line, want)
        seen[want] += 1
    assert {k[0] for k in seen} == set(range(1, M.SO_MAX_SEG + 1)) and {k[1] for k in seen} == {0, 1} and {k[2] for k in seen} == {0, 1}


@pytest.mark.parametrize("geometry,option_set", streams.COMBOS)
def test_classes_land_on_their_side(tables, geometry, option_set):
    """n: the assumed depth (arm + margin) stays within 4, the fused tail's limit, and the density below the sparse threshold.  d: within
    the small ring, density above the threshold.  r: an arm of 5 or more along every planted direction (too deep for the
    tail), none beyond the small ring unless arm_t lengthens the runs; a one-direction variant stays within depth 4 along the other.
    s: beyond the small ring -- with cross_L1 = 8 there is none, the arms then reach the limit itself."""
    tab = tables(geometry, option_set)
    L1 = streams.OPTION_SETS[option_set].get("cross_L1", 34)
    small_L = min(M.SMALL_L_KNOB, L1)
    P = streams.GEOMETRIES[geometry][0] * streams.GEOMETRIES[geometry][1]
    thr = M.default_thresholds_ppm()["sparse"] * 1e-6 * P
    for key, f in tab.items():
        ah, av = f["armmax"]
        if key[0] == "n":
            assert max(ah, av) + M.ASSUME_MARGIN <= 4 and max(f["nz"]) <= thr, (key, f["armmax"], f["nz"])
        elif key[0] == "d":
            assert max(ah, av) <= small_L and max(f["nz"]) > thr, (key, f["armmax"], f["nz"], thr)
        elif key[0] == "r":
            along = {"r0": (ah, av), "r1": (av,), "r2": (ah,)}[key]
            across = {"r0": (), "r1": (ah,), "r2": (av,)}[key]
            assert min(along) >= 5 and all(a + M.ASSUME_MARGIN <= 4 for a in across), (key, f["armmax"])
            if option_set != "arm_t":
                assert max(ah, av) <= small_L, (key, f["armmax"])
        else:
            assert max(ah, av) > small_L if small_L < L1 else max(ah, av) == L1, (key, f["armmax"])


@pytest.mark.parametrize("so_fast", [None, 0])
def test_coverage_floors(exe, tables, so_fast):
    """Per scanline family (default, ADC_SO_FAST=0), summed over all committed streams: at least three Matches of every kind."""
    total = collections.Counter()
    for geometry, option_set in streams.COMBOS:
        tab = tables(geometry, option_set)
        for name, order in streams.stream_orders(geometry).items():
            keys = streams.expand(geometry, order)
            preds = M.predict_stream(exe, streams.GEOMETRIES[geometry], streams.OPTION_SETS[option_set], so_fast, keys, tab)
            for k in M.kinds_of(preds):
                total.update(k)
            if option_set == "L8" or geometry == "g160d64":  # no small ring / one disparity per lane: never sparse, gather, flat, fused
                assert all(p["d16"] == p["d20"] == p["d22"] == p["fuse"] == 0 for p in preds)
            if option_set == "L8":
                assert all(p["d10"] == 0 and p["d2"] == 0 for p in preds)
    print("so_fast=%s: %s" % (so_fast, dict(total)))
    for kind in M.KINDS:
        if kind == "fused" and so_fast is None:
            assert total[kind] == 0  # (rows of these sizes run the pinned family, which cannot take the pass over)
            continue
        assert total[kind] >= FLOOR, (kind, dict(total))


def _model_rows(exe, geometry, option_set, so_fast, keys, tab):
    """HandleModel over one stream: per Match the scenario it enqueues, which gate redoes it, and the state behind it.  The state does
    not depend on the plan, so the scenarios are collected first and planned in one call (by the caller)."""
    mk = lambda: M.HandleModel(exe, *streams.GEOMETRIES[geometry], cross_L1=streams.OPTION_SETS[option_set].get("cross_L1", 34), so_fast=so_fast)
    m, scen = mk(), []
    none = {"dual": 1, "first_fused": 0, "sparse": 0, "gather": 0, "flat": 0, "tail_moved": 0, "forms": []}
    for k in keys:
        scen.append(m.scenario())
        m.apply(none, tab[k])

    def rows(plans):
        m, out = mk(), []
        for k, sc, plan in zip(keys, scen, plans):
            assert m.scenario() == sc
            p = m.apply(plan, tab[k])
            out.append({"arms": sc["valid"], "can": sc["can"], "fits": sc["fits"], "dual": plan["dual"], "redos": p["redo"], "redo_h": int(p["redo_h"]),
                        "redo_v": int(p["redo_v"]), "partial": p["d11"], "so_seg_off": m.so_seg_off, "agg_dual": m.agg_dual, "sh": m.armmax_small[0],
                        "sv": m.armmax_small[1], "ah": m.armmax_host[0], "av": m.armmax_host[1], "nzh": m.rec_nz[0], "nzv": m.rec_nz[1]})
        return out
    return m, scen, rows


@pytest.mark.parametrize("so_fast", [None, 0])
def test_model_agrees_with_the_header(exe, tables, so_fast):
    """Every committed stream's oracle facts through learn_plan.h (`emul_learn stream`: redo decision, commit, plan inputs, with the ring
    word taken from the gates of the launches agg_plan.h plans) and through HandleModel: the two agree on every Match -- redone or not
    and by which gate, the assumption, so_seg_off, agg_dual, armmax_small, the can / fits inputs of the plan."""
    jobs, text, scenarios = [], [], []
    for geometry, option_set in streams.COMBOS:
        tab = tables(geometry, option_set)
        w, h, dmin, dmax = streams.GEOMETRIES[geometry]
        for name, order in streams.stream_orders(geometry).items():
            keys = streams.expand(geometry, order)
            m, scen, rows = _model_rows(exe, geometry, option_set, so_fast, keys, tab)
            jobs.append(((geometry, option_set, name), keys, len(scenarios), rows))
            scenarios += scen
            text.append("G W=%d H=%d VPL=%d L1=%d so_fast=%d density_ppm=%d" % (w, h, m.vpl, m.L1, -1 if so_fast is None else so_fast, m.thr["sparse"]))
            text += ["M ah=%d av=%d nzh=%d nzv=%d" % (*tab[k]["armmax"], *tab[k]["nz"]) for k in keys]
    plans = M.plan_many(exe, scenarios)
    out = subprocess.run([M.build_emul("emul_learn"), "stream"], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(scenarios)
    redone = collections.Counter()
    for where, keys, at, rows in jobs:
        for i, want in enumerate(rows(plans[at:at + len(keys)])):
            got = {k: int(v) for k, v in (t.split("=", 1) for t in out[at + i].split() if "=" in t) if k in want}
            assert got == want, (where, i, keys[i], got, want)
            redone[(want["redo_h"], want["redo_v"])] += 1
    assert min(redone[(0, 0)], redone[(1, 0)], redone[(0, 1)], redone[(1, 1)]) >= FLOOR, redone
