"""GPU tier: the state a handle learns from its earlier Matches -- assumed arm depths, record densities, plan history, the four
"hold for 64 Matches" counters -- against the oracle (every map, bit for bit, and the record densities) and against a model of the
host rules (tests/stream_model.py: which Match is redone, runs two plans, runs sparse / gather / flat launches, may move its tail).

Streams (tests/streams.py) run in tests/stream_probe.py, an interpreter of their own per scanline family.  The way out of each hold
is walked Match by Match; the length of every hold is read from the code that sets it (stream_model.holds())."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cases
from tests import stream_model as M
from tests import streams

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "stream_probe.py")
FAMILIES = {"default": {}, "so_fast0": {"ADC_SO_FAST": "0"}}


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _probe(args, env, timeout=240):
    o = subprocess.run([sys.executable, PROBE, *args], env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    if o.returncode == 3 or o.returncode < 0:  # a Match returned an error, or the probe died: nothing more runs on this GPU
        pytest.exit("stream probe %s ended with status %d:\n%s" % (args, o.returncode, o.stdout[-2000:] + o.stderr[-2000:]), returncode=3)
    assert o.returncode == 0, o.stdout[-2000:] + o.stderr[-2000:]
    return json.loads([l for l in o.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.fixture(scope="module")
def tables(oracle, tmp_path_factory):
    """(geometry, option set) -> ({image key: facts + want}, path of the maps for the probe): one oracle run per image and module"""
    cache = {}
    root = tmp_path_factory.mktemp("stream_tables")

    def get(geometry, option_set):
        if (geometry, option_set) not in cache:
            tab = streams.oracle_table(oracle, geometry, option_set)
            path = str(root / ("%s_%s.npz" % (geometry, option_set)))
            np.savez(path, **{"want_" + k: v["want"] for k, v in tab.items()})
            cache[(geometry, option_set)] = (tab, path)
        return cache[(geometry, option_set)]
    return get


# ------------------------------------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("geometry,option_set", streams.COMBOS)
def test_streams_follow_the_model(hip, tables, geometry, option_set, family):
    """Every Match of the fixed order and of the two random blocks: the map equals the oracle's; counters 18 / 19 equal the record
    densities the oracle's arms and support counts give for the image just matched (a redone Match included); the deltas of counters
    2, 10, 11, 16, 20, 22 equal the model's; counter 13 moves exactly where the model lets the tail move; no seam fails (counter 4)."""
    tab, path = tables(geometry, option_set)
    res = _probe([geometry, option_set, path], FAMILIES[family])
    thr = {"sparse": res["thresholds"]["17"], "gather": res["thresholds"]["21"], "flat": res["thresholds"]["23"]}
    exe = M.build_emul()
    so_fast = 0 if family == "so_fast0" else None
    errors = []
    for name, order in streams.stream_orders(geometry).items():
        keys = streams.expand(geometry, order)
        rows = res["streams"][name]
        assert [r["key"] for r in rows] == keys
        preds = M.predict_stream(exe, streams.GEOMETRIES[geometry], streams.OPTION_SETS[option_set], so_fast, keys, tab, thresholds_ppm=thr)
        prev = {str(c): 0 for c in (2, 4, 10, 11, 13, 16, 20, 22)}
        for i, (row, p) in enumerate(zip(rows, preds)):
            c = row["c"]
            delta = {k: c[k] - prev[k] for k in prev}
            prev = {k: c[k] for k in prev}
            print("%s %2d %s %-12s bad %d nz %d/%d deltas %s model %s" % (name, i, row["key"], row["entry"], row["bad"], c["18"], c["19"], delta,
                                                                          {k: p[k] for k in ("d2", "d10", "d11", "d16", "d20", "d22", "fuse")}))
            where = "%s Match %d (%s, %s)" % (name, i, row["key"], row["entry"])
            if row["bad"]:
                errors.append("%s: %d pixels differ" % (where, row["bad"]))
            if [c["18"], c["19"]] != tab[row["key"]]["nz"]:
                errors.append("%s: record densities %s, oracle %s" % (where, [c["18"], c["19"]], tab[row["key"]]["nz"]))
            for cnt, key in ((2, "d2"), (10, "d10"), (11, "d11"), (16, "d16"), (20, "d20"), (22, "d22")):
                if delta[str(cnt)] != p[key]:
                    errors.append("%s: counter %d moved by %d, model %d" % (where, cnt, delta[str(cnt)], p[key]))
            if delta["13"] != p["fuse"]:  # (counter 4 stays 0 on these handles: where the model predicts fusion, the counter must move)
                errors.append("%s: counter 13 moved by %d, model %d" % (where, delta["13"], p["fuse"]))
            if c["4"] != 0:
                errors.append("%s: a scanline seam failed (counter 4 = %d)" % (where, c["4"]))
            if option_set == "L8" or geometry == "g160d64":
                if any(c[k] for k in ("13", "16", "20", "22")) or (option_set == "L8" and c["10"]):
                    errors.append("%s: a short-arm form ran where none may (%s)" % (where, c))
    assert not errors, "\n".join(errors[:40])


# ------------------------------------------------------------------------------------------------------------- way out of a hold
def test_two_plans_end_after_the_hold(hip, tables):
    """s, n (the plan switches: two plans from here on), then n until counter 12 reads 0: exactly as many two-plan Matches as the
    hold is set to.  The next n runs ONE plan with gather and flat launches; the next s is redone once, from the aggregation on, and
    switches the mode on again; the n after that runs two plans."""
    A = hip
    hold = M.holds()["agg_dual"]
    tab, _ = tables("g160", "default")
    w, h, _, _ = streams.GEOMETRIES["g160"]
    img = {k: streams.image("g160", k) for k in ("s0", "n0")}
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(streams.option("g160", "default")))
    seen = []

    def match(k):
        before = {c: st.debug_counter(c) for c in (2, 10, 11, 20, 22)}
        got = st.match(*img[k])
        assert _same(got, tab[k]["want"]), "Match %d (%s) differs" % (len(seen), k)
        seen.append(k)
        return {c: st.debug_counter(c) - v for c, v in before.items()}
    try:
        assert match("s0") == {2: 0, 10: 0, 11: 0, 20: 0, 22: 0}
        assert match("n0") == {2: 0, 10: 0, 11: 0, 20: 0, 22: 0}  # (the full ring of the long-arm image stays valid)
        assert st.debug_counter(12) == hold and st.debug_counter(9) == 1
        two_plan = 0
        while st.debug_counter(12) > 0:
            assert two_plan < hold, "the hold outlasts what it is set to"
            d = match("n0")
            assert d == {2: 0, 10: 1, 11: 0, 20: 0, 22: 0}, (two_plan, d)
            two_plan += 1
        assert two_plan == hold
        d = match("n0")  # one plan again: assumed small rings, the previous image's densities
        assert d[10] == 0 and d[2] == 0 and d[20] >= 3 and d[22] == 1, d
        d = match("s0")  # ... and the first long-arm image costs a redo again
        assert d[2] == 1 and d[11] == 1 and d[10] == 0, d
        assert st.debug_counter(12) == hold and st.debug_counter(9) == 2
        d = match("n0")
        assert d == {2: 0, 10: 1, 11: 0, 20: 0, 22: 0}, d
        assert st.debug_counter(4) == 0
    finally:
        st.Release()


SO_HOLD_ENV = {"ADC_SO_SEG": "3", "ADC_SO_FAST": "0"}


@pytest.fixture(scope="module")
def so_hold_rows(hip):
    """the n2w pair 2 x hold + 1 times on one handle, rows cut into three segments with a warm-up of 16 steps (own interpreter)"""
    n = 2 * M.holds()["so_seg_off"] + 1
    rows = _probe(["repeat", "n2w", str(n)], dict(SO_HOLD_ENV, ADC_SO_WARM="16"))["rows"]
    assert len(rows) == n
    return rows


def test_whole_scanline_rows_end_after_the_hold(hip, so_hold_rows):
    """Rows cut into three segments with a warm-up of 16 steps on the n2w pair (own interpreter: the switches are read once): the first
    Match fails a seam and is redone with whole rows (counter 4 = 1), whole rows are kept for the Matches of the hold, then the
    segments are back -- that Match fails and is redone again.  Over two full periods counter 4 reads exactly 3 and moves exactly in
    the first Match of each period; counter 5 reads 1 behind every Match (a redo runs whole rows).  With the production warm-up the same stream has no failed seam, as many segments behind every Match
    as fit 160 columns with that warm-up (two of the three asked for), and the tail moves from the second Match on."""
    hold = M.holds()["so_seg_off"]
    rows, n = so_hold_rows, len(so_hold_rows)
    assert not any(r["bad"] for r in rows), [i for i, r in enumerate(rows) if r["bad"]]
    c4 = [r["c"]["4"] for r in rows]
    c13 = [r["c"]["13"] for r in rows]
    print("counter 4:", c4, "\ncounter 13:", c13)
    assert c4 == [1 + i // hold for i in range(n)], c4
    assert all(r["c"]["5"] == 1 for r in rows) and all(r["c"]["2"] == 0 for r in rows)
    rows = _probe(["repeat", "n2w", str(n)], SO_HOLD_ENV)["rows"]
    assert len(rows) == n and not any(r["bad"] for r in rows)
    nseg = M.so_segments(160, 48, 2, 0, seg_env=3)
    assert nseg == 2
    print("production warm-up: counters 4 / 5 / 2 behind the last Match:", {k: rows[-1]["c"][k] for k in ("4", "5", "2")})
    assert all(r["c"]["4"] == 0 and r["c"]["5"] == nseg and r["c"]["2"] == 0 for r in rows)
    assert [r["c"]["13"] for r in rows] == list(range(n))


def test_whole_scanline_rows_no_match_moves_its_tail(hip, so_hold_rows):
    """Counter 13 moves in no Match of the stream above.  The Matches in which the segments come back (hold and 2 x hold) run on
    arms assumed from a noise image and could move their tail -- but a handle whose seam failed tries its segments on their own first
    (so_seg_probe, adc_so_can_fuse_agg), and in this stream they fail every time."""
    c13 = [r["c"]["13"] for r in so_hold_rows]
    print("counter 13:", c13)
    assert c13 == [0] * len(c13), c13


def test_tail_moves_again_once_the_segments_have_held(hip):
    """The other way out: lambda = (1, 1), cross_t = (2, 1), ADC_SO_FAST=0, production warm-up.  The n2w noise pair saturates the cost and
    fails its seams (counter 4 = 1); the handle then matches the structured s2w pair, whose seams hold and whose arms the low colour
    thresholds keep short.  Whole rows for the Matches of
    the hold; the first Match after it runs segments again, alone (counter 13 still 0); its seams hold, and from the next Match on the
    tail moves in every Match.  Counter 4 stays 1."""
    hold = M.holds()["so_seg_off"]
    n = hold + 3
    rows = _probe(["repeat", "lam11", str(n)], {"ADC_SO_FAST": "0"})["rows"]
    assert len(rows) == n and not any(r["bad"] for r in rows), [i for i, r in enumerate(rows) if r["bad"]]
    c4, c5, c13, c2 = ([r["c"][k] for r in rows] for k in ("4", "5", "13", "2"))
    print("counter 4:", c4, "\ncounter 5:", c5, "\ncounter 13:", c13, "\ncounter 2:", c2)
    nseg = M.so_segments(160, 48, 2, 0)
    assert c4 == [1] * n and c2 == [0] * n
    assert c5 == [1] * hold + [nseg] * 3
    assert c13 == [0] * (hold + 1) + [1, 2]


def test_chained_median_ends_after_the_hold(hip, oracle):
    """240x330, D = 32, structured: a "seam differed" verdict armed through the debug hook makes adc_wait redo the median in the
    chained form; counter 8 then reads 0 for the Matches of the hold (the redone one included) and >= 1 again behind the first
    Match after it; counters 0 and 7 stay at 1."""
    A = hip
    from adcensus_amd import workloads
    from oracle import pyoracle
    hold = M.holds()["med_spec_off"]
    w, h, d = 240, 330, 32
    left, right = workloads.structured_pair(w, h, d, seed=11)
    opt = pyoracle.Option(max_disparity=d)
    want = oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(w, h, cases.to_product_option(opt))
    try:
        assert _same(st.match(left, right), want) and st.debug_counter(8) >= 1 and st.debug_counter(7) == 0
        st.debug_run(A.RUN_MEDIAN, 101)
        for k in range(hold):
            assert _same(st.match(left, right), want), k
            assert st.debug_counter(8) == 0, "Match %d of the hold ran speculative bands" % k
            assert st.debug_counter(0) == 1 and st.debug_counter(7) == 1
        assert _same(st.match(left, right), want)
        assert st.debug_counter(8) >= 1, "the speculative bands did not come back after %d Matches" % hold
        assert st.debug_counter(0) == 1 and st.debug_counter(7) == 1
    finally:
        st.Release()


def test_median_segments_end_after_the_hold(hip):
    """528x400 noise, D = 16, four column segments without a warm-up (own interpreter): the segment seams of the first Match differ,
    the median is redone on whole rows and the handle keeps whole rows (counter 15 = 1).  Both holds are then set on the handle -- by
    the first Match itself when its band seams differ too (counter 8 = 0 behind it), else by a "seam differed" verdict armed for the
    second Match.  The two holds run SIDE BY SIDE: the segments are back exactly med_spec_off Matches after the Match that
    set the chained form -- seen as the next seam failure (counter 7), since behind a redone Match counter 15 reads 1 again."""
    hs, hg = M.holds()["med_spec_off"], M.holds()["med_seg_off"]
    assert hs == hg
    n = hs + 3
    rows = _probe(["repeat", "med528", str(n)], {"ADC_MEDIAN_SEG": "4", "ADC_MEDIAN_WARM": "0"})["rows"]
    assert len(rows) == n and not any(r["bad"] for r in rows), [i for i, r in enumerate(rows) if r["bad"]]
    c7 = [r["c"]["7"] for r in rows]
    c8 = [r["c"]["8"] for r in rows]
    c15 = [r["c"]["15"] for r in rows]
    print("counter 7:", c7, "\ncounter 8:", c8, "\ncounter 15:", c15)
    assert c7[0] == 1 and c15[0] == 1, (c7[0], c15[0])
    start = 0 if c8[0] == 0 else 1  # the Match that set the chained form
    assert c7[start] == start + 1 and c8[start] == 0
    back = start + hs
    assert c7[start:back] == [start + 1] * hs, c7                      # nothing speculative, nothing fails during the hold
    assert all(v == 0 for v in c8[start:back]) and all(v == 1 for v in c15[:back]), (c8, c15)
    assert c7[back] == start + 2, "no segmented attempt %d Matches after the chained form was set (counter 7: %s)" % (hs, c7)


# --------------------------------------------------------------------------------------------------------------------- farm
def test_farm_runs_the_short_arm_forms(hip, tables):
    """PairFarm, three pipelines, 203x40, [-10, 90): twelve pairs of all four classes in a fixed mixed order from pageable host
    buffers, then the same batch in reverse order -- every result equals the oracle's whichever pipeline's learned state it met."""
    A = hip
    tab, _ = tables("g203", "default")
    w, h, _, _ = streams.GEOMETRIES["g203"]
    keys = streams.expand("g203", "nsdrnrsdnsrd")
    imgs = {k: streams.image("g203", k) for k in set(keys)}
    farm = A.PairFarm(w, h, cases.to_product_option(streams.option("g203", "default")), device=0, pipelines=3)
    try:
        done = 0
        for batch in (keys, keys[::-1]):
            outs = [np.full((h, w), -1.0, np.float32) for _ in batch]
            scratch_l, scratch_r = np.empty((h, w, 3), np.uint8), np.empty((h, w, 3), np.uint8)
            for k, o in zip(batch, outs):
                scratch_l[:], scratch_r[:] = imgs[k]
                farm.submit(scratch_l, scratch_r, o)
                scratch_l[:] = 0
                scratch_r[:] = 0
            done += len(batch)
            assert farm.drain() == done  # (pairs delivered since the farm was created)
            bad = [(i, k) for i, (k, o) in enumerate(zip(batch, outs)) if not _same(o, tab[k]["want"])]
            assert not bad, bad
    finally:
        farm.close()
