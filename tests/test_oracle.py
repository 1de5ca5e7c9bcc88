"""CPU tier: pins the oracles.

* the golden SHA-256 table tests/golden/golden.json was produced by the REAL reference build
  (oracle/_ref) in the build container (tools/make_golden.py);
* the plain-C port must reproduce every stage dump of every golden case bit-for-bit;
* when oracle/_ref is present it is re-checked against the same table (recipe drift guard).
"""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import cases

with open(os.path.join(cases.GOLDEN_DIR, "golden.json")) as f:
    GOLDEN = json.load(f)["cases"]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _check(oracle, name):
    left, right, opt = cases.make_case(name)
    dumps = oracle.run(left, right, opt)
    bad = [k for k, v in dumps.items() if _sha(cases.canonical(k, v, opt)) != GOLDEN[name][k]]
    assert not bad, "%s oracle differs from the reference golden on %s: %s" % (oracle.kind, name, bad)


def test_golden_table_complete():
    assert set(GOLDEN.keys()) == set(cases.GOLDEN_CASES)


@pytest.mark.parametrize("name", cases.FAST_CASES + ["cone"])
def test_port_matches_reference_golden(port_oracle, name):
    _check(port_oracle, name)


@pytest.mark.parametrize("name", ["cone", "s2_96x64_d32", "q_20x40_d32"])
def test_ref_build_matches_golden(ref_oracle, name):
    if ref_oracle is None:
        pytest.skip("oracle/_ref not built and /root/reference absent")
    _check(ref_oracle, name)


@pytest.mark.parametrize("name", cases.OPT_ALL_CASES)
def test_option_case_changes_its_target_stage(name):
    """A case of the option space (tests/cases.py: OPT_SETS) that changed nothing would test nothing: in the reference's golden
    table the stage its set targets differs from the same pair and range under default options."""
    stage = cases.OPT_TARGET[name]
    assert GOLDEN[name][stage] != GOLDEN[cases.OPT_DEFAULTS[name]][stage], (name, stage)


def test_option_sets_equal_by_construction():
    """so_tso 0 / -3 and 256 / 1000, cross_L1 0 / -5, cross_t1 0 / -4, irv_th 0 / -0.5 and 1 / 5: values on the same side of
    everything the reference compares them with give the same dumps, stage for stage, on every pair."""
    checked = 0
    for a, b in cases.OPT_EQUAL_SETS.items():
        names = [n for n in cases.OPT_ALL_CASES if n.startswith("opt_%s_" % a)]
        assert len(names) >= 2, a
        for n in names:
            twin = n.replace("opt_%s_" % a, "opt_%s_" % b, 1)
            assert GOLDEN[n] == GOLDEN[twin], (n, twin)
            checked += 1
    assert checked >= 2 * len(cases.OPT_EQUAL_SETS)


def test_option_space_is_complete():
    """41 sets, each on two pairs or more; nothing of the out-of-scope kind (lambda <= 0) slipped in."""
    assert len(cases.OPT_SETS) == 41
    for s in cases.OPT_SETS:
        assert len([n for n in cases.OPT_ALL_CASES if n.startswith("opt_%s_" % s)]) >= 2, s
    for n in cases.OPT_ALL_CASES:
        opt = cases.make_case(n)[2] if n.startswith("opt_lam_") else None
        assert opt is None or (opt.lambda_ad > 0 and opt.lambda_census > 0)


@pytest.mark.parametrize("seed", [1101, 1202, 1303, 1404])
def test_random_option_hull_draws_port_equals_reference(port_oracle, ref_oracle, seed):
    """The 24 draws over the whole option hull that the GPU tier runs (tests/test_gpu_random.py: draw_hull): the port equals the
    reference build on every stage dump, and every cost volume is finite -- defined behaviour before a GPU sees them."""
    from tests import test_gpu_random as R
    assert seed in R.HULL_SEEDS and len(R.HULL_SEEDS) == 4
    if ref_oracle is None:
        pytest.skip("oracle/_ref not built and /root/reference absent")
    rng = np.random.default_rng(seed)
    for k in range(6):
        (left, right), opt = R.draw_hull(rng)
        a, b = port_oracle.run(left, right, opt), ref_oracle.run(left, right, opt)
        tag = R.hull_tag(seed, k, left.shape, opt)
        bad = [s for s in a if not np.array_equal(cases.canonical(s, a[s], opt).view(np.uint8), cases.canonical(s, b[s], opt).view(np.uint8))]
        assert not bad, (tag, bad)
        assert all(np.isfinite(b[s]).all() for s in ("cost_init", "cost_aggr", "cost_so")), tag


def test_oracle_initialize_contract(port_oracle, ref_oracle):
    """Initialize -> false for w,h <= 0 or empty disparity range (ADCensusStereo.cpp:31-40)."""
    from oracle import pyoracle
    img = np.zeros((4, 4, 3), np.uint8)
    for orc in [o for o in (port_oracle, ref_oracle) if o is not None]:
        with pytest.raises(RuntimeError):
            orc.run(img, img, pyoracle.Option(min_disparity=5, max_disparity=5))
        with pytest.raises(RuntimeError):
            orc.run(img, img, pyoracle.Option(min_disparity=9, max_disparity=3))


def test_median_is_recursive(port_oracle):
    """The 3x3 median runs in place (adcensus_util.cpp:55-81 with in==out): it must differ from an
    out-of-place median on a generic map -- guards against 'fixing' the oracle."""
    rng = np.random.default_rng(0)
    d = rng.uniform(0, 60, (40, 50)).astype(np.float32)
    rec = port_oracle.median3_inplace(d)
    pad = np.pad(d, 1, constant_values=np.nan)
    win = np.stack([pad[r:r + 40, c:c + 50] for r in range(3) for c in range(3)], -1)
    interior = np.median(win[1:-1, 1:-1], axis=-1)
    assert (rec[1:-1, 1:-1] != interior).mean() > 0.1
