"""GPU tier: randomly drawn geometries and OPTIONS against the CPU oracle -- aimed at the region voting of round 5 (all ten passes
of multistep_refiner.cpp:153-227 as one fixed-point iteration, irv_plan.h), whose state encoding, band / workgroup layout and vote
depend on image size, disparity range, arm limits and the two voting thresholds: the voting stage in isolation (oracle's LR-checked
map, labels and arms in; oracle's map after the voting out) and the whole Match, bit for bit."""
import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases

pytestmark = pytest.mark.gpu


def _draw(rng):
    w, h = int(rng.integers(40, 520)), int(rng.integers(24, 300))
    d = int(rng.choice([16, 37, 64, 100, 128, 192]))
    dmin = int(rng.choice([0, 0, 0, -9, 5]))
    kind = int(rng.integers(0, 3))
    if kind == 0:
        pair = workloads.structured_pair(w, h, d, seed=int(rng.integers(1, 1 << 30)))
    elif kind == 1:
        pair = workloads.quantized_noise_pair(w, h, d, seed=int(rng.integers(1, 1 << 30)), levels=int(rng.choice([16, 32, 64])))
    else:
        pair = workloads.noise_pair(w, h, seed=int(rng.integers(1, 1 << 30)))
    l1 = int(rng.choice([4, 9, 17, 34, 34, 50]))
    opt = pyoracle.Option(min_disparity=dmin, max_disparity=dmin + d, cross_L1=l1, cross_L2=max(1, l1 // 2),
                          cross_t1=int(rng.integers(8, 40)), cross_t2=int(rng.integers(3, 12)),
                          irv_ts=int(rng.choice([0, 5, 20, 20, 45])), irv_th=float(rng.choice([0.1, 0.3, 0.4, 0.4, 0.7])),
                          lrcheck_thres=float(rng.choice([0.5, 1.0, 1.0, 2.0])))
    return pair, opt


@pytest.mark.parametrize("seed", [101, 202, 303, 404])
def test_random_geometries_and_options_equal_oracle(hip, oracle, seed):
    A = hip
    rng = np.random.default_rng(seed)
    bad = []
    for k in range(6):
        (left, right), opt = _draw(rng)
        h, w = left.shape[:2]
        o = oracle.run(left, right, opt)
        tag = "seed %d case %d: %dx%d [%d, %d) L1 %d ts %d th %.1f" % (seed, k, w, h, opt.min_disparity, opt.max_disparity, opt.cross_L1,
                                                                      opt.irv_ts, opt.irv_th)
        st = A.ADCensusStereo(device=0)
        assert st.Initialize(w, h, cases.to_product_option(opt)), tag
        # the voting stage in isolation
        st.debug_set_images(left, right)
        st.debug_write(A.BUF_ARMS, o["arms"])
        st.debug_write(A.BUF_SUPCOUNT_H, o["sup_count_h"])
        st.debug_write(A.BUF_DISP_LEFT, o["disp_after_lr"])
        st.debug_write(A.BUF_OUTLIER_LABEL, o["outlier_label"])
        st.debug_run(A.RUN_REGION_VOTING)
        got = st.debug_read(A.BUF_DISP_LEFT)
        if not np.array_equal(np.asarray(got).view(np.uint32), o["disp_after_irv"].view(np.uint32)):
            bad.append(tag + " (voting stage: %d pixels)" % int((np.asarray(got).view(np.uint32) != o["disp_after_irv"].view(np.uint32)).sum()))
        # the whole Match, twice (the second one runs on the adapted voting budget / assumed ring depth)
        for rep in range(2):
            d = st.match(left, right)
            if not np.array_equal(d.view(np.uint32), o["disp_final"].view(np.uint32)):
                bad.append(tag + " (Match %d: %d pixels)" % (rep, int((d.view(np.uint32) != o["disp_final"].view(np.uint32)).sum())))
        st.Release()
    assert not bad, bad


@pytest.mark.parametrize("seed", [505, 606])
def test_random_long_arm_limits_equal_oracle(hip, oracle, seed):
    """Long arm limits (49 / 64 / 128 / 255: past the voting slack count's 128-bit window, rings of up to 511 entries) on flat-patch
    images whose arms reach them (tests/cases.py: flat_patch_pair): the voting stage in isolation and the whole Match, bit for bit."""
    A = hip
    rng = np.random.default_rng(seed)
    bad = []
    for k in range(3):
        w, h = int(rng.integers(300, 700)), int(rng.integers(40, 200))
        d = int(rng.choice([16, 32, 64]))
        l1 = int(rng.choice([49, 64, 128, 255]))
        left, right = cases.flat_patch_pair(w, h, d, seed=int(rng.integers(1, 1 << 30)))
        opt = pyoracle.Option(max_disparity=d, cross_L1=l1, cross_L2=int(rng.choice([l1 // 2, l1])),
                              irv_ts=int(rng.choice([0, 5, 20, 45])), irv_th=float(rng.choice([0.1, 0.4, 0.7])))
        o = oracle.run(left, right, opt)
        tag = "seed %d case %d: %dx%d D %d L1 %d L2 %d ts %d th %.1f" % (seed, k, w, h, d, l1, opt.cross_L2, opt.irv_ts, opt.irv_th)
        st = A.ADCensusStereo(device=0)
        assert st.Initialize(w, h, cases.to_product_option(opt)), tag
        st.debug_set_images(left, right)
        st.debug_write(A.BUF_ARMS, o["arms"])
        st.debug_write(A.BUF_SUPCOUNT_H, o["sup_count_h"])
        st.debug_write(A.BUF_DISP_LEFT, o["disp_after_lr"])
        st.debug_write(A.BUF_OUTLIER_LABEL, o["outlier_label"])
        st.debug_run(A.RUN_REGION_VOTING)
        got = np.asarray(st.debug_read(A.BUF_DISP_LEFT)).view(np.uint32)
        if not np.array_equal(got, o["disp_after_irv"].view(np.uint32)):
            bad.append(tag + " (voting stage: %d pixels)" % int((got != o["disp_after_irv"].view(np.uint32)).sum()))
        for rep in range(2):
            dm = st.match(left, right)
            if not np.array_equal(dm.view(np.uint32), o["disp_final"].view(np.uint32)):
                bad.append(tag + " (Match %d: %d pixels)" % (rep, int((dm.view(np.uint32) != o["disp_final"].view(np.uint32)).sum())))
        st.Release()
    assert not bad, bad


# the whole option hull: every numeric field from a list that holds the extremes of the option space (tests/cases.py: OPT_SETS)
# and ordinary values in between.  (lambda_* > 0: the reference divides by them.)
HULL = {
    "lambda_ad": [1, 2, 10, 10, 255, 1000], "lambda_census": [1, 3, 30, 30, 200, 1000],
    "cross_L1": [-5, 0, 1, 2, 9, 17, 34, 34], "cross_L2": [-3, 0, 1, 8, 17, 17, 100000],
    "cross_t1": [-4, 0, 1, 8, 20, 20, 40, 255, 256], "cross_t2": [0, 1, 6, 6, 12, 256, 1000],
    "so_p1": [0.0, 0.01, 0.8, 1.0, 1.0, 3.0, 100.0, 1e5, -1.0], "so_p2": [0.0, 0.03, 1.0, 2.5, 3.0, 3.0, 300.0, 3e5, -3.0],
    "so_tso": [-3, 0, 1, 11, 15, 15, 255, 256, 1000],
    "irv_ts": [-1, 0, 1, 5, 20, 20, 45, 100000], "irv_th": [-0.5, 0.0, 0.1, 0.4, 0.4, 0.7, 0.99, 1.0, 5.0],
    "lrcheck_thres": [-1.0, 0.0, 0.3, 0.5, 1.0, 1.0, 2.0, 1e9],
}
HULL_SEEDS = [1101, 1202, 1303, 1404]


def draw_hull(rng):
    """Geometry and pair as in _draw (whose own sequence stays what it is), then all twelve numeric fields from HULL."""
    pair, opt = _draw(rng)
    for field, values in HULL.items():
        v = rng.choice(values)
        setattr(opt, field, float(v) if isinstance(values[0], float) else int(v))
    return pair, opt


def hull_tag(seed, k, shape, opt):
    return "seed %d case %d: %dx%d [%d, %d) lambda %d/%d L %d/%d t %d/%d P %g/%g tso %d ts %d th %g lr %g" % (
        seed, k, shape[1], shape[0], opt.min_disparity, opt.max_disparity, opt.lambda_ad, opt.lambda_census, opt.cross_L1, opt.cross_L2,
        opt.cross_t1, opt.cross_t2, opt.so_p1, opt.so_p2, opt.so_tso, opt.irv_ts, opt.irv_th, opt.lrcheck_thres)


@pytest.mark.parametrize("seed", HULL_SEEDS)
def test_random_draws_over_the_option_hull_equal_oracle(hip, oracle, seed):
    """4 seeds x 6 draws over the whole option hull (tests/test_oracle.py runs the same draws for port == reference, so they are
    known to be defined behaviour): the voting stage in isolation and two Matches, bit for bit."""
    A = hip
    rng = np.random.default_rng(seed)
    bad = []
    for k in range(6):
        (left, right), opt = draw_hull(rng)
        h, w = left.shape[:2]
        o = oracle.run(left, right, opt)
        tag = hull_tag(seed, k, left.shape, opt)
        st = A.ADCensusStereo(device=0)
        assert st.Initialize(w, h, cases.to_product_option(opt)), tag + ": " + A.last_error()
        st.debug_set_images(left, right)
        st.debug_write(A.BUF_ARMS, o["arms"])
        st.debug_write(A.BUF_SUPCOUNT_H, o["sup_count_h"])
        st.debug_write(A.BUF_DISP_LEFT, o["disp_after_lr"])
        st.debug_write(A.BUF_OUTLIER_LABEL, o["outlier_label"])
        st.debug_run(A.RUN_REGION_VOTING)
        got = np.asarray(st.debug_read(A.BUF_DISP_LEFT)).view(np.uint32)
        if not np.array_equal(got, o["disp_after_irv"].view(np.uint32)):
            bad.append(tag + " (voting stage: %d pixels)" % int((got != o["disp_after_irv"].view(np.uint32)).sum()))
        for rep in range(2):
            d = st.match(left, right)
            if not np.array_equal(d.view(np.uint32), o["disp_final"].view(np.uint32)):
                bad.append(tag + " (Match %d: %d pixels)" % (rep, int((d.view(np.uint32) != o["disp_final"].view(np.uint32)).sum())))
        st.Release()
    assert not bad, bad
