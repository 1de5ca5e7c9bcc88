"""GPU tier: the LR check, the interpolation (table walk AND f64 walk) and the discontinuity adjustment on the constructed inputs of
tests/refine_patterns.py -- debug_set_images, debug_write of the inputs, debug_run of the ONE stage, bitwise comparison with the
oracle entered at that stage (oracle.refine_from).  One handle per geometry.  tests/test_refine_oracle.py shows on the CPU that
the inputs reach the branches they were built for; here the kernels must give what the reference gives on them."""
import numpy as np
import pytest

from oracle import pyoracle
from oracle.pyoracle import DDA, INTERP, LR
from tests import cases
from tests import refine_patterns as rp

pytestmark = pytest.mark.gpu

TABLE_WALK, F64_WALK = 0, 1  # arg of debug_run(RUN_INTERPOLATION): the handle's own walk / the f64 walk


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def oracle(ref_oracle, port_oracle):
    """the checker of this module: pyoracle.stage_entry_oracle (a reference build that has refine_from, else the port)"""
    return pyoracle.stage_entry_oracle(ref_oracle, port_oracle)


class Handle:
    def __init__(self, A, geometry):
        w, h, dmin, dmax, thres = geometry
        self.A, self.st = A, A.ADCensusStereo(device=0)
        opt = pyoracle.Option(min_disparity=dmin, max_disparity=dmax, lrcheck_thres=thres)
        if not self.st.Initialize(w, h, cases.to_product_option(opt)):
            raise RuntimeError("Initialize failed: " + A.last_error())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.st.Release()

    def interpolate(self, p, arg):
        A, st = self.A, self.st
        st.debug_set_images(p.img, p.img)
        st.debug_write(A.BUF_DISP_LEFT, p.disp)
        st.debug_write(A.BUF_OUTLIER_LABEL, p.label)
        st.debug_run(A.RUN_INTERPOLATION, arg)
        return st.debug_read(A.BUF_DISP_LEFT)

    def lr_check(self, p):
        A, st = self.A, self.st
        st.debug_write(A.BUF_DISP_LEFT, p.disp)
        st.debug_write(A.BUF_DISP_RIGHT, p.disp_right)
        st.debug_run(A.RUN_LRCHECK)
        return st.debug_read(A.BUF_DISP_LEFT), st.debug_read(A.BUF_OUTLIER_LABEL)

    def adjust(self, p):
        A, st = self.A, self.st
        st.debug_set_images(p.img, p.img)
        st.debug_write(A.BUF_DISP_LEFT, p.disp)
        st.debug_write(A.BUF_VOLUME_A, p.cost)
        st.debug_run(A.RUN_DISCONTINUITY)
        return st.debug_read(A.BUF_DISP_LEFT)


def by_geometry(patterns):
    groups = {}
    for p in patterns:
        groups.setdefault(p.geometry, []).append(p)
    return groups


def check_interpolation(A, oracle, patterns, walks):
    """every pattern through every walk of `walks`, one handle per geometry; returns the failures"""
    bad = []
    for geometry, group in by_geometry(patterns).items():
        with Handle(A, geometry) as hd:
            for p in group:
                want, _ = oracle.refine_from(INTERP, INTERP, p.disp, p.opt, left=p.img, label=p.label)
                for arg in walks:
                    got = hd.interpolate(p, arg)
                    n = int((bits(got) != bits(want)).sum())
                    if n:
                        y, x = (int(v) for v in np.argwhere(bits(got) != bits(want))[0])
                        bad.append("%r walk %d: %d pixels differ, first (%d, %d) got %r want %r" % (p, arg, n, y, x, float(got[y, x]), float(want[y, x])))
    return bad


@pytest.mark.parametrize("rng_index", range(len(rp.RANGES)))
def test_lr_check_on_constructed_maps(hip, oracle, rng_index):
    """Quarter-integer maps (dense lroundf ties), col_rl == 0, pixels at col_rl that an earlier pixel of the raster scan had
    invalidated: the map AND the labels, for every size x threshold of the range."""
    bad = []
    for geometry, group in by_geometry(rp.lr_set(rng_index)).items():
        with Handle(hip, geometry) as hd:
            for p in group:
                want, want_label = oracle.refine_from(LR, LR, p.disp, p.opt, disp_right=p.disp_right)
                got, got_label = hd.lr_check(p)
                n, m = int((bits(got) != bits(want)).sum()), int((got_label != want_label).sum())
                if n or m:
                    bad.append("%r: %d map pixels, %d labels differ" % (p, n, m))
    assert not bad, bad


@pytest.mark.parametrize("ms", rp.REACH_MS)
def test_interpolation_reach(hip, oracle, ms):
    """One target, one valid pixel at step m of ray s -- every ray, the first steps, the trip boundaries (2 | 4 | 4 steps), the last
    step of the range and the first one outside it -- through both walks."""
    bad = check_interpolation(hip, oracle, rp.reach(ms), (TABLE_WALK, F64_WALK))
    assert not bad, bad[:10]


def test_interpolation_ties_and_second_pass(hip, oracle):
    """All 16 rays hit: first ray in order among equal colour distances (mismatch), smallest value (occlusion); occlusion targets
    whose nearest hit is a first-pass fill, a real one and a no-hit 0.0f."""
    bad = check_interpolation(hip, oracle, rp.tie() + rp.two_pass(), (TABLE_WALK, F64_WALK))
    assert not bad, bad


@pytest.mark.parametrize("shape_index", range(len(rp.RANDOM_SHAPES)))
def test_interpolation_random_maps(hip, oracle, shape_index):
    """Random maps of five densities per shape: odd sizes, one row / one column / one pixel, search range 1, the last ray table that
    fits LDS (576) and the first that is read from global memory (577; 600 with walks of 200 steps through an empty band)."""
    bad = check_interpolation(hip, oracle, rp.random_maps(shape_index), (TABLE_WALK, F64_WALK))
    assert not bad, bad


def test_interpolation_many_targets_then_one(hip, oracle):
    """More than 32768 targets on one list: the walk's grid-stride loop runs its second iteration (the list prefetch).  Then a
    single-target map on the same handle: no list or counter state survives."""
    pats = rp.many()
    _, _, tx, ty = rp.reach_geometry(rp.MANY_MS)
    h, w = pats[0].disp.shape
    after = []
    for s, m in ((3, 7), (12, 63)):  # one target in row 0 of the 256 x 160 image, one valid pixel on ray s at step m
        dx, dy = rp.ray_offset(s, m)
        disp = np.full((h, w), np.inf, np.float32)
        disp[ty + dy, tx + dx] = rp.reach_value(s)
        label = np.zeros((h, w), np.uint8)
        label[ty, tx] = 1 + s % 2
        after.append(rp.Pattern("reach", "after_many_s%d_m%d" % (s, m), pats[0].opt, disp, label, pats[0].img))
    bad = check_interpolation(hip, oracle, [pats[0], after[0], pats[1], after[1]], (TABLE_WALK, F64_WALK))
    assert not bad, bad


@pytest.mark.parametrize("w", [4094, 4095])
def test_interpolation_at_the_table_walks_edge(hip, oracle, w):
    """Range [2045, 2047) at H = 3: W = 4094 is the last width on the table walk (2047 * 8196 = 2^24 - 4), W = 4095 takes the f64 walk
    by the production predicate (tests/test_emul_itp_plan.py pins both sides)."""
    bad = check_interpolation(hip, oracle, [rp.edge_2p24(w)], (TABLE_WALK,))
    assert not bad, bad


def test_interpolation_and_match_at_a_large_offset(hip, oracle, port_oracle):
    """[30001, 30017) at 64 x 32: a search range above 30000 -- the f64 walk by the production predicate, on a handle that allocates
    no code maps (itp_plan.h) -- and one whole Match of a seeded pair at that offset.  The Match is compared with the PORT: with
    every candidate column outside the image the reference's right-view winner-takes-all reads cost_local[-1 - min_disparity]
    (ADCensusStereo.cpp:296-298), 120 KB in front of a 64-byte vector; the port restates the pipeline without that read, and the
    LR check never consumes the right-view map there (every col_right is outside the image)."""
    bad = check_interpolation(hip, oracle, rp.offset(), (TABLE_WALK,))
    assert not bad, bad
    from adcensus_amd import workloads
    left, right = workloads.quantized_noise_pair(64, 32, 16, seed=61)
    opt = pyoracle.Option(min_disparity=rp.OFFSET_RANGE[0], max_disparity=rp.OFFSET_RANGE[1])
    want = port_oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    st = hip.ADCensusStereo(device=0)
    assert st.Initialize(64, 32, cases.to_product_option(opt)), hip.last_error()
    try:
        got = st.match(left, right)
    finally:
        st.Release()
    assert int((bits(got) != bits(want)).sum()) == 0


@pytest.mark.parametrize("rng_index", range(len(rp.RANGES)))
def test_discontinuity_adjustment_on_constructed_maps(hip, oracle, rng_index):
    """Integer plateaus with steps on both sides of the Sobel threshold and +inf pixels (never met before: the pipeline runs the
    adjustment behind the filling), widths 2 and 3, 70 rows = two workgroups of the row kernel, min_disparity < 0, = 0 and > 0."""
    bad = []
    for geometry, group in by_geometry(rp.dda_set(rng_index)).items():
        with Handle(hip, geometry) as hd:
            for p in group:
                want, _ = oracle.refine_from(DDA, DDA, p.disp, p.opt, cost=p.cost, label=np.zeros(p.disp.shape, np.uint8))
                got = hd.adjust(p)
                n = int((bits(got) != bits(want)).sum())
                if n:
                    bad.append("%r: %d pixels differ" % (p, n))
    assert not bad, bad
