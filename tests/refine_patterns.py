"""Constructed inputs for the refinement stages (tests/test_refine_oracle.py on the CPU, tests/test_gpu_refine_stages.py and
tests/test_gpu_fullsize.py on the GPU): LR check, interpolation and discontinuity adjustment entered directly through
oracle.refine_from / the debug surface, with maps built to hit what the stage dumps of natural images reach only by accident.
Everything is seeded and small.  Every input obeys the rules check_inputs() asserts: no NaN and no -0.0 (the pipeline produces
neither outside the wrapped-count cases), finite right maps, disparities of adjustment inputs inside [min_disparity, max_disparity)
-- the reference's un-offset cost index then stays inside the volume for 1 <= y <= H - 2."""
import math

import numpy as np

from oracle import pyoracle

F = np.float32
INF = F(np.inf)


class Pattern:
    """One stage input.  family / name identify it; opt carries the disparity range (and the LR threshold); disp = the left map;
    label, img (interpolation), disp_right (LR check), cost (adjustment) as the stage needs them; info = what the builder planted."""

    def __init__(self, family, name, opt, disp, label=None, img=None, disp_right=None, cost=None, **info):
        self.family, self.name, self.opt = family, name, opt
        self.disp = np.ascontiguousarray(disp, F)
        self.label = None if label is None else np.ascontiguousarray(label, np.uint8)
        self.img = None if img is None else np.ascontiguousarray(img, np.uint8)
        self.disp_right = None if disp_right is None else np.ascontiguousarray(disp_right, F)
        self.cost = None if cost is None else np.ascontiguousarray(cost, F)
        self.info = info
        check_inputs(self)

    @property
    def geometry(self):
        """what a handle is created for: (W, H, min_disparity, max_disparity, LR threshold)"""
        h, w = self.disp.shape
        return (w, h, self.opt.min_disparity, self.opt.max_disparity, float(self.opt.lrcheck_thres))

    def __repr__(self):
        return "%s/%s" % (self.family, self.name)


def check_inputs(p):
    h, w = p.disp.shape
    for a in (p.disp, p.disp_right, p.cost):
        if a is not None:
            assert not np.isnan(a).any(), p
            assert not (np.signbit(a) & (a == 0)).any(), p  # no -0.0
            assert not (a == -np.inf).any(), p
    if p.disp_right is not None:
        assert p.disp_right.shape == (h, w) and np.isfinite(p.disp_right).all(), p
    if p.label is not None:
        assert p.label.shape == (h, w) and p.label.max(initial=0) <= 2, p
    if p.img is not None:
        assert p.img.shape == (h, w, 3), p
    if p.cost is not None:
        d = p.opt.max_disparity - p.opt.min_disparity
        assert p.cost.shape == (h, w, d) and np.isfinite(p.cost).all(), p
        fin = p.disp[np.isfinite(p.disp)]
        assert ((fin >= p.opt.min_disparity) & (fin < p.opt.max_disparity)).all(), p
        assert (fin == np.floor(fin)).all(), p  # integer plateaus: lround(d) == d


def _opt(dmin, dmax, **kw):
    return pyoracle.Option(min_disparity=dmin, max_disparity=dmax, **kw)


def search_range(opt):
    return max(abs(opt.max_disparity), abs(opt.min_disparity))  # multistep_refiner.cpp:236


# ------------------------------------------------------------------------------------------------ interpolation
def ray_offset(s, m):
    """(dx, dy) of step m of ray s from a target in row 0: the arithmetic of multistep_refiner.cpp:254-268 (ang += pi / 16 with the
    float pi, a float divide, widened on the addition; double sin / cos; lround).  tests/test_refine_oracle.py confirms every
    position planted with it by the reference's own walk: found with a range that includes step m, not found by a shorter one."""
    ang = 0.0
    step = float(F(3.1415926) / F(16))
    for _ in range(s):
        ang += step

    def lround(v):
        return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)
    return lround(m * math.cos(ang)), lround(0 + m * math.sin(ang))


REACH_MS = (2, 3, 7, 33, 64, 65)
REACH_STEPS = (1, 2, 3, 6, 7, 10, 11)


def reach_value(s):
    return F(s * 3 - 20) + F(0.25)  # 16 distinct values, negative for s <= 6, never 0.0 (the fill of a target no ray finds)


def reach_geometry(ms):
    """(W, H, target x, target y): rays run to the right, to the left and downwards (0 <= angle < pi), ms steps at the most"""
    return 2 * ms + 5, ms + 2, ms + 2, 0


def reach(ms):
    """One target, one valid pixel at step m of ray s, for the 16 rays and m in {1, 2, 3, 6, 7, 10, 11, ms - 1, ms} (1 <= m <= ms).
    Step ms lies outside the walk (m < max_search): not found, the fill is 0.0f -- unless an earlier step of some ray rounds to
    the same pixel (the 45-degree ray's steps 1 and 2 do), which info["found"] says.  The label alternates between the lists."""
    w, h, tx, ty = reach_geometry(ms)
    earlier = {ray_offset(s, m) for s in range(16) for m in range(1, ms)}
    img = np.zeros((h, w, 3), np.uint8)
    img[:] = (90, 90, 90)
    out = []
    for m in sorted({m for m in REACH_STEPS + (ms - 1, ms) if 1 <= m <= ms}):
        for s in range(16):
            dx, dy = ray_offset(s, m)
            disp = np.full((h, w), INF, F)
            disp[ty + dy, tx + dx] = reach_value(s)
            label = np.zeros((h, w), np.uint8)
            label[ty, tx] = 1 + (s + m) % 2
            im = img.copy()
            im[ty + dy, tx + dx] = (10 * s + 5, 255 - 10 * s, 7 * s)
            out.append(Pattern("reach", "ms%d_m%d_s%d" % (ms, m, s), _opt(0, ms), disp, label, im, target=(ty, tx),
                               planted=(ty + dy, tx + dx), found=m < ms or (dx, dy) in earlier))
    return out


def _first_hits(disp, ty, tx, ms):
    """[(y, x) or None per ray]: the walk of one target restated with ray_offset (builders' self-check only)"""
    h, w = disp.shape
    hits = []
    for s in range(16):
        hit = None
        for m in range(1, ms):
            dx, dy = ray_offset(s, m)
            y, x = ty + dy, tx + dx
            if not (0 <= y < h and 0 <= x < w):
                break
            if disp[y, x] != INF:
                hit = (y, x)
                break
        hits.append(hit)
    return hits


TIE_MS, TIE_STEP = 33, 9


def tie():
    """All 16 rays hit, at step TIE_STEP, 16 distinct values (seven negative) -- on a uniform image (every colour distance equal: the
    mismatch fill is ray 0's value) and on a 4-level image (several rays share the smallest distance: the first of them in ray
    order), each once as a mismatch and once as an occlusion (the smallest value).  info["values"] / ["colours"]: per ray."""
    ms = TIE_MS
    w, h, tx, ty = reach_geometry(ms)
    values = [F((s * 7 + 5) % 16 - 6) + F(0.5) for s in range(16)]  # (the smallest belongs to ray 13)
    disp = np.full((h, w), INF, F)
    spots = [(ty + ray_offset(s, TIE_STEP)[1], tx + ray_offset(s, TIE_STEP)[0]) for s in range(16)]
    assert len(set(spots)) == 16
    for s, (y, x) in enumerate(spots):
        disp[y, x] = values[s]
    assert _first_hits(disp, ty, tx, ms) == spots  # every ray meets its own pixel first
    levels = [3, 2, 1, 2, 0, 3, 1, 1, 2, 0, 3, 1, 0, 2, 3, 1]  # target level 1: rays 2, 6, 7, 11, 15 tie at distance 0
    out = []
    for kind in ("uniform", "levels"):
        img = np.full((h, w, 3), 60, np.uint8)
        if kind == "levels":
            for s, (y, x) in enumerate(spots):
                img[y, x] = 60 * levels[s]
        for which in (1, 2):
            label = np.zeros((h, w), np.uint8)
            label[ty, tx] = which
            out.append(Pattern("tie", "%s_list%d" % (kind, which), _opt(0, ms), disp, label, img, target=(ty, tx), values=values,
                               colours=[int(img[y, x, 0]) for y, x in spots], own_colour=60))
    return out


def two_pass():
    """Occlusion targets whose nearest hit on a ray is a mismatch target (19 x 9, range [0, 7)).  Bottom row: mismatch A (2, 8) is
    filled with 5.0 from the valid pixel (8, 8), six steps to its right; mismatch B (16, 8) finds nothing (two invalid pixels on
    either side, then the border) and gets 0.0f.  Three rows up: occlusion O1 (2, 5) meets A straight below it and nothing else
    -- 5.0, or no hit at all when A's fill is withheld; occlusion O2 (16, 5) meets B below it and the valid 7.0 at (18, 5) --
    min(7.0, 0.0f) = 0.0f, or 7.0 when B's fill is withheld."""
    w, h, ms = 19, 9, 7
    disp = np.full((h, w), INF, F)
    label = np.zeros((h, w), np.uint8)
    disp[8, 8], disp[5, 18] = 5.0, 7.0
    label[8, 2] = label[8, 16] = 1
    label[5, 2] = label[5, 16] = 2
    img = (np.arange(h * w * 3, dtype=np.int64).reshape(h, w, 3) * 37 % 251).astype(np.uint8)
    return [Pattern("two_pass", "19x9", _opt(0, ms), disp, label, img, a=(8, 2), b=(8, 16), o1=(5, 2), o2=(5, 16))]


def random_draw(seed, density, w, h, dense_half=True):
    """The draw of test_interpolation_on_the_code_map_is_exact (tests/test_emul.py): valid pixels of the given density, a dense
    region (0.3) from column 100 on, disparities 0..90 with random fractions, random labels -- and an image of 8 levels per
    channel, so that colour distances tie."""
    rng = np.random.default_rng(seed)
    valid = rng.random((h, w)) < density
    if dense_half and w > 100:
        valid[:, 100:] |= rng.random((h, w - 100)) < 0.3
    disp = np.where(valid, rng.integers(0, 90, (h, w)).astype(F) + rng.random((h, w)).astype(F), INF).astype(F)
    label = rng.integers(0, 3, (h, w)).astype(np.uint8)
    img = (rng.integers(0, 8, (h, w, 3)) * 32).astype(np.uint8)
    return disp, label, img


RANDOM_SHAPES = ((157, 83, 96), (7, 150, 30), (150, 7, 5), (1, 1, 9), (97, 31, 1), (50, 40, 576), (50, 40, 577), (203, 61, 600))
RANDOM_DENSITIES = (0.0, 0.0005, 0.003, 0.25, 1.0)
# seeds of the maps whose first draw (seed 1000 * shape index + density index) does not reach the floor of 10 occlusion fills that depend
# on a first-pass fill (tests/test_refine_oracle.py): a 50 x 40 map of density 0.0005 needs a valid pixel to begin with
RANDOM_SEEDS = {(6, 1): 24900}


def random_maps(shape_index):
    w, h, ms = RANDOM_SHAPES[shape_index]
    out = []
    for k, density in enumerate(RANDOM_DENSITIES):
        seed = RANDOM_SEEDS.get((shape_index, k), 1000 * shape_index + k)
        disp, label, img = random_draw(seed, density, w, h)
        out.append(Pattern("random", "%dx%d_ms%d_d%g" % (w, h, ms, density), _opt(0, ms), disp, label, img, density=density))
    return out


def random_can_depend(p):
    """a fill of this map can depend on another pixel at all: there is a neighbour, and the walk takes a step"""
    return p.disp.size > 1 and search_range(p.opt) > 1


MANY_MS = 64


def many():
    """256 x 160, density 0.0005, every pixel on ONE list (all labels 1 / all labels 2): more than 32768 targets, so the grid-stride
    loop of the walk runs a second iteration and its list prefetch is used."""
    out = []
    for which in (1, 2):
        disp, _, img = random_draw(7000 + which, 0.0005, 256, 160, dense_half=False)
        assert int(np.isinf(disp).sum()) > 32768
        out.append(Pattern("many", "list%d" % which, _opt(0, MANY_MS), disp, np.full(disp.shape, which, np.uint8), img))
    return out


def edge_2p24(w):
    """Range [2045, 2047), H = 3: search range 2047.  W = 4094 pads to a pitch of 8196 -- 2047 * 8196 = 2^24 - 4, the last handle on the
    table walk; W = 4095 takes the f64 walk.  A sparse random map with a mismatch and an occlusion target at the left border whose
    only hit lies 2046 and 2045 steps to the right."""
    disp, label, img = random_draw(8000 + w, 0.003, w, 3, dense_half=False)
    disp[1, :2047] = INF
    label[1, :2047] = 0
    disp[1, 2046] = F(2045.5)
    label[1, 0], label[1, 1] = 1, 2
    return Pattern("edge_2p24", "w%d" % w, _opt(2045, 2047), disp, label, img)


def edge_2p24_full(s):
    """4094 x 2048, range [2045, 2047): one target in row 0, one valid pixel at step 2046 of ray s (7, 8, 9: the steepest rays) -- the
    hit's linear offset in the padded map, 2046 * 8196 + dx + 2047, is the largest value the walk's float division ever sees."""
    w, h, ms = 4094, 2048, 2047
    tx, ty = 2047, 0
    dx, dy = ray_offset(s, ms - 1)
    disp = np.full((h, w), INF, F)
    disp[ty + dy, tx + dx] = reach_value(s)
    label = np.zeros((h, w), np.uint8)
    label[ty, tx] = 1 + s % 2
    img = np.full((h, w, 3), 90, np.uint8)
    return Pattern("edge_2p24", "full_s%d" % s, _opt(2045, 2047), disp, label, img, target=(ty, tx), planted=(ty + dy, tx + dx))


OFFSET_RANGE = (30001, 30017)


def offset():
    """64 x 32 at [30001, 30017): search range 30017 > 30000 -- the f64 walk by the production predicate."""
    out = []
    for k, density in enumerate((0.003, 0.25)):
        disp, label, img = random_draw(9000 + k, density, 64, 32)
        out.append(Pattern("offset", "d%g" % density, _opt(*OFFSET_RANGE), disp, label, img, density=density))
    return out


def interpolation_small():
    """every interpolation pattern up to 203 x 61 and the `many` pair's size that the table walk takes: what both GPU walks and the
    CPU emulations run"""
    out = []
    for ms in REACH_MS:
        out += reach(ms)
    out += tie() + two_pass()
    for i in range(len(RANDOM_SHAPES)):
        out += random_maps(i)
    return out


# ------------------------------------------------------------------------------------------------------ LR check
LR_SIZES = ((70, 9), (64, 5), (65, 5), (1, 4), (2, 1))
RANGES = ((0, 16), (-6, 10), (3, 19))
LR_THRESHOLDS = (0.0, 0.25, 1.0)
LR_SEED = 100


def lr_set(rng_index):
    """The LR patterns of one disparity range: every size x threshold.  Left and right maps of quarter-integers in [min - 3, max + 3]
    (x - d and col_right + disp_r sit on a .5 tie for every fourth value: dense lroundf ties), 10 % of the left pixels +inf; one
    pixel of every map at least 3 wide is set, with values of the same kind, so that its col_rl is 0."""
    dmin, dmax = RANGES[rng_index]
    out = []
    for si, (w, h) in enumerate(LR_SIZES):
        for ti, thres in enumerate(LR_THRESHOLDS):
            rng = np.random.default_rng(LR_SEED + 100 * rng_index + 10 * si + ti)
            lo, hi = 4 * (dmin - 3), 4 * (dmax + 3)
            left = (rng.integers(lo, hi + 1, (h, w)).astype(F) * F(0.25)).astype(F)
            right = (rng.integers(lo, hi + 1, (h, w)).astype(F) * F(0.25)).astype(F)
            left[rng.random((h, w)) < 0.10] = INF
            left, right = left + F(0), right + F(0)  # (-0.0 + 0.0 = +0.0)
            if w >= 3:  # the col_rl == 0 quirk, once per map (a draw meets it only now and then, and hardly ever in a range above 0):
                left[0, 2], right[0, 0] = 2.0, 0.25  # col_right = lround(2 - 2.0) = 0, |2.0 - 0.25| > thres, col_rl = lround(0 + 0.25) = 0
            out.append(Pattern("lr", "%dx%d_r%d_t%g" % (w, h, rng_index, thres), _opt(dmin, dmax, lrcheck_thres=thres), left, disp_right=right))
    return out


def lroundf(v):
    v = float(F(v))
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def lr_classes(p, label_ref):
    """Counts of the LR check's branches on one pattern (multistep_refiner.cpp:104-150), from the inputs and the REFERENCE's label map:
    the branch taken is recomputed per pixel with the raster scan's in-place state, and the label it implies must be the
    reference's.  `late_occlusion`: labelled occlusion although the ORIGINAL left map at col_rl does not exceed d -- the pixel at
    col_rl < x had been invalidated before."""
    h, w = p.disp.shape
    thres = F(p.opt.lrcheck_thres)
    cur = p.disp.copy()
    n = dict(consistent=0, invalid_in=0, col_right_out=0, col_rl_out=0, col_rl_zero=0, mismatch_le=0, occlusion=0, late_occlusion=0)
    for y in range(h):
        for x in range(w):
            d = cur[y, x]
            if d == INF:
                n["invalid_in"] += 1
                want = 1
            else:
                cr = lroundf(F(x) - d)
                if not 0 <= cr < w:
                    n["col_right_out"] += 1
                    want = 1
                else:
                    dr = p.disp_right[y, cr]
                    if not abs(F(d - dr)) > thres:
                        n["consistent"] += 1
                        want = 0
                    else:
                        crl = lroundf(F(cr) + dr)
                        if not 0 < crl < w:
                            n["col_rl_out"] += 1
                            n["col_rl_zero"] += crl == 0
                            want = 1
                        elif cur[y, crl] > d:
                            n["occlusion"] += 1
                            n["late_occlusion"] += not p.disp[y, crl] > d
                            want = 2
                        else:
                            n["mismatch_le"] += 1
                            want = 1
                if want:
                    cur[y, x] = INF
            assert label_ref[y, x] == want, (p, y, x, int(label_ref[y, x]), want)
    return n, cur


# ------------------------------------------------------------------------------------ discontinuity adjustment
DDA_SIZES = ((2, 5), (3, 3), (66, 70))
DDA_SEED = 300


def dda_set(rng_index):
    """The adjustment patterns of one disparity range: integer plateaus (column stripes 1..5 wide whose level moves by -3 .. +4 from
    stripe to stripe, row bands moving by -1 .. +1: steps of 1 stay below the Sobel threshold of 5, steps of 2 and more lie above
    it), 5 % of the pixels +inf, a random f32 volume."""
    dmin, dmax = RANGES[rng_index]
    out = []
    for si, (w, h) in enumerate(DDA_SIZES):
        rng = np.random.default_rng(DDA_SEED + 10 * rng_index + si)
        col = np.empty(w, np.int64)
        x, lev = 0, int(rng.integers(dmin + 4, dmax - 4))
        while x < w:
            n = int(rng.integers(1, 6))
            col[x:x + n] = lev
            lev = int(np.clip(lev + rng.choice([-3, -2, -1, 1, 2, 4]), dmin + 1, dmax - 2))
            x += n
        row = np.cumsum(rng.integers(-1, 2, h) * (rng.random(h) < 0.3))
        disp = np.clip(col[None, :] + row[:, None], dmin, dmax - 1).astype(F)
        disp[rng.random((h, w)) < 0.05] = INF
        cost = rng.random((h, w, dmax - dmin)).astype(F)
        img = (rng.integers(0, 8, (h, w, 3)) * 32).astype(np.uint8)
        out.append(Pattern("dda", "%dx%d_r%d" % (w, h, rng_index), _opt(dmin, dmax), disp, img=img, cost=cost))
    return out


def inf_in_window(disp):
    """[H][W] bool: the pixel's 3 x 3 window holds a +inf"""
    h, w = disp.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = np.isinf(disp)
    out = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            out |= pad[dy:dy + h, dx:dx + w]
    return out
