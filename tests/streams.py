"""Image streams for the state a handle LEARNS from its earlier Matches (tests/stream_model.py, tests/stream_probe.py,
tests/test_stream_model.py, tests/test_gpu_streams.py): four image classes built from the generators the suite already has, the
geometries and option sets they run under, the orders they are matched in, and what the oracle says about each image.

  n  uniform noise: arms 0 .. 2, 1 .. 2 % of the pixels with a pass-changing record
  d  short arms, record density above the sparse threshold (dense_pair / planted_pair of tests/test_gpu_sparse_agg.py, alternately)
  r  noise with planted runs (tests/gather_patterns.py): arms 5 .. 8 -- too deep for the fused tail, up to the small-ring limit;
     alternately both directions (runs of 6 .. 9), vertical runs only and horizontal runs only (runs of 6): one depth gate each
  s  arms beyond the small ring (workloads.structured_pair / cases.flat_patch_pair, alternately)
"""
import numpy as np

from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases, gather_patterns

CLASSES = "ndrs"

# name: (W, H, min_disparity, max_disparity) -- the smallest sizes at which the forms still differ
GEOMETRIES = {
    "g160": (160, 48, 0, 128),     # two scanline segments per row, no more fit
    "g203": (203, 40, -10, 90),    # 100 of 128 lanes used, the rest padding; flat tile remainder 75
    "g321": (321, 37, 5, 261),     # two 128-float chunks; tile remainder 65
    "g160d64": (160, 48, 0, 64),   # one disparity per lane: no sparse form may ever run
}

OPTION_SETS = {
    "default": {},
    "L9": dict(cross_L1=9, cross_L2=4),      # the narrowest limit that still has a small ring
    "L8": dict(cross_L1=8, cross_L2=4),      # none: agg_small_ok is false
    "cost": dict(lambda_ad=2, lambda_census=200),
    "arm_t": dict(cross_t1=40, cross_t2=12),  # noise arms grow
    "L255": dict(cross_L1=255, cross_L2=255),
}

# (geometry, option set) pairs that run: the default set everywhere, every other set on two geometries
COMBOS = [("g160", "default"), ("g203", "default"), ("g321", "default"), ("g160d64", "default"),
          ("g160", "L9"), ("g203", "L9"), ("g160", "L8"), ("g321", "L8"), ("g203", "cost"), ("g321", "cost"),
          ("g160", "arm_t"), ("g203", "arm_t"), ("g321", "L255"), ("g160d64", "L255")]

# 17 Matches with every ordered transition between the four classes, the self-transitions included (a de Bruijn sequence B(4, 2),
# written out linearly); the short-arm transitions come first: the first n -> s switch puts the handle into the two-plan mode
FIXED_ORDER = "nnddrrnrdnssdsrsn"

ENTRIES = ("match", "match_async", "match_device")


def option(geometry, option_set):
    w, h, dmin, dmax = GEOMETRIES[geometry]
    return pyoracle.Option(min_disparity=dmin, max_disparity=dmax, **OPTION_SETS[option_set])


def random_orders(geometry):
    """The seeded random order of 24 Matches of a geometry as two blocks of 12, each for a fresh handle: short-arm classes only (after
    the first s -> n switch a handle sits in the two-plan mode for the rest of a short stream), then all four."""
    rng = np.random.default_rng(7000 + sorted(GEOMETRIES).index(geometry))
    short = "".join("ndr"[int(k)] for k in rng.integers(0, 3, 12))
    mixed = "".join(CLASSES[int(k)] for k in rng.integers(0, 4, 12))
    return short, mixed


def stream_orders(geometry):
    """{stream name: order}: every stream runs on a handle of its own"""
    short, mixed = random_orders(geometry)
    return {"fixed": FIXED_ORDER, "short": short, "mixed": mixed}


def _variants(geometry):
    """{class: [builders]}: the k-th image of a class in a stream is variant k % len"""
    from tests import test_gpu_sparse_agg as sparse
    w, h, dmin, dmax = GEOMETRIES[geometry]
    d = dmax - dmin
    base = 8100 + 100 * sorted(GEOMETRIES).index(geometry)
    return {
        "n": [lambda: workloads.noise_pair(w, h, seed=base + 1), lambda: workloads.noise_pair(w, h, seed=base + 2)],
        "d": [lambda: sparse.dense_pair(w, h, seed=base + 11), lambda: sparse.planted_pair(w, h, seed=base + 12)],
        "r": [lambda: gather_patterns.run_pair(w, h, seed=base + 21, lengths=(6, 7, 8, 9)),
              lambda: gather_patterns.run_pair(w, h, seed=base + 22, horizontal=False, lengths=(6,)),
              lambda: gather_patterns.run_pair(w, h, seed=base + 23, vertical=False, lengths=(6,))],
        "s": [lambda: workloads.structured_pair(w, h, d, seed=base + 31),
              lambda: cases.flat_patch_pair(w, h, d, seed=base + 32, patch_w=(30, 120), patch_h=(12, 40), band_h=(6, 20))],
    }


def image_keys(geometry):
    """every image of a geometry as "class + variant index" ("r1")"""
    return [c + str(k) for c, v in _variants(geometry).items() for k in range(len(v))]


def image(geometry, key):
    l, r = _variants(geometry)[key[0]][int(key[1:])]()
    return np.ascontiguousarray(l), np.ascontiguousarray(r)


def expand(geometry, order):
    """order of classes -> the image key of every Match (the variants of a class alternate within the stream)"""
    n = {c: len(v) for c, v in _variants(geometry).items()}
    seen = {c: 0 for c in CLASSES}
    out = []
    for c in order:
        out.append(c + str(seen[c] % n[c]))
        seen[c] += 1
    return out


def facts_from(arms, sup_count_h, sup_count_v):
    """What a Match of this image must leave on the handle, from the oracle's dumps: armmax = (longest horizontal, longest vertical)
    arm; nz = the pixels with a pass-changing horizontal / vertical record as adc_rec_changes_pixel(rec, true) defines them on the
    records k_make_records packs -- horizontal: left | right != 0 or the VERTICAL support count != 1, vertical: up | down != 0 or the
    HORIZONTAL support count != 1; the counts as stored (uint16)."""
    a = np.asarray(arms)
    sh, sv = np.asarray(sup_count_h).astype(np.uint16), np.asarray(sup_count_v).astype(np.uint16)
    nzh = ((a[..., 0] != 0) | (a[..., 1] != 0) | (sv != 1))
    nzv = ((a[..., 2] != 0) | (a[..., 3] != 0) | (sh != 1))
    return {"armmax": [int(a[..., 0:2].max()), int(a[..., 2:4].max())], "nz": [int(nzh.sum()), int(nzv.sum())]}


def facts(oracle, pair, opt):
    o = oracle.run(pair[0], pair[1], opt, stages=["arms", "sup_count_h", "sup_count_v"])
    return facts_from(o["arms"], o["sup_count_h"], o["sup_count_v"])


def oracle_table(oracle, geometry, option_set, keys=None):
    """{image key: {"armmax", "nz", "want" (disp_final)}}: one oracle run per image, shared by everything that needs it"""
    opt = option(geometry, option_set)
    out = {}
    for key in (keys or image_keys(geometry)):
        l, r = image(geometry, key)
        o = oracle.run(l, r, opt, stages=["arms", "sup_count_h", "sup_count_v", "disp_final"])
        out[key] = dict(facts_from(o["arms"], o["sup_count_h"], o["sup_count_v"]), want=o["disp_final"])
    return out
