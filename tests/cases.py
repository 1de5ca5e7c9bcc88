"""Named, seeded test cases shared by the golden generator (tools/make_golden.py), the oracle tests
and the GPU parity tests.  A case = (left BGR, right BGR, option)."""
import os

import numpy as np

from adcensus_amd import workloads
from oracle import pyoracle

_HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(_HERE, "golden")


def cone_pair():
    z = np.load(os.path.join(GOLDEN_DIR, "cone_pair.npz"))
    return np.ascontiguousarray(z["left"]), np.ascontiguousarray(z["right"])


def data_pair(name):
    """cloth3 / piano / wood2: the other pairs of the reference's Data/ directory, committed as BGR arrays, one file per
    view so that each stays below 1 MiB (tests/golden/<name>_{left,right}.npz, written by tools/make_golden.py; PNG decode
    is lossless)."""
    left = np.load(os.path.join(GOLDEN_DIR, name + "_left.npz"))["left"]
    right = np.load(os.path.join(GOLDEN_DIR, name + "_right.npz"))["right"]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


DATA_RANGES = {"cloth3": 128, "piano": 64, "wood2": 128}  # Data/*/d_range.txt


def _crop(pair, y0, y1, x0, x1):
    return tuple(np.ascontiguousarray(a[y0:y1, x0:x1]) for a in pair)


def flat_patch_pair(width, height, disp_range, seed, patch_w=(80, 400), patch_h=(20, 80), band_h=(6, 40)):
    """Long-arm test pattern: flat colour patches (patch_w x patch_h pixels) with +-2 noise per view, so that cross arms run to the
    arm limit.  The right view shifts row bands (band_h rows) by different disparities, each band in two or three column pieces
    with disparities of their own: occlusions and mismatches, hence an active region-voting chain."""
    rng = np.random.default_rng(seed)
    cw = width + disp_range
    canvas = np.empty((height, cw, 3), np.int16)
    canvas[:] = rng.integers(0, 256, 3)
    for _ in range(max(4, 3 * (cw * height) // (patch_w[0] * patch_h[0]))):
        rw, rh = int(rng.integers(patch_w[0], patch_w[1] + 1)), int(rng.integers(patch_h[0], patch_h[1] + 1))
        x0, y0 = int(rng.integers(-rw // 2, cw)), int(rng.integers(-rh // 2, height))
        canvas[max(0, y0):max(0, y0 + rh), max(0, x0):max(0, x0 + rw)] = rng.integers(0, 256, 3)
    left = canvas[:, :width].copy()
    right = np.empty_like(left)
    y = 0
    while y < height:
        bh = int(rng.integers(band_h[0], band_h[1] + 1))
        cuts = sorted(int(c) for c in rng.integers(1, max(2, width), int(rng.integers(1, 3))))
        for xa, xb in zip([0] + cuts, cuts + [width]):
            d = int(rng.integers(0, max(1, disp_range)))
            right[y:y + bh, xa:xb] = canvas[y:y + bh, xa + d:xb + d]  # (right(x) = left(x + d))
        y += bh
    left = left + rng.integers(-2, 3, left.shape)
    right = right + rng.integers(-2, 3, right.shape)
    return tuple(np.ascontiguousarray(np.clip(a, 0, 255).astype(np.uint8)) for a in (left, right))


def flat_block_pair(width, height, block, shift, seed):
    """Uniform noise with ONE exactly flat block x block square at (8, 8); right view = left rolled by `shift` columns.  With arm
    limits of 255 a region of block x block pixels exceeds the reference's 16-bit support counts (cross_aggregator.h:101): 256 x 256
    wraps to a count of 0 (0 / 0 and x / 0 in the aggregation divide), larger squares wrap to small non-zero counts."""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
    left[8:8 + block, 8:8 + block] = rng.integers(0, 256, 3, dtype=np.uint8)
    return np.ascontiguousarray(left), np.ascontiguousarray(np.roll(left, shift, axis=1))


def slack_window_voting_input(width=256, height=1):
    """A region-voting input (LR-checked map, outlier labels, arms, horizontal support counts) built so that the changes that
    decide a vote lie past the 128 columns the voting slack count reads per row (k_voting.hip: irv_region_changes).  Per row:
    pixel 0 is a mismatch whose region reaches column 200 (right arm 200, arm limit >= 200); columns 1..10 are valid with
    disparity 3, the mismatches 128..200 fill with disparity 9 from the valid columns 201.. (their right arms reach the row's
    end).  Pixel 0 fails its first vote (10 pixels <= irv_ts = 20) with a budget of 10 changes; the 73 fills behind it then flip
    its next vote to 9 -- all of them outside the window [0, 128).  Returns (disp, label, arms, sup_h, option)."""
    disp = np.full((height, width), np.inf, np.float32)
    label = np.zeros((height, width), np.uint8)
    arms = np.zeros((height, width, 4), np.uint8)
    disp[:, 1:11] = 3.0
    disp[:, 201:] = 9.0
    label[:, 0] = 1
    label[:, 128:201] = 1
    arms[:, 0, 1] = 200
    arms[:, 128:201, 1] = np.arange(width - 1 - 128, width - 1 - 201, -1, dtype=np.int64).astype(np.uint8)
    sup_h = np.ascontiguousarray(arms[:, :, 0].astype(np.uint16) + arms[:, :, 1] + 1)
    opt = pyoracle.Option(max_disparity=16, cross_L1=255, cross_L2=255, irv_ts=20, irv_th=0.4)
    return disp, label, np.ascontiguousarray(arms), sup_h, opt


def region_voting_reference(disp, label, arms, opt):
    """The reference's iterative region voting (multistep_refiner.cpp:153-227) as plain loops: five iterations, mismatches then
    occlusions, each list in raster order, in place."""
    d = disp.copy()
    h, w = d.shape
    dmin, D = opt.min_disparity, opt.max_disparity - opt.min_disparity
    for _ in range(5):
        for which in (1, 2):
            for y, x in zip(*np.nonzero((label == which) & np.isinf(d))):
                hist = np.zeros(D, np.int64)
                for yt in range(y - int(arms[y, x, 2]), y + int(arms[y, x, 3]) + 1):
                    for xs in range(x - int(arms[yt, x, 0]), x + int(arms[yt, x, 1]) + 1):
                        if d[yt, xs] != np.inf:
                            hist[int(np.floor(d[yt, xs] + 0.5)) - dmin] += 1
                m, c = int(hist.max()), int(hist.sum())
                if m > 0 and c > opt.irv_ts and np.float32(m) / np.float32(c) > np.float32(opt.irv_th):
                    d[y, x] = float(int(np.argmax(hist)) + dmin)
    return d


def _long(l1, l2=None, d=32, **kw):
    return dict(max_disparity=d, cross_L1=l1, cross_L2=l1 if l2 is None else l2, **kw)


# name -> (builder returning (left,right), option kwargs)
_CASES = {
    # BASELINE.json configs[0]/[1]
    "cone": (cone_pair, dict(max_disparity=64)),
    "cone_neg": (cone_pair, dict(min_disparity=-16, max_disparity=48)),
    "cone_d16": (cone_pair, dict(max_disparity=16)),
    "cone_nolr": (cone_pair, dict(do_lr_check=0)),
    "cone_nofill": (cone_pair, dict(do_filling=0)),
    "cone_dda": (cone_pair, dict(do_discontinuity_adjustment=1)),
    "cone_params": (cone_pair, dict(lambda_ad=7, lambda_census=20, cross_L1=20, cross_L2=9, cross_t1=25, cross_t2=8,
                                    so_p1=0.8, so_p2=2.5, so_tso=11, irv_ts=12, irv_th=0.3, lrcheck_thres=1.5)),
    "cone_crop_d40": (lambda: _crop(cone_pair(), 100, 231, 120, 377), dict(max_disparity=40)),
    # cross_L1 = 40: the aggregation ring (81 entries) does not fit the register ring -> LDS full ring
    "cone_crop_L40": (lambda: _crop(cone_pair(), 100, 231, 120, 377), dict(max_disparity=40, cross_L1=40)),
    # small synthetic cases: odd sizes, W < D, census-skip sizes, 1-pixel-wide/high, VPL = 2 and 4
    "s2_96x64_d32": (lambda: workloads.structured_pair(96, 64, 32, seed=11), dict(max_disparity=32)),
    "s2_320x180_d128": (lambda: workloads.structured_pair(320, 180, 128, seed=12), dict(max_disparity=128)),
    "s2_200x120_d200": (lambda: workloads.structured_pair(200, 120, 200, seed=13), dict(max_disparity=200)),
    "q_257x131_d64": (lambda: workloads.quantized_noise_pair(257, 131, 64, seed=14), dict(max_disparity=64)),
    "q_20x40_d32": (lambda: workloads.quantized_noise_pair(20, 40, 32, seed=15), dict(max_disparity=32)),
    "q_9x20_d8": (lambda: workloads.quantized_noise_pair(9, 20, 8, seed=16), dict(max_disparity=8)),
    "q_30x7_d8": (lambda: workloads.quantized_noise_pair(30, 7, 8, seed=17), dict(max_disparity=8)),
    "q_1x40_d8": (lambda: workloads.quantized_noise_pair(1, 40, 8, seed=18), dict(max_disparity=8)),
    "q_40x1_d8": (lambda: workloads.quantized_noise_pair(40, 1, 8, seed=19), dict(max_disparity=8)),
    "q_3x3_d2": (lambda: workloads.quantized_noise_pair(3, 3, 2, seed=20), dict(max_disparity=2)),
    "noise_128x72_d64": (lambda: workloads.noise_pair(128, 72, seed=21), dict(max_disparity=64)),
    # short arms + D a multiple of 128: small aggregation ring with two disparities per lane, pass pairs (1 and 2 chunks)
    "noise_160x90_d128": (lambda: workloads.noise_pair(160, 90, seed=23), dict(max_disparity=128)),
    "noise_150x40_d256": (lambda: workloads.noise_pair(150, 40, seed=24), dict(max_disparity=256)),
    "s2_150x100_neg": (lambda: workloads.structured_pair(150, 100, 48, seed=22), dict(min_disparity=-8, max_disparity=40)),
    # min_disparity > 0: the right-view WTA, the fused-cost record padding and the scanline
    # interior test all have dmin-dependent branches.  (The reference reads out of bounds in the last min_disparity
    # columns of the right-view map, ADCensusStereo.cpp:296-300: those columns are excluded, see canonical().)
    "cone_pos": (cone_pair, dict(min_disparity=8, max_disparity=72)),
    "q_40x30_pos_wltd": (lambda: workloads.quantized_noise_pair(40, 30, 64, seed=25), dict(min_disparity=5, max_disparity=69)),
    "noise_160x90_d128_pos": (lambda: workloads.noise_pair(160, 90, seed=26), dict(min_disparity=3, max_disparity=131)),
    "s2_150x100_pos": (lambda: workloads.structured_pair(150, 100, 48, seed=27), dict(min_disparity=4, max_disparity=52)),
    # 128 < D < 192: four disparities per lane with a last 64-disparity chunk that is all padding
    "s2_200x120_d160": (lambda: workloads.structured_pair(200, 120, 160, seed=28), dict(max_disparity=160)),
    "noise_96x50_d160_neg": (lambda: workloads.noise_pair(96, 50, seed=29), dict(min_disparity=-70, max_disparity=90)),
    # disparity ranges above 256 (chunked voting histogram, 8 disparities per lane)
    "s2_360x60_d300": (lambda: workloads.structured_pair(360, 60, 300, seed=30), dict(max_disparity=300)),
    "noise_80x40_d520": (lambda: workloads.noise_pair(80, 40, seed=31), dict(min_disparity=-10, max_disparity=510)),
    # the largest range the product accepts (ADC_MAX_DISP_RANGE = 1024: 16 disparities per lane; the voting chain falls back
    # to 8 waves per workgroup because 16 histograms of 1024 bins do not fit into 64 KB of LDS)
    "s2_72x48_d1024": (lambda: workloads.structured_pair(72, 48, 40, seed=32), dict(min_disparity=-512, max_disparity=512)),
    # round 4: ranges above 1024 -- 32 disparities per lane, up to ADC_MAX_DISP_RANGE = 2047 (the 11-bit bins of the voting state map)
    "noise_64x24_d1100": (lambda: workloads.noise_pair(64, 24, seed=33), dict(min_disparity=-40, max_disparity=1060)),
    "s2_80x20_d2047": (lambda: workloads.structured_pair(80, 20, 48, seed=34), dict(min_disparity=-1000, max_disparity=1047)),
    # discontinuity adjustment with min_disparity != 0: the reference indexes the cost row with the ABSOLUTE
    # disparity (multistep_refiner.cpp:331-339), i.e. it reads the neighbouring pixel's costs
    "cone_crop_dda_neg": (lambda: _crop(cone_pair(), 100, 231, 120, 377), dict(min_disparity=-6, max_disparity=40, do_discontinuity_adjustment=1)),
    "cone_crop_dda_pos": (lambda: _crop(cone_pair(), 100, 231, 120, 377), dict(min_disparity=3, max_disparity=43, do_discontinuity_adjustment=1)),
    # the other Middlebury pairs of the reference's Data/ directory, ranges from Data/*/d_range.txt
    "cloth3": (lambda: data_pair("cloth3"), dict(max_disparity=128)),
    "piano": (lambda: data_pair("piano"), dict(max_disparity=64)),
    "wood2": (lambda: data_pair("wood2"), dict(max_disparity=128)),
    # long arm limits (cross_L1 up to the reference's MAX_ARM_LENGTH = 255) on flat patches, where the arms do reach the limit.
    # L1 = 48 / 49: the two sides of the voting slack count's 128-bit window ((xa & 31) + ml + mr + 1 <= 128, k_voting.hip)
    "flat_640x96_L48": (lambda: flat_patch_pair(640, 96, 32, seed=40), _long(48)),
    "flat_640x96_L49": (lambda: flat_patch_pair(640, 96, 32, seed=40), _long(49)),
    "flat_640x96_L64": (lambda: flat_patch_pair(640, 96, 32, seed=41), _long(64)),
    "flat_640x96_L128": (lambda: flat_patch_pair(640, 96, 32, seed=42), _long(128)),
    "flat_640x96_L255": (lambda: flat_patch_pair(640, 96, 32, seed=43), _long(255)),
    # the reference clamps the arm limit to 255: these equal flat_640x96_L255 stage for stage
    "flat_640x96_L300": (lambda: flat_patch_pair(640, 96, 32, seed=43), _long(300)),
    "flat_640x96_L1000": (lambda: flat_patch_pair(640, 96, 32, seed=43), _long(1000)),
    # vertical arms up to 255 too
    "flat_560x320_L255": (lambda: flat_patch_pair(560, 320, 24, seed=44, patch_h=(150, 320), band_h=(40, 120)), _long(255, d=24)),
    # odd arm options: L2 > L1, L2 = 0, t2 >= t1
    "flat_640x96_L64_L2gt": (lambda: flat_patch_pair(640, 96, 32, seed=45), _long(64, 200)),
    "flat_640x96_L128_L2zero": (lambda: flat_patch_pair(640, 96, 32, seed=46), _long(128, 0)),
    "flat_640x96_L128_t2t1": (lambda: flat_patch_pair(640, 96, 32, seed=47), _long(128, 60, cross_t1=12, cross_t2=15)),
    # odd shapes at L1 = 255: W < L, one row, one column
    "flat_200x64_L255": (lambda: flat_patch_pair(200, 64, 32, seed=48), _long(255)),
    "flat_600x1_L255": (lambda: flat_patch_pair(600, 1, 32, seed=49, patch_h=(1, 1), band_h=(1, 1)), _long(255)),
    "flat_1x300_L255": (lambda: flat_patch_pair(1, 300, 8, seed=50, patch_w=(1, 1), patch_h=(100, 300)), _long(255, d=8)),
    # 16-bit support counts wrap (cross_aggregator.h:101): a 256 x 256 flat block gives counts of 0 (NaN and inf in the
    # aggregated volume), a 300 x 300 block counts that wrapped to small non-zero values
    "wrap0_320x288_d16": (lambda: flat_block_pair(320, 288, 256, -4, seed=51), _long(255, d=16)),
    "wrap_320x320_d8": (lambda: flat_block_pair(320, 320, 300, -3, seed=52), _long(255, d=8)),
}

# ---- the option space (opt_<set>_<pair>[_r]) -------------------------------------------------------------------------------------
# Extreme and ordinary-but-untested values of the twelve numeric option fields, one field group per set, everything else default.
# The reference validates nothing but the disparity range, so every value here is a legal input; its behaviour on all of them is
# defined (a UBSAN build of its sources runs them clean, tests/test_sanitize.py) and the port restates it bit for bit.
# Deliberately NOT covered: lambda_ad <= 0 / lambda_census <= 0 (the reference divides by zero: sign and payload of the resulting
# NaN are nothing to pin bit for bit) and NaN thresholds.
# Pairs, all seeded and small: s2 = structured 96x64, q = quantized noise 70x45 (arms <= 1 under default options: the sets that
# need regions -- scanline threshold, voting -- do not use it), flat = flat patches 160x48 (arms that reach the limit), s2w =
# structured 160x48 with D = 128 (two disparities per lane: class offsets, fused cost windows and the fused tail are per-VPL
# code), n2w = uniform noise 160x48 with D = 128 (arms of 0..1: the only pair on which the last aggregation pass moves into the first
# scanline pass, k_scanline_seg_agg, which needs horizontal arms <= 3; 160 columns are the fewest that allow two row segments).
# s2x = structured 160x40 with D = 64 = the padded range: wide enough for whole interior chunks of the scanline kernels, whose class
# rule is a form of its own (adc_so_class_offsets_interior) -- the scanline threshold sets use it.
# "_r" = the range [-5, 27) with the discontinuity adjustment on.
OPT_PAIRS = {
    "s2": (lambda: workloads.structured_pair(96, 64, 32, seed=11), dict(max_disparity=32)),
    "q": (lambda: workloads.quantized_noise_pair(70, 45, 32, seed=5, levels=16), dict(max_disparity=32)),
    "flat": (lambda: flat_patch_pair(160, 48, 16, seed=3, patch_w=(20, 80), patch_h=(8, 30)), dict(max_disparity=32)),
    "s2w": (lambda: workloads.structured_pair(160, 48, 128, seed=61), dict(max_disparity=128)),
    "n2w": (lambda: workloads.noise_pair(160, 48, seed=71), dict(max_disparity=128)),
    "s2x": (lambda: workloads.structured_pair(160, 40, 64, seed=81), dict(max_disparity=64)),
    # flat patches of 6..30 x 4..12 pixels in bands of 3..10 rows: regions that mix several disparities (votes whose winning share
    # stays below the default irv_th) and arms that end between cross_L2 and cross_L1 on a colour step between cross_t2 and cross_t1
    "fs": (lambda: flat_patch_pair(160, 48, 16, seed=1, patch_w=(6, 30), patch_h=(4, 12), band_h=(3, 10)), dict(max_disparity=32)),
    "fs4": (lambda: flat_patch_pair(160, 48, 16, seed=4, patch_w=(6, 30), patch_h=(4, 12), band_h=(3, 10)), dict(max_disparity=32)),
}
_OPT_R = dict(min_disparity=-5, max_disparity=27, do_discontinuity_adjustment=1)
# family -> (stage a set of the family must change against the default options, pair tags it runs on)
OPT_FAMILIES = {
    "cost": ("cost_init", ["s2", "flat", "s2w", "n2w"]),
    "penalty": ("cost_so", ["s2", "flat", "s2w", "n2w", "s2_r"]),
    "tso": ("cost_so", ["s2", "flat", "s2w", "n2w", "s2x", "s2_r"]),
    "arm_t": ("arms", ["s2", "flat", "q"]),
    "arm_l": ("arms", ["s2", "flat", "q"]),
    "voting": ("disp_after_irv", ["s2", "flat", "flat_r"]),
    "lr": ("outlier_label", ["s2", "flat", "q"]),
}
# set -> (family, option fields[, pair tags of its own: where the family's pairs cannot show the set -- arms of at most 1 (q) never
# reach cross_L2, the colour steps of the large flat patches lie on one side of cross_t2, and no region of s2 / flat votes with
# a winning share below the default irv_th])
OPT_SETS = {
    "lam_1_1": ("cost", dict(lambda_ad=1, lambda_census=1)),
    "lam_2_200": ("cost", dict(lambda_ad=2, lambda_census=200)),
    "lam_255_3": ("cost", dict(lambda_ad=255, lambda_census=3)),
    "lam_1000_1000": ("cost", dict(lambda_ad=1000, lambda_census=1000)),
    "p_zero": ("penalty", dict(so_p1=0.0, so_p2=0.0)),
    "p1_gt_p2": ("penalty", dict(so_p1=3.0, so_p2=1.0)),
    "p_small": ("penalty", dict(so_p1=0.01, so_p2=0.03)),
    "p_big": ("penalty", dict(so_p1=100.0, so_p2=300.0)),
    "p_1e5": ("penalty", dict(so_p1=1e5, so_p2=3e5)),
    "p_neg": ("penalty", dict(so_p1=-1.0, so_p2=-3.0)),
    "tso_m3": ("tso", dict(so_tso=-3)),
    "tso_0": ("tso", dict(so_tso=0)),
    "tso_1": ("tso", dict(so_tso=1)),
    "tso_255": ("tso", dict(so_tso=255)),
    "tso_256": ("tso", dict(so_tso=256)),
    "tso_1000": ("tso", dict(so_tso=1000)),
    "t1_m4": ("arm_t", dict(cross_t1=-4)),
    "t1_0": ("arm_t", dict(cross_t1=0)),
    "t1_1": ("arm_t", dict(cross_t1=1)),
    "t1_255": ("arm_t", dict(cross_t1=255)),
    "t1t2_256": ("arm_t", dict(cross_t1=256, cross_t2=256)),
    "t2_0": ("arm_t", dict(cross_t2=0), ["s2", "flat", "fs"]),
    "t2_1000": ("arm_t", dict(cross_t2=1000), ["s2", "fs"]),
    "L1_m5": ("arm_l", dict(cross_L1=-5)),
    "L1_0": ("arm_l", dict(cross_L1=0)),
    "L1_2": ("arm_l", dict(cross_L1=2), ["s2", "flat", "fs"]),
    "L1_1_L2_0": ("arm_l", dict(cross_L1=1, cross_L2=0)),
    "L2_m3": ("arm_l", dict(cross_L2=-3), ["s2", "q", "fs"]),
    "L2_100000": ("arm_l", dict(cross_L2=100000), ["s2", "fs"]),
    "ts_m1": ("voting", dict(irv_ts=-1)),
    "ts_1": ("voting", dict(irv_ts=1)),
    "ts_100000": ("voting", dict(irv_ts=100000)),
    "th_m05": ("voting", dict(irv_th=-0.5), ["fs", "fs4", "fs4_r"]),
    "th_0": ("voting", dict(irv_th=0.0), ["fs", "fs4", "fs4_r"]),
    "th_099": ("voting", dict(irv_th=0.99)),
    "th_1": ("voting", dict(irv_th=1.0)),
    "th_5": ("voting", dict(irv_th=5.0)),
    "lr_m1": ("lr", dict(lrcheck_thres=-1.0)),
    "lr_0": ("lr", dict(lrcheck_thres=0.0)),
    "lr_03": ("lr", dict(lrcheck_thres=0.3)),
    "lr_1e9": ("lr", dict(lrcheck_thres=1e9)),
}
# sets that the reference makes equal by construction (every colour step is >= 0 > so_tso and <= 255 < so_tso; the arm limit is
# clamped to >= 0; no colour difference is < cross_t1 <= 0; a winning share is > 0 and <= 1): equal stage for stage, pair by pair
OPT_EQUAL_SETS = {"tso_m3": "tso_0", "tso_1000": "tso_256", "L1_m5": "L1_0", "t1_m4": "t1_0", "th_m05": "th_0", "th_5": "th_1"}


def _opt_case(pair_tag, fields):
    pair, _, r = pair_tag.partition("_")
    build, kw = OPT_PAIRS[pair]
    return build, dict(kw, **(_OPT_R if r else {}), **fields)


OPT_DEFAULTS = {}   # case name -> the case of the same pair and range under default options
OPT_TARGET = {}     # case name -> stage its set must change against OPT_DEFAULTS[name]
OPT_CASES = {fam: [] for fam in OPT_FAMILIES}  # family -> case names
_OPT_DEFAULT_TAGS = ("s2", "q", "flat", "s2w", "n2w", "s2x", "fs", "fs4", "s2_r", "flat_r", "fs4_r")
for _tag in _OPT_DEFAULT_TAGS:
    _CASES["opt_default_" + _tag] = _opt_case(_tag, {})
for _set, (_fam, _fields, *_own) in OPT_SETS.items():
    for _tag in (_own[0] if _own else OPT_FAMILIES[_fam][1]):
        _name = "opt_%s_%s" % (_set, _tag)
        _CASES[_name] = _opt_case(_tag, _fields)
        OPT_DEFAULTS[_name] = "opt_default_" + _tag
        OPT_TARGET[_name] = OPT_FAMILIES[_fam][0]
        OPT_CASES[_fam].append(_name)
OPT_DEFAULT_CASES = ["opt_default_" + t for t in _OPT_DEFAULT_TAGS]
OPT_ALL_CASES = [n for fam in OPT_FAMILIES for n in OPT_CASES[fam]]
# the penalty sets whose path costs need not converge within the scanline segments' 64-column warm-up (gpu_harness.stage_report)
OPT_SEAMS_MAY_FAIL = [n for n in OPT_CASES["penalty"] if n.startswith(("opt_p_big_", "opt_p_1e5_", "opt_p_neg_"))]
# ... and the one cost case that is the same thing from the other side: lambda = (1, 1) on uniform noise saturates the cost (44 % of the
# aggregated volume is exactly 2.0 and no pixel's costs spread by more than 1.0 = so_p1), so a path never takes the branch that
# forgets where it started -- whatever the warm-up length.  Its seams DO fail on the MI355X (profiles/README.md); the whole-row redo
# is exact.  (On the structured and flat pairs the same lambda leaves contrast, and the seams hold.)
OPT_SEAMS_MAY_FAIL.append("opt_lam_1_1_n2w")

GOLDEN_CASES = list(_CASES.keys())
# subset that the CPU-only tier recomputes with the port (kept small: the whole CPU suite must run in minutes)
FAST_CASES = ["cone_crop_d40", "s2_96x64_d32", "q_257x131_d64", "q_20x40_d32", "q_9x20_d8", "q_30x7_d8", "q_1x40_d8",
              "q_40x1_d8", "q_3x3_d2", "noise_128x72_d64", "s2_150x100_neg", "s2_200x120_d200", "noise_160x90_d128",
              "q_40x30_pos_wltd", "noise_160x90_d128_pos", "s2_150x100_pos", "s2_200x120_d160", "noise_96x50_d160_neg",
              "s2_360x60_d300", "noise_80x40_d520", "s2_72x48_d1024", "noise_64x24_d1100", "s2_80x20_d2047", "cone_crop_dda_neg", "cone_crop_dda_pos",
              # long arms (port: about a second each)
              "flat_640x96_L48", "flat_640x96_L49", "flat_640x96_L64", "flat_640x96_L128", "flat_640x96_L255", "flat_640x96_L1000",
              "flat_640x96_L64_L2gt", "flat_640x96_L128_L2zero", "flat_640x96_L128_t2t1", "flat_200x64_L255", "flat_600x1_L255",
              "flat_1x300_L255"]
FAST_CASES += OPT_DEFAULT_CASES + OPT_ALL_CASES  # (the option space: about 0.1 s each)
# named long-arm cases that the reference's arm clamp (MAX_ARM_LENGTH = 255) makes equal, stage for stage
CLAMPED_CASES = {"flat_640x96_L300": "flat_640x96_L255", "flat_640x96_L1000": "flat_640x96_L255"}


def canonical(stage, arr, opt):
    """The part of a stage dump that is defined behaviour of the reference: for min_disparity > 0 the right-view
    WTA map's last min_disparity columns come from an out-of-bounds read (ADCensusStereo.cpp:296-300 with
    best_disparity still 0) and are left out of hashes and comparisons.  (They are never consumed: the LR check
    reads column lround(x - d) <= W - 1 - min_disparity.)"""
    if stage == "disp_right_wta" and opt.min_disparity > 0:
        return np.ascontiguousarray(arr[:, :max(0, arr.shape[1] - opt.min_disparity)])
    return arr


def make_case(name):
    build, kw = _CASES[name]
    left, right = build()
    return left, right, pyoracle.Option(**kw)


def to_product_option(opt):
    """pyoracle.Option -> adcensus_amd.ADCensusOption (identical layout)."""
    import ctypes as C
    from adcensus_amd import ADCensusOption
    o = ADCensusOption()
    C.memmove(C.byref(o), C.byref(opt), C.sizeof(o))
    return o
