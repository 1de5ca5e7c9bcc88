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
