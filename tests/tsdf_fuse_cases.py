"""Cases of the stereo-aware TSDF fusion (tests/tsdf_fuse_ref.py), shared by tests/test_tsdf_fuse_api.py (CPU: the reference's
properties, the shared header against it) and tests/test_gpu_tsdf_fuse.py (the kernels against it).  The smallest shapes at which the
kernels can still go wrong: volumes of 16 x 5 x 7 (35 rows: no multiple of the 16 rows of a workgroup), 260 x 4 x 4 (a row longer than
the 256 voxels of one wave) and 64 x 48 x 40 (the chain's); maps of 37 x 23 (tail lanes, an unaligned row start) and 64 x 48.

fuse case(name) -> dict(params, size (W, H), init (tsdf, color) or None, frames [dict(frame, map, image, weight, wparams, prov, conf,
fp)]): a frame is fused with `weight` (uint8 [H][W]) when given, else with the weights of wparams / prov / conf when wparams is given,
else without a weight map.  reference(name) -> dict(volumes [after each frame], reports, wmaps [the weight map or None], wreports).
weight case(name) -> dict(size, frame, map, prov, conf, wparams); weight_reference(name) -> (weight, report).  Computed once, read-only."""
import functools

import numpy as np

from tests import tsdf_cases as TC
from tests import tsdf_fuse_ref as FR
from tests import tsdf_ref as T
from tests import tsdf_track_cases as KC

F = np.float32
INF = F(np.inf)
CALIB_37 = (30.0, 0.1, 18.0, 11.0, 0.0)       # focal_px, baseline, cx, cy, doffs: cx, cy whole numbers (fx == 0 / fy == 0 on the axis)
CALIB_37_DOFFS = (30.0, 0.1, 18.0, 11.0, 1.25)
CALIB_64 = (48.0, 0.1, 31.5, 23.5, 0.0)
SMALL_VOLUME = (16, 5, 7, 0.0625, (-0.46875, -0.15625, 0.55), 0.15)  # xw = 0 exactly at i = 7, yw = 0 at j = 2
GAP = F(2.0 ** -7)


def _frame(frame, m, image=None, weight=None, wparams=None, prov=None, conf=None, fp=None):
    return dict(frame=frame, map=m, image=image, weight=weight, wparams=wparams, prov=prov, conf=conf, fp=fp)


def ramp_depth(W, H):
    """0.6875 + x / 128: every value and every difference exact in binary32, so the spread of any 2 x 2 block is 2^-7 exactly"""
    return np.broadcast_to(F(0.6875) + np.arange(W, dtype=F) * GAP, (H, W)).astype(F)


def provenance(W, H, seed):
    """every fill class with every LR outcome, a quarter of the pixels with the speckle bit"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 16, (H, W)) | (rng.integers(0, 4, (H, W)) == 0) * FR.PROV_SPECKLE).astype(np.uint8)


def confidence(W, H, seed, pivot):
    """uniform in [0, 1) with a NaN, negatives, values above 1, +-inf and the pivot itself sprinkled in"""
    rng = np.random.default_rng(seed)
    c = rng.random((H, W)).astype(F)
    special = np.array([np.nan, -0.25, 1.5, pivot, np.inf, -np.inf, 0.0, 1.0, np.nextafter(F(pivot), F(0))], F)
    pick = rng.integers(0, 3 * len(special), (H, W))
    return np.where(pick < len(special), special[pick % len(special)], c).astype(F)


def _build(name):
    P, TF = T.params, T.frame
    if name == "plain_two_frames":
        # no weight map, no flag: adc_tsdf_integrate's own result
        p = P(*SMALL_VOLUME, flags=T.COLOR)
        m = TC._spoil(TC.tilted_disparity(37, 23, 4.0, 0.02, -0.03))
        return dict(params=p, size=(37, 23), frames=[_frame(TF(CALIB_37), m, TC.image(37, 23, 1)), _frame(TF(CALIB_37, *TC.POSE_A), m)])
    if name == "mixed_weights":
        # 0 / 1 / 255 and a few others, three frames into max_weight 300: the cap is met on the way
        p = P(*SMALL_VOLUME, max_weight=300, flags=T.COLOR)
        rng = np.random.default_rng(11)
        frames = []
        for i in range(3):
            w = rng.choice(np.array([0, 1, 255, 2, 17, 128], np.uint8), (23, 37), p=(0.25, 0.25, 0.25, 0.1, 0.1, 0.05))
            frames.append(_frame(TF(CALIB_37), TC.tilted_disparity(37, 23, 4.0 + 0.2 * i, 0.02, -0.03), TC.image(37, 23, 20 + i), weight=w))
        return dict(params=p, size=(37, 23), frames=frames)
    if name == "all_ones":
        c = dict(_build("plain_two_frames"))
        c["frames"] = [dict(f, weight=np.ones((23, 37), np.uint8)) for f in c["frames"]]
        return c
    if name == "numerator_64bit":
        # w = 65535, t = +-32767 uploaded, wo = 255, max_weight 65535: q = 32767 in free space in front of a far plane reaches the
        # largest numerator, 65534 * 65535 + 65534 * 255 + 32895; a near plane gives the other values of q
        p = P(*SMALL_VOLUME, max_weight=65535)
        rng = np.random.default_rng(12)
        t = rng.choice([32767, -32767, 0, 12345], (7, 5, 16), p=(0.7, 0.1, 0.1, 0.1))
        w = rng.choice([65535, 65534, 65281, 0], (7, 5, 16), p=(0.7, 0.1, 0.1, 0.1))
        m = np.full((23, 37), F(3.0), F)
        m[:, 18:] = F(0.8)
        return dict(params=p, size=(37, 23), init=(T.make_words(t, w), None),
                    frames=[_frame(TF(CALIB_37, kind=T.FROM_DEPTH), m, weight=np.full((23, 37), 255, np.uint8)) for _ in range(2)])
    if name == "gap_edges":
        # the spread of the four taps is 2^-7 everywhere: frame 0 with interp_gap = 2^-7 interpolates, frame 1 with the float below it
        # (the spread is one ulp above the gap) does not; fx == 0 on the column xw = 0, fy == 0 on the row yw = 0
        p = P(*SMALL_VOLUME)
        fr = TF(CALIB_37, kind=T.FROM_DEPTH)
        m = ramp_depth(37, 23)
        return dict(params=p, size=(37, 23), frames=[_frame(fr, m, fp=FR.fuse_params(FR.FUSE_BILINEAR, float(GAP))),
                                                     _frame(fr, m, fp=FR.fuse_params(FR.FUSE_BILINEAR, float(np.nextafter(GAP, F(0)))))])
    if name == "disparity_specials":
        # disparity kind: +inf holes, a NaN (one invalid tap among four around it), a -inf, a block of negative values (valid; across its
        # border the raw values differ by about 8 and the gap refuses them), zeros (without doffs: no depth; with doffs: valid)
        p = P(*SMALL_VOLUME, flags=T.COLOR)
        m = TC._spoil(TC.tilted_disparity(37, 23, 4.0, 0.02, -0.03))
        m[15:18, 5:9] = F(0.0)
        w = FR.weight_params(depth_power=2, z_ref=0.7)
        fp = FR.fuse_params(FR.FUSE_BILINEAR, 0.5)
        return dict(params=p, size=(37, 23), frames=[_frame(TF(CALIB_37), m, TC.image(37, 23, 3), wparams=w, fp=fp),
                                                     _frame(TF(CALIB_37_DOFFS, *TC.POSE_A), (m + F(0.3)).astype(F), TC.image(37, 23, 4), wparams=w, fp=fp)])
    if name == "long_row":
        # a row longer than the 256 voxels of one wave, wider than the 64 x 48 view: x0 = W - 1 and voxels outside; colour
        p = P(260, 4, 4, 0.005, (-0.65, -0.01, 0.8), 0.02, flags=T.COLOR)
        m = TC.tilted_disparity(64, 48, 5.8, 0.01, 0.0)
        prov, conf = provenance(64, 48, 5), confidence(64, 48, 6, 0.25)
        w = FR.weight_params((16, 4, 1, 0), 0.25, FR.W_SCALE_CONFIDENCE, 4, 0.8)
        return dict(params=p, size=(64, 48), frames=[_frame(TF(CALIB_64, TC.rot(0.0, 3.0), (0.0, 0.0, 0.0)), m, TC.image(64, 48, 2), wparams=w, prov=prov, conf=conf,
                                                            fp=FR.fuse_params(FR.FUSE_BILINEAR, 0.05))])
    if name == "corner_wide":
        # the chain's volume around a room corner seen by the small camera: the volume is wider and taller than the view (x0 = W - 1
        # and y0 = H - 1 fall back to the nearest pixel), depth kind, z4 weights, the edges of the corner gated by 0.2 m
        p = P(64, 48, 40, 0.04, (-1.28, -0.96, 1.0), 0.16, flags=T.COLOR)
        focal, cx, cy = KC.intrinsics(37, 23)
        calib = (focal, 0.16, cx, cy, 0.0)
        frames = []
        for i, ps in enumerate((KC.A_POSE, KC.SMALL)):
            d, _ = KC.render(KC.CORNER3, 37, 23, focal, cx, cy, *ps)
            frames.append(_frame(TF(calib, *ps, kind=T.FROM_DEPTH), d, TC.image(37, 23, 30 + i), wparams=FR.weight_params((16, 4, 1, 0), 0.0, 0, 4, 1.5),
                                 fp=FR.fuse_params(FR.FUSE_BILINEAR, 0.2)))
        return dict(params=p, size=(37, 23), frames=frames)
    raise KeyError(name)


CASE_NAMES = ("plain_two_frames", "all_ones", "mixed_weights", "numerator_64bit", "gap_edges", "disparity_specials", "long_row", "corner_wide")
IDENTITY_CASES = ("plain_two_frames", "all_ones")  # equal to adc_tsdf_integrate


def _build_weight(name):
    TF = T.frame
    m37 = TC._spoil(TC.tilted_disparity(37, 23, 4.0, 0.05, -0.03))
    m37[15:18, 5:9] = F(0.0)
    m37[19, 20:30] = F(5e-39)  # fb / s = 3 / 5e-39 overflows: D = +inf
    base = dict(size=(37, 23), frame=TF(CALIB_37), map=m37, prov=provenance(37, 23, 1), conf=confidence(37, 23, 2, 0.375))
    if name == "defaults_map_only":
        return dict(base, prov=None, conf=None, wparams=None)
    if name == "fills_and_speckle":
        return dict(base, conf=None, wparams=FR.weight_params((200, 90, 30, 7), depth_power=0))
    if name == "confidence_threshold":
        return dict(base, prov=None, wparams=FR.weight_params((255, 0, 0, 0), 0.375, 0, 2, 0.6))
    if name == "confidence_scaled":
        return dict(base, wparams=FR.weight_params((16, 4, 1, 0), 0.375, FR.W_SCALE_CONFIDENCE, 4, 0.75))
    if name == "power0_scaled_doffs":
        return dict(base, frame=TF(CALIB_37_DOFFS), wparams=FR.weight_params((255, 128, 64, 1), 0.0, FR.W_SCALE_CONFIDENCE, 0, 1.0))
    if name == "depth_kind_64":
        focal, cx, cy = KC.intrinsics(64, 48)
        d, _ = KC.render(KC.CORNER3, 64, 48, focal, cx, cy, *KC.A_POSE)
        d = d.copy()
        d[3, 4:9] = (0.0, np.nan, np.inf, -1.0, 1e-30)
        return dict(size=(64, 48), frame=TF((focal, 0.16, cx, cy, 0.0), kind=T.FROM_DEPTH), map=d, prov=provenance(64, 48, 3), conf=confidence(64, 48, 4, 0.5),
                    wparams=FR.weight_params((16, 4, 1, 0), 0.5, 0, 4, 1.5))
    raise KeyError(name)


WEIGHT_CASE_NAMES = ("defaults_map_only", "fills_and_speckle", "confidence_threshold", "confidence_scaled", "power0_scaled_doffs", "depth_kind_64")


def _freeze(a):
    if a is not None:
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    c = dict(init=None)
    c.update(_build(name))
    for f in c["frames"]:
        for k in ("map", "image", "weight", "prov", "conf"):
            _freeze(f[k])
    if c["init"] is not None:
        c["init"] = tuple(_freeze(a) for a in c["init"])
    return c


@functools.lru_cache(maxsize=None)
def weight_case(name):
    c = _build_weight(name)
    for k in ("map", "prov", "conf"):
        _freeze(c[k])
    return c


@functools.lru_cache(maxsize=None)
def weight_reference(name):
    c = weight_case(name)
    w, rep = FR.weights(c["map"], c["frame"], c["wparams"], c["prov"], c["conf"])
    return _freeze(w), rep


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    vol = c["init"] if c["init"] is not None else T.empty(c["params"])
    volumes, reports, wmaps, wreports = [], [], [], []
    for f in c["frames"]:
        w, wrep = f["weight"], None
        if w is None and f["wparams"] is not None:
            w, wrep = FR.weights(f["map"], f["frame"], f["wparams"], f["prov"], f["conf"])
        vol, rep = FR.fuse(vol, c["params"], f["frame"], f["map"], f["image"], w, f["fp"])
        volumes.append(tuple(_freeze(a) for a in vol))
        reports.append(rep)
        wmaps.append(_freeze(w))
        wreports.append(wrep)
    return dict(volumes=volumes, reports=reports, final=vol, wmaps=wmaps, wreports=wreports)
