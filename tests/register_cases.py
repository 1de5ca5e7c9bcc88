"""Scenes, target cameras and the case list shared by the CPU and GPU tiers of the registration tests (tests/test_register_api.py,
tests/test_gpu_register.py).  The reference result of a case is computed once (functools.lru_cache) and never modified."""
import functools
import math

import numpy as np

import adcensus_amd as A
from tests import register_ref as R

F = np.float32
SPECIALS = [np.inf, np.nan, -np.inf, 0.0, -3.5, 1e-40, 3e38]  # +inf, NaN, -inf, 0, a negative, a denormal, 3e38


def calib_for(W, H):
    """(focal_px, baseline, cx, cy, doffs): fractional principal point (no pixel sits on the axis), Middlebury-like doffs."""
    return (float(F(0.8 * max(W, H))), 0.16, float(F(W / 2 - 0.3)), float(F(H / 2 + 0.2)), 1.25)


def scene(W, H, kind, seed=1, specials=True):
    """float32 [H][W]: two planes (the lower / right half is the second) with small noise, a nearer constant rectangle (equal values:
    equal depths), and the special values at positions spread over the raster.  kind decides the unit: disparities around 20..50 px, or
    the depths such disparities stand for."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    d = (F(20) + F(0.01) * x + F(0.005) * y).astype(F)
    second = (y >= H // 2) if H > 1 else (x >= W // 2)
    d = np.where(second, F(30) + F(0.004) * x + F(0.02) * y, d).astype(F)
    d = (d + rng.uniform(-0.05, 0.05, (H, W)).astype(F)).astype(F)
    y0, y1, x0, x1 = H // 4, max(H // 4 + 1, (3 * H) // 5), W // 3, max(W // 3 + 1, (2 * W) // 3)
    d[y0:y1, x0:x1] = F(50)
    if kind == R.FROM_DEPTH:
        focal, baseline, _, _, doffs = calib_for(W, H)
        d = (F(focal * baseline) / (d + F(doffs))).astype(F)
    flat = d.reshape(-1)
    for k, v in enumerate(SPECIALS if specials else []):
        flat[((2 * k + 1) * flat.size) // (2 * len(SPECIALS))] = F(v)
    return np.ascontiguousarray(d)


def rot(ax_deg, ay_deg):
    ax, ay = math.radians(ax_deg), math.radians(ay_deg)
    rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    return (ry @ rx).astype(F).ravel()


def target(name, W, H, Wt, Ht):
    """The target sets of the tests; intrinsics follow the target's size so that the scene lands inside it."""
    focal, baseline, cx, cy, _ = calib_for(W, H)
    sx, sy = Wt / W, Ht / H
    base = dict(width=Wt, height=Ht, fx=focal * sx, fy=focal * sy, cx=cx * sx, cy=cy * sy)
    if name == "identity":  # (same size: the source's own camera)
        return A.RegTarget(**base)
    if name == "shift":  # a camera beside the left one: parallax of 1.5 baselines, along the longer axis of the image
        return A.RegTarget(t=[-1.5 * baseline, 0, 0] if W >= H else [0, -1.5 * baseline, 0], **base)
    if name == "rot5":  # turned by 5 degrees, moved, strongly distorted
        return A.RegTarget(R=rot(1.0, 5.0), t=[0.05, -0.02, 0.01], k1=-0.28, k2=0.09, p1=0.001, p2=-0.0007, k3=0.01, **base)
    if name == "behind":  # turned by 180 degrees: everything is behind the camera
        return A.RegTarget(R=[-1, 0, 0, 0, 1, 0, 0, 0, -1], **base)
    if name == "huge":  # a huge focal length: everything is out of range
        return A.RegTarget(**dict(base, fx=1e9, fy=1e9))
    if name == "tiny":  # every pixel lands within a hundredth of a pixel of (1, 1): ties
        return A.RegTarget(**dict(base, fx=0.01, fy=0.01, cx=1.0, cy=1.0))
    if name == "cap":  # 12 target pixels per source pixel: every footprint is cut at ADC_REG_MAX_SPLAT
        return A.RegTarget(**dict(base, fx=12 * focal * sx, fy=12 * focal * sy))
    raise KeyError(name)


# (name, source W x H, input kind, target set, target W x H)
CASES = [
    ("identity_depth", (333, 77), R.FROM_DEPTH, "identity", (333, 77)),
    ("identity_disp", (333, 77), R.FROM_DISPARITY, "identity", (333, 77)),
    ("shift_collide", (333, 77), R.FROM_DEPTH, "shift", (333, 77)),
    ("rot5_small", (333, 77), R.FROM_DISPARITY, "rot5", (160, 96)),
    ("rot5_2x", (333, 77), R.FROM_DEPTH, "rot5", (666, 154)),
    ("behind", (333, 77), R.FROM_DISPARITY, "behind", (333, 77)),
    ("huge", (333, 77), R.FROM_DEPTH, "huge", (333, 77)),
    ("tiny_3x3", (333, 77), R.FROM_DISPARITY, "tiny", (3, 3)),
    ("tiny_plain_3x3", (333, 77), R.FROM_DEPTH, "tiny", (3, 3)),  # (no special values: the nearest surface is the constant rectangle)
    ("cap", (333, 77), R.FROM_DEPTH, "cap", (333, 77)),
    ("shift_1x1", (333, 77), R.FROM_DISPARITY, "shift", (1, 1)),
    ("row_shift", (4099, 1), R.FROM_DISPARITY, "shift", (4099, 1)),
    ("row_widest", (4099, 1), R.FROM_DEPTH, "identity", (32767, 1)),
    ("column_shift", (1, 2053), R.FROM_DISPARITY, "shift", (1, 2053)),
    ("column_1x1", (1, 2053), R.FROM_DEPTH, "rot5", (1, 1)),
    ("three_rows_2x", (1025, 3), R.FROM_DISPARITY, "shift", (2050, 6)),
    ("three_rows_small", (1025, 3), R.FROM_DEPTH, "identity", (160, 96)),
    ("kitti_shift", (1242, 375), R.FROM_DISPARITY, "shift", (1242, 375)),
    ("kitti_rot5_2x", (1242, 375), R.FROM_DEPTH, "rot5", (2484, 750)),
]
CASE_NAMES = [c[0] for c in CASES]
# (case, splat) whose candidates exceed the filled pixels / where equal depths meet on a target pixel: asserted on the reference's own
# counts.  A target smaller than the source collides without splat only: with it a footprint narrower than a pixel is mostly empty.
COLLISION_CASES = [("shift_collide", True), ("kitti_shift", True), ("three_rows_small", False), ("tiny_3x3", False)]
TIE_CASES = [("tiny_plain_3x3", False), ("three_rows_small", False)]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(map, kind, calib, target, tbgr) of a named case."""
    _, (W, H), kind, tname, (Wt, Ht) = CASES[CASE_NAMES.index(name)]
    m = scene(W, H, kind, specials="plain" not in name)
    m.setflags(write=False)
    rng = np.random.default_rng(7)
    tbgr = rng.integers(1, 256, (Ht, Wt, 3), dtype=np.uint8)  # (no zero byte: a copied colour is told from "nothing")
    tbgr.setflags(write=False)
    return dict(map=m, kind=kind, calib=calib_for(W, H), target=target(tname, W, H, Wt, Ht), tbgr=tbgr, size=(W, H), tsize=(Wt, Ht))


@functools.lru_cache(maxsize=None)
def reference(name, splat=True):
    c = case(name)
    depth, index, rep = R.register(c["map"], c["kind"], c["calib"], c["target"], splat)
    depth.setflags(write=False)
    index.setflags(write=False)
    return depth, index, rep


@functools.lru_cache(maxsize=None)
def reference_align(name):
    c = case(name)
    out, valid = R.align(c["map"], c["kind"], c["calib"], c["target"], c["tbgr"])
    out.setflags(write=False)
    valid.setflags(write=False)
    return out, valid
