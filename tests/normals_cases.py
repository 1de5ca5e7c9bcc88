"""Maps, calibrations, parameters and the case list shared by the CPU and GPU tiers of the surface-normal tests
(tests/test_normals_api.py, tests/test_gpu_normals.py).  The reference result of a case is computed once (functools.lru_cache) and
never modified."""
import functools

import numpy as np

from tests import normals_ref as N

F = np.float32
G0 = 2.0 ** -12  # a max_diff whose gate G is 0: only taps with the centre's own fixed-point disparity


def calib_for(W, H, doffs=0.0):
    """(focal_px, baseline, cx, cy, doffs): fractional principal point (no pixel sits on the axis)"""
    return (800.0, 0.16, float(F(W / 2 - 0.3)), float(F(H / 2 + 0.2)), float(doffs))


def slanted(W, H, d0=20.0, gx=0.3, gy=0.1, noise=0.0, seed=3):
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = d0 + gx * x + gy * y
    if noise:
        d = d + np.random.default_rng(seed).uniform(-noise, noise, (H, W))
    return d.astype(F)


def mixed_map():
    """67 x 35: a slanted plane, a step of 40 px at x = 40, two constant patches (22 px: behind doffs = -25, so s <= 0; 60 px), a
    spike no gate reaches, a usable pixel alone in a block of NaN, holes of +inf, NaN, -inf, values >= 32768, a region of negative
    disparities."""
    W, H = 67, 35
    d = slanted(W, H, noise=0.02)
    d[:, 40:] += F(40)
    d[2:18, 2:18] = F(22)
    d[18:34, 2:18] = F(60)
    d[25, 30] = F(500)
    d[20:27, 55:62] = np.nan
    d[23, 58] = F(75.5)
    for k, v in enumerate([np.inf, np.nan, -np.inf, 32768.0, 40000.0, 1e30, -np.inf, 3e38]):
        d[3 + 2 * k, 45 + (5 * k) % 9] = F(v)
    d[0:11, 58:66] *= F(-1)
    return np.ascontiguousarray(d)


def tiles_map():
    """131 x 70: crosses tile edges in both directions whatever tile up to 128 x 64 a kernel chooses; a plane with noise, a step, holes
    on and next to the 64 / 128 column and the 16 / 32 / 64 row boundaries."""
    W, H = 131, 70
    d = slanted(W, H, d0=30.0, gx=0.11, gy=-0.07, noise=0.05, seed=5)
    d[40:, 70:] += F(6)
    for y, x in ((15, 63), (16, 64), (31, 127), (32, 128), (63, 64), (64, 63), (69, 130), (0, 0), (47, 100)):
        d[y, x] = np.inf
    d[63:66, 126:130] = np.nan
    return np.ascontiguousarray(d)


def _small(W, H):
    return slanted(W, H, d0=10.0, gx=0.25, gy=-0.15, noise=0.01, seed=W * 100 + H)


# (name, map builder, doffs, radius, max_diff, min_points)
CASES = [
    ("one_1x1", lambda: _small(1, 1), 0.0, 1, 1.0, 3),
    ("two_2x2", lambda: _small(2, 2), 0.0, 1, 64.0, 3),  # (4 taps at most, r = 1: n >= 3 but never a full window; the fit exists)
    ("two_2x2_full", lambda: _small(2, 2), 0.0, 1, 64.0, 9),
    ("row_1x40", lambda: _small(40, 1), 0.0, 3, 64.0, 3),
    ("column_40x1", lambda: _small(1, 40), 0.0, 3, 64.0, 3),
    ("window_9x7_r7", lambda: _small(9, 7), 0.0, 7, 64.0, 3),
    ("window_9x7_r7_full", lambda: _small(9, 7), 0.0, 7, 64.0, 225),
    ("mixed_r1_g0", mixed_map, -25.0, 1, G0, 3),
    ("mixed_r1_full", mixed_map, -25.0, 1, 1.0, 9),
    ("mixed_r3", mixed_map, -25.0, 3, 1.0, 3),
    ("mixed_r3_gmax_full", mixed_map, -25.0, 3, 64.0, 49),
    ("mixed_r7_gmax", mixed_map, -25.0, 7, 64.0, 3),
    ("mixed_r7_g0", mixed_map, -25.0, 7, G0, 3),
    ("mixed_r7_full", mixed_map, -25.0, 7, 4.0, 225),
    ("mixed_default", mixed_map, 1.25, 2, 1.0, 5),
    ("tiles_default", tiles_map, 0.0, 2, 1.0, 5),
    ("tiles_r7", tiles_map, 0.0, 7, 2.0, 3),
]
CASE_NAMES = [c[0] for c in CASES]
# the cases named for all three classes: asserted on the reference's own counts, otherwise the tests show nothing
MIXED_ALL_CLASSES = ["mixed_r1_g0", "mixed_r3", "mixed_r7_gmax", "mixed_r7_g0", "mixed_r1_full", "mixed_r3_gmax_full", "mixed_r7_full"]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(map, calib, radius, max_diff, min_points, size) of a named case."""
    _, build, doffs, radius, max_diff, min_points = CASES[CASE_NAMES.index(name)]
    m = build()
    m.setflags(write=False)
    H, W = m.shape
    return dict(map=m, calib=calib_for(W, H, doffs), radius=radius, max_diff=max_diff, min_points=min_points, size=(W, H))


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    out, out8, rep = N.normals(c["map"], c["calib"], c["radius"], c["max_diff"], c["min_points"])
    out.setflags(write=False)
    out8.setflags(write=False)
    return out, out8, rep


assert (N.gate(G0), N.gate(64.0)) == (0, 65536)
for _name in MIXED_ALL_CLASSES:
    _rep = reference(_name)[2]
    assert _rep["fitted"] > 0 and _rep["few_points"] > 0 and _rep["degenerate"] > 0, (_name, _rep)
