"""Cases of the TSDF volume (tests/tsdf_ref.py), shared by tests/test_tsdf_api.py (CPU: the reference's properties, the shared
header against it) and tests/test_gpu_tsdf.py (the kernels against it).  The smallest shapes at which the kernels can still go
wrong: 8 x 8 x 8; 72 x 40 x 24 (a partial wave: rows that are no multiple of 64 lanes x 4 voxels); 260 x 12 x 8 (a row longer than
the 256 voxels of one wave: a partial second piece); 128 x 128 x 72 (4608 tiles of 256 voxels: the one-workgroup scan runs its second
turn of 4096), for extraction only.  Images of 48 x 36 and 80 x 60.

case(name) -> dict(params, size (W, H), frames [(frame, map, image or None)], init (tsdf, color) or None, min_weight); reference(name)
-> dict(volumes [after each frame], reports [per frame], points, xreport), computed once and read-only."""
import functools

import numpy as np

from tests import tsdf_ref as T

F = np.float32
INF = F(np.inf)
CALIB_80 = (60.0, 0.1, 39.5, 29.5, 0.0)     # focal_px, baseline, cx, cy, doffs
CALIB_80_DOFFS = (60.0, 0.1, 39.5, 29.5, 1.25)
CALIB_48 = (40.0, 0.1, 23.5, 17.5, 0.0)
TILE = 256          # voxels per tile of the extraction (k_tsdf.hip)
SCAN_TURN = 4096    # tiles per turn of its one-workgroup scan


def rot(ax_deg, ay_deg, az_deg=0.0):
    """R (float32, row-major 9) = Rz * Ry * Rx"""
    ax, ay, az = np.radians([ax_deg, ay_deg, az_deg])
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return tuple(float(v) for v in (rz @ ry @ rx).astype(F).ravel())


def image(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def plane_disparity(W, H, calib, Z):
    return np.full((H, W), F(F(calib[0]) * F(calib[1])) / F(Z) - F(calib[4]), F)


def tilted_disparity(W, H, d0, gx, gy):
    y, x = np.mgrid[0:H, 0:W]
    return (d0 + gx * (x - W / 2) + gy * (y - H / 2)).astype(F)


def raycast_depth(W, H, calib, R, t, surface):
    """Z (float32 [H][W], +inf = no depth) of an analytic world surface seen from the camera Xc = R * Xw + t; surface(o, d) -> ray
    parameter s (float64 [H][W], nan = miss) of the nearest hit of o + s * d (world)."""
    focal, _, cx, cy, _ = calib
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dc = np.stack([(x - cx) / focal, (y - cy) / focal, np.ones_like(x)], -1)  # Zc = s along these rays
    o = -R.T @ t
    d = dc @ R  # = R^T * dc per pixel
    s = surface(o, d)
    return np.where(np.isfinite(s) & (s > 0), s, np.inf).astype(F)


def plane_surface(n, c):
    n = np.asarray(n, np.float64)

    def hit(o, d):
        with np.errstate(all="ignore"):
            return (c - o @ n) / (d @ n)
    return hit


def sphere_surface(centre, radius):
    centre = np.asarray(centre, np.float64)

    def hit(o, d):
        oc = o - centre
        a, b, c = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - radius * radius
        with np.errstate(all="ignore"):
            return (-b - np.sqrt(b * b - 4 * a * c)) / (2 * a)
    return hit


ORIGIN_72 = (-0.72, -0.4, 0.6)
POSE_A = (rot(4.0, -9.0, 2.0), (0.05, -0.03, 0.04))
POSE_B = (rot(-6.0, 7.0, -3.0), (-0.06, 0.02, 0.02))


def _spoil(m):
    """+inf holes, a NaN, a -inf, and a block of negative disparities (their absolute value is taken)"""
    m = m.copy()
    H, W = m.shape
    m[H // 3:H // 3 + 6, W // 4:W // 4 + 9] = INF
    m[2, 3] = F(np.nan)
    m[H - 3, W - 5] = -INF
    m[H // 2:, W // 2:] *= F(-1)
    return m


def _build(name):
    P, FR = T.params, T.frame
    if name == "cube8_plane":
        p = P(8, 8, 8, 0.05, (-0.2, -0.2, 0.5), 0.12)
        return dict(params=p, size=(48, 36), frames=[(FR(CALIB_48), plane_disparity(48, 36, CALIB_48, 0.7), None)])
    if name == "plane5_saturates":
        p = P(72, 40, 24, 0.02, ORIGIN_72, 0.06, max_weight=3, flags=T.COLOR)
        m = plane_disparity(80, 60, CALIB_80, 0.84)
        return dict(params=p, size=(80, 60), frames=[(FR(CALIB_80), m, image(80, 60, 10 + i)) for i in range(5)])
    if name == "tilted_holes_two_poses":
        p = P(72, 40, 24, 0.02, ORIGIN_72, 0.06, flags=T.COLOR)
        m0 = _spoil(tilted_disparity(80, 60, 7.0 - 1.25, 0.012, -0.02))
        m1 = _spoil(tilted_disparity(80, 60, 7.3 - 1.25, -0.01, 0.015))
        return dict(params=p, size=(80, 60), frames=[(FR(CALIB_80_DOFFS, *POSE_A), m0, image(80, 60, 1)), (FR(CALIB_80_DOFFS, *POSE_B), m1, None)])
    if name == "long_row":
        p = P(260, 12, 8, 0.005, (-0.65, -0.03, 0.8), 0.02, flags=T.COLOR)
        return dict(params=p, size=(80, 60), frames=[(FR(CALIB_80, rot(0.0, 3.0), (0.0, 0.0, 0.0)), tilted_disparity(80, 60, 7.2, 0.01, 0.0), image(80, 60, 2))])
    if name == "depth_kind_cropped":
        p = P(72, 40, 24, 0.02, ORIGIN_72, 0.06, z_min=0.7, z_max=0.95)
        m = raycast_depth(80, 60, CALIB_80, T.IDENTITY, (0, 0, 0), plane_surface((0.2, -0.1, 1.0), 0.85))
        m[5:9, 10:20] = 0
        m[20:24, 30:44] = F(-0.8)
        m[40, 40] = F(np.nan)
        m[41:44, 50:60] = INF
        return dict(params=p, size=(80, 60), frames=[(FR(CALIB_80, kind=T.FROM_DEPTH), m, None)])
    if name == "behind_and_overflow":
        p = P(72, 40, 24, 0.02, ORIGIN_72, 0.06)
        m = plane_disparity(48, 36, CALIB_48, 0.1)
        m[10:20, 12:30] = F(1e-38)  # fb / s overflows: D = +inf, free space
        return dict(params=p, size=(48, 36), frames=[(FR(CALIB_48, T.IDENTITY, (0.0, 0.0, -0.8)), m, None)])
    if name == "wholly_outside":
        p = P(8, 8, 8, 0.05, (-0.2, -0.2, 0.5), 0.12, flags=T.COLOR)
        rng = np.random.default_rng(5)
        init = (rng.integers(0, 2 ** 32, (8, 8, 8), dtype=np.uint32), rng.integers(0, 2 ** 32, (8, 8, 8), dtype=np.uint32))
        m = plane_disparity(48, 36, CALIB_48, 0.7)
        return dict(params=p, size=(48, 36), init=init, frames=[(FR(CALIB_48, T.IDENTITY, (0.0, 0.0, -5.0)), m, image(48, 36, 3)),
                                                               (FR(CALIB_48, T.IDENTITY, (50.0, 0.0, 0.0)), m, None)])
    if name == "sphere_three_poses":
        p = P(72, 40, 24, 0.02, ORIGIN_72, 0.06, flags=T.COLOR)
        surf = sphere_surface((0.0, 0.0, 0.9), 0.17)
        poses = [(T.IDENTITY, (0.0, 0.0, 0.0)), POSE_A, POSE_B]
        return dict(params=p, size=(80, 60), frames=[(FR(CALIB_80, R, t, kind=T.FROM_DEPTH), raycast_depth(80, 60, CALIB_80, R, t, surf), image(80, 60, 20 + i))
                                                     for i, (R, t) in enumerate(poses)])
    if name == "uploaded_edges":
        # hand-made: t = 0, +-32767, a stored -32768, weights below min_weight, crossings on the last voxel of each axis
        p = P(8, 4, 4, 0.5, (1.0, 2.0, 3.0), 0.25, flags=T.COLOR)
        t = np.full((4, 4, 8), 32767, np.int64)
        w = np.full((4, 4, 8), 5, np.int64)
        t[:, :, 7] = -32767              # x crossings between i = 6 and the last voxel of every row
        t[:, 3, :4] = -100               # y crossings towards the last row, s = 32767 / 32867
        t[3, :2, 2:6] = -32768           # z crossings towards the last slab; read as -32767
        t[1, 1, 1] = 0                   # t = 0 counts as non-negative
        t[1, 1, 2] = -5
        t[2, 2, 3] = -7
        w[2, 2, 3] = 2                   # below min_weight 3: no crossing with it
        w[0, 0, 7] = 300                 # pad saturates at 255 only when both weights do
        w[0, 0, 6] = 400
        rng = np.random.default_rng(6)
        return dict(params=p, size=(48, 36), init=(T.make_words(t, w), rng.integers(0, 2 ** 32, (4, 4, 8), dtype=np.uint32)), frames=[], min_weight=3)
    if name == "saturating_weights":
        # uploaded state at the ends of both counters: w = 65534 / 65535 with max_weight 65535, cw = 254 / 255
        p = P(8, 8, 8, 0.05, (-0.2, -0.2, 0.5), 0.12, max_weight=65535, flags=T.COLOR)
        rng = np.random.default_rng(7)
        t = rng.integers(-32767, 32768, (8, 8, 8))
        w = rng.choice([0, 1, 65533, 65534, 65535], (8, 8, 8))
        col = rng.integers(0, 2 ** 24, (8, 8, 8), dtype=np.uint32) | (rng.choice([0, 253, 254, 255], (8, 8, 8)).astype(np.uint32) << np.uint32(24))
        m = plane_disparity(48, 36, CALIB_48, 0.7)
        return dict(params=p, size=(48, 36), init=(T.make_words(t, w), col), frames=[(FR(CALIB_48), m, image(48, 36, 30 + i)) for i in range(3)])
    if name == "big_scan":
        # a sphere's quantised distance written straight into 128 x 128 x 72 words: 4608 tiles, extraction only
        p = P(128, 128, 72, 0.01, (-0.64, -0.64, 0.5), 0.03)
        xw, yw, zw = T.centres(p)
        d = np.sqrt(xw[None, None, :].astype(np.float64) ** 2 + yw[None, :, None].astype(np.float64) ** 2 + (zw[:, None, None].astype(np.float64) - 0.86) ** 2) - 0.3
        t = np.rint(np.clip(d / 0.03, -1, 1) * T.Q).astype(np.int64)
        w = np.where(np.abs(d) < 0.2, 4, 1)
        return dict(params=p, size=(48, 36), init=(T.make_words(t, w), None), frames=[], min_weight=2)
    raise KeyError(name)


INTEGRATE_CASES = ("cube8_plane", "plane5_saturates", "tilted_holes_two_poses", "long_row", "depth_kind_cropped", "behind_and_overflow", "wholly_outside",
                   "sphere_three_poses", "saturating_weights")
CASE_NAMES = INTEGRATE_CASES + ("uploaded_edges", "big_scan")
CAPACITY_CASE = "sphere_three_poses"


def _freeze(a):
    if a is not None:
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    c = dict(init=None, min_weight=1)
    c.update(_build(name))
    for _, m, img in c["frames"]:
        _freeze(m)
        _freeze(img)
    if c["init"] is not None:
        c["init"] = tuple(_freeze(a) for a in c["init"])
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    vol = c["init"] if c["init"] is not None else T.empty(c["params"])
    volumes, reports = [], []
    for fr, m, img in c["frames"]:
        vol, rep = T.integrate(vol, c["params"], fr, m, img)
        volumes.append(tuple(_freeze(a) for a in vol))
        reports.append(rep)
    pts, xrep = T.extract(vol, c["params"], c["min_weight"])
    return dict(volumes=volumes, reports=reports, final=vol, points=_freeze(pts), xreport=xrep)


def capacities(points):
    """0, 1, around the first tile boundary of the record list that lies inside it, the exact count, above"""
    edge = min(TILE, max(points - 2, 2))
    return sorted({0, 1, edge - 1, edge, edge + 1, points - 1, points, points + 7})
