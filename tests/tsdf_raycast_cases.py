"""Cases of the TSDF volume's ray cast (tests/tsdf_raycast_ref.py), shared by tests/test_tsdf_raycast_api.py (CPU: the shared header
against the reference) and tests/test_gpu_tsdf_raycast.py (the kernel against it).  Every case is a volume of voxel words (and colour
words) that adc_tsdf_upload brings in, and a view.  The shapes are the smallest at which the kernel can go wrong: volumes 4 x 4 x 4,
8 x 12 x 16 and 64 x 48 x 128; views 1 x 1, 7 x 5, 37 x 23 (no multiple of the 8 x 8 pixels of a wave or the 16 x 16 of a workgroup:
partial waves and workgroups) and one 256 x 192.

case(name) -> dict(params, volume (tsdf, color), view); reference(name) -> the dict of tsdf_raycast_ref.raycast, computed once, read-only."""
import functools

import numpy as np

from tests import tsdf_cases as TC
from tests import tsdf_raycast_ref as RR
from tests import tsdf_ref as T

F = np.float32
MID = (8, 12, 16, 0.05, (-0.2, -0.3, 0.5), 0.15)          # x in [-0.2, 0.2], y in [-0.3, 0.3], z in [0.5, 1.3]
CONE_VOLUME = (64, 48, 128, 0.04, (-1.28, -0.96, 11.0), 0.16)  # (tests/test_gpu_tsdf.py)
# exact rotations whose principal ray runs along a world axis: the third row of R is that axis
LOOK_X = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0)
LOOK_Y = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
LOOK_BACK = (-1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0)  # half a turn about y: looks along -z


def pose(R, centre):
    """(R, t) of a camera with the world -> camera rotation R at the world position `centre`: t = -(R * centre)"""
    Rm = np.asarray(R, np.float64).reshape(3, 3)
    return tuple(R), tuple(float(v) for v in -(Rm @ np.asarray(centre, np.float64)))


def field_volume(p, distance, weight=4, colour_seed=None):
    """voxel words whose t is the rounded signed distance (metres, float64, positive on the free side) in units of trunc / 32767,
    every voxel of weight `weight` (an int or an array); colour words at random when the volume has them"""
    cx, cy, cz = (np.asarray(c, np.float64) for c in T.centres(p))
    d = distance(cx[None, None, :], cy[None, :, None], cz[:, None, None]) + np.zeros((p["nz"], p["ny"], p["nx"]))
    t = np.rint(np.clip(d / float(F(p["trunc"])), -1.0, 1.0) * T.Q).astype(np.int64)
    w = np.broadcast_to(np.asarray(weight, np.int64), t.shape)
    color = None
    if p["flags"] & T.COLOR:
        color = np.random.default_rng(colour_seed).integers(0, 2 ** 32, t.shape, dtype=np.uint32)
    return T.make_words(t, w), color


def plane(n, c):
    """signed distance to the plane n . X = c, positive where n . X < c"""
    n = np.asarray(n, np.float64)
    L = np.linalg.norm(n)
    return lambda x, y, z: (c - (n[0] * x + n[1] * y + n[2] * z)) / L


def sphere(centre, radius):
    return lambda x, y, z: np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius


def union(*fields):
    return lambda x, y, z: np.minimum.reduce([f(x, y, z) for f in fields])


TILTED = plane((-0.2, -0.1, 1.0), 0.9)  # z = 0.9 + 0.2 x + 0.1 y, free towards smaller z


def _mid(flags=0, trunc=0.15):
    return T.params(*MID[:5], trunc, flags=flags)


def _holes(words, seed, share, weights):
    rng = np.random.default_rng(seed)
    t = T.word_t(words)
    w = np.where(rng.random(words.shape) < share, rng.choice(np.asarray(weights), words.shape), T.word_w(words))
    return T.make_words(t, w)


def _build(name):
    V = RR.view
    if name in ("tiny_front", "tiny_1x1"):
        p = T.params(4, 4, 4, 0.1, (-0.2, -0.2, 0.4), 0.3)
        vol = field_volume(p, plane((0.0, 0.1, 1.0), 0.62))
        v = V(7, 5, 12.0, 3.0, 2.0, step=0.05) if name == "tiny_front" else V(1, 1, 10.0, 0.0, 0.0, step=0.05)
        return p, vol, v
    if name == "rotated":
        p = _mid(T.COLOR)
        R, t = pose(TC.rot(9.0, -14.0, 21.0), (0.12, -0.1, 0.1))
        return p, field_volume(p, TILTED, colour_seed=3), V(37, 23, 30.0, 18.2, 11.4, R, t)
    if name in ("look_x", "look_y", "look_z"):
        # the principal pixel (3, 2) has dx = dy = 0: a ray direction with two exactly zero components; the pixels of its row and
        # column have one.  Planes across the looked-along axis, in the LAST cell of that axis.
        p = _mid()
        if name == "look_x":
            vol, (R, t) = field_volume(p, plane((1.0, 0.02, 0.03), 0.177)), pose(LOOK_X, (-0.5, 0.0, 0.9))
        elif name == "look_y":
            vol, (R, t) = field_volume(p, plane((0.03, 1.0, 0.02), 0.268)), pose(LOOK_Y, (0.0, -0.7, 0.9))
        else:
            vol, (R, t) = field_volume(p, plane((0.02, 0.03, 1.0), 1.25)), pose(T.IDENTITY, (0.0, 0.0, 0.0))
        return p, vol, V(7, 5, 14.0, 3.0, 2.0, R, t)
    if name == "inside":
        p = _mid()
        R, t = pose(TC.rot(3.0, 4.0, 0.0), (0.01, 0.02, 0.62))
        return p, field_volume(p, TILTED), V(37, 23, 20.0, 18.0, 11.0, R, t)
    if name == "beside":
        p = _mid()
        R, t = pose(T.IDENTITY, (0.9, 0.0, 0.0))
        return p, field_volume(p, TILTED), V(7, 5, 30.0, 3.0, 2.0, R, t)
    if name == "past":  # behind the volume, looking away from it
        p = _mid()
        R, t = pose(T.IDENTITY, (0.0, 0.0, 1.5))
        return p, field_volume(p, TILTED), V(7, 5, 30.0, 3.0, 2.0, R, t)
    if name == "from_behind":  # the surface met from its back
        p = _mid()
        R, t = pose(LOOK_BACK, (0.02, 0.01, 1.8))
        return p, field_volume(p, TILTED), V(37, 23, 40.0, 18.0, 11.0, R, t)
    if name == "near_inside_far_short":  # z_near inside the volume; z_far in front of the surface for the upper rows
        p = _mid()
        return p, field_volume(p, TILTED), V(37, 23, 30.0, 18.0, 11.0, z_near=0.62, z_far=0.9)
    if name == "holes":  # (skip > voxel: a hit behind a free sample can land in a cell with an unseen corner)
        p = _mid(T.COLOR, trunc=0.1)
        tsdf, color = field_volume(p, TILTED, colour_seed=5)
        color = np.where(np.random.default_rng(6).random(color.shape) < 0.4, color & np.uint32(0x00FFFFFF), color)  # (cw = 0: no observed colour)
        return p, (_holes(tsdf, 7, 0.08, (0,)), color), V(37, 23, 30.0, 18.0, 11.0, skip=0.1)
    if name == "min_weight_3":
        p = _mid()
        tsdf, _ = field_volume(p, TILTED)
        return p, (_holes(tsdf, 8, 0.2, (0, 1, 2, 3, 5, 300)), None), V(37, 23, 30.0, 18.0, 11.0, min_weight=3)
    if name == "exhausted":
        p = _mid()
        return p, field_volume(p, TILTED), V(37, 23, 30.0, 18.0, 11.0, max_steps=5)
    if name in ("skip_eq_step", "skip_gt_step"):
        p = _mid(trunc=0.1)  # (most of the volume in front of the surface is saturated free space)
        return p, field_volume(p, TILTED), V(37, 23, 30.0, 18.0, 11.0, step=0.025, skip=0.025 if name == "skip_eq_step" else 0.05)
    if name == "t_zero":
        # dyadic geometry: the principal ray's samples fall on voxel centres exactly, and the plane z = 1.03125 goes through a layer
        # of centres, whose t is 0: f == 0 exactly at a sample
        p = T.params(8, 8, 16, 0.0625, (-0.25, -0.25, 0.5), 0.1875)
        vol = field_volume(p, plane((0.0, 0.0, 1.0), 1.03125))
        assert (T.word_t(vol[0]) == 0).sum() == 64
        return p, vol, V(7, 5, 16.0, 3.5, 2.5, pose(T.IDENTITY, (0.03125, 0.03125, 0.0))[0], pose(T.IDENTITY, (0.03125, 0.03125, 0.0))[1], z_near=0.53125, step=0.03125)
    if name == "t_min":  # a stored t of -32768 behind the surface
        p = _mid(trunc=0.1)
        tsdf, _ = field_volume(p, TILTED)
        tsdf = np.where(T.word_t(tsdf) == -T.Q, T.make_words(np.full(tsdf.shape, -32768), T.word_w(tsdf)), tsdf)
        R, t = pose(TC.rot(-4.0, 6.0, 2.0), (0.05, 0.0, 0.3))
        return p, (tsdf, None), V(37, 23, 30.0, 18.0, 11.0, R, t, step=0.06)
    if name in ("scene_37x23", "scene_256x192"):
        p = T.params(*CONE_VOLUME, flags=T.COLOR)
        scene = union(plane((0.1, -0.2, 1.0), 14.9), sphere((0.2, -0.1, 13.2), 0.55))
        tsdf, color = field_volume(p, scene, colour_seed=11)
        color = np.where(np.random.default_rng(12).random(color.shape) < 0.2, color & np.uint32(0x00FFFFFF), color)
        tsdf = _holes(tsdf, 13, 0.01, (0, 1))
        R, t = pose(TC.rot(2.0, -3.0, 1.0), (0.1, 0.05, 8.0))
        if name == "scene_37x23":
            return p, (tsdf, color), V(37, 23, 60.0, 18.0, 11.0, R, t, z_near=0.5, step=0.02, skip=0.08, min_weight=2)
        return p, (tsdf, color), V(256, 192, 420.0, 127.5, 95.5, R, t, z_near=0.5, step=0.02, skip=0.08)
    raise KeyError(name)


CASE_NAMES = ("tiny_front", "tiny_1x1", "rotated", "look_x", "look_y", "look_z", "inside", "beside", "past", "from_behind", "near_inside_far_short", "holes",
              "min_weight_3", "exhausted", "skip_eq_step", "skip_gt_step", "t_zero", "t_min", "scene_37x23", "scene_256x192")
# what each case must reach: statuses that occur (checked by the CPU test, so that a case cannot silently lose its branch)
REACHES = dict(tiny_front=("hit",), tiny_1x1=("hit",), rotated=("hit", "miss"), look_x=("hit",), look_y=("hit",), look_z=("hit",), inside=("hit",),
               beside=("miss",), past=("miss",), from_behind=("behind",), near_inside_far_short=("hit", "no_surface"), holes=("hit", "behind"),
               min_weight_3=("hit", "behind"), exhausted=("exhausted",), skip_eq_step=("hit",), skip_gt_step=("hit",), t_zero=("hit",), t_min=("hit",),
               scene_37x23=("hit", "behind"), scene_256x192=("hit", "behind"))


def _freeze(a):
    if a is not None:
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    p, vol, v = _build(name)
    return dict(params=p, volume=tuple(_freeze(None if a is None else np.ascontiguousarray(a, np.uint32)) for a in vol), view=v)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    r = RR.raycast(c["volume"], c["params"], c["view"])
    for k in ("depth", "normals", "bgr", "status", "samples"):
        _freeze(r[k])
    return r
