"""Small named cases of frame-to-model tracking (tests/tsdf_track_ref.py, adcensus_amd/csrc/tsdf_track.h, k_tsdf_track.hip), each with
the counts it is there to reach and the status it ends with (REACHES).  The scene is analytic: three or four planes of a room corner
(the back wall z = 2.5, the right wall x = 1.0, the floor y = 0.8, in some cases the left wall x = -1.2), rendered from the geometry in
float64 and rounded to float32 -- depth as camera Z, normals in the camera frame pointing at the camera (negative z for a surface that
faces it: the convention of adc_normals and of the ray cast), fourth float 1.  Nothing here comes from the ray caster.

case(name) -> dict(W, H, map, fnormals or None, frame, model, mdepth, mnormals, params, truth or None); reference(name) -> the
dict of tsdf_track_ref.track, computed once per process and shared."""
import functools

import numpy as np

from tests import tsdf_cases as TC
from tests import tsdf_ref as T
from tests import tsdf_track_ref as TR

F = np.float32
CORNER3 = (((0.0, 0.0, -1.0), -2.5), ((-1.0, 0.0, 0.0), -1.0), ((0.0, -1.0, 0.0), -0.8))  # (n, d): the plane n . X = d, n towards the room
CORNER4 = CORNER3 + (((1.0, 0.0, 0.0), -1.2),)
IDENTITY = T.IDENTITY


def pose(R, centre):
    """(R, t) of a camera with the world -> camera rotation R at the world position `centre`: t = -(R * centre)"""
    Rm = np.asarray(R, np.float64).reshape(3, 3)
    return tuple(float(v) for v in R), tuple(float(F(v)) for v in -(Rm @ np.asarray(centre, np.float64)))


def intrinsics(W, H):
    """(focal, cx, cy) of a camera with a horizontal field of view of about 62 degrees"""
    return 0.83 * W, 0.5 * W - 0.5, 0.5 * H - 0.5


def render(planes, W, H, focal, cx, cy, R, t):
    """(depth float32 [H][W], normals float32 [H][W][4]) of the planes seen by the camera (R, t): the nearest plane in front of each
    pixel's ray; 0 / zeros where a ray meets none"""
    Rm = np.asarray(R, np.float64).reshape(3, 3)
    c = -(Rm.T @ np.asarray(t, np.float64))
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = np.stack([(xs - cx) / focal, (ys - cy) / focal, np.ones_like(xs)], -1) @ Rm  # (R^T d per pixel, as rows)
    best = np.full((H, W), np.inf)
    normal = np.zeros((H, W, 3))
    for n, d in planes:
        n = np.asarray(n, np.float64)
        den = dirs @ n
        with np.errstate(all="ignore"):
            z = (d - n @ c) / den
        hit = (den < 0) & (z > 0) & (z < best)  # (den < 0: the ray runs against the normal, the plane faces the camera)
        best = np.where(hit, z, best)
        normal = np.where(hit[..., None], Rm @ n, normal)
    seen = np.isfinite(best)
    depth = np.where(seen, best, 0.0).astype(F)
    normals = np.concatenate([normal, seen[..., None].astype(np.float64)], -1).astype(F)
    return depth, normals


def scene(W, H, guess_pose, true_pose, model_pose=None, model_size=None, planes=CORNER3, kind=T.FROM_DEPTH, with_normals=False, **kw):
    """the frame rendered at true_pose, tracked from guess_pose against the model rendered at model_pose (the guess when None)"""
    focal, cx, cy = intrinsics(W, H)
    calib = (focal, 0.16, cx, cy, 1.25)
    depth, fn = render(planes, W, H, focal, cx, cy, *true_pose)
    if kind == T.FROM_DISPARITY:
        with np.errstate(all="ignore"):
            depth = np.where(depth > 0, F(F(calib[0]) * F(calib[1])) / depth - F(calib[4]), F(np.nan)).astype(F)
    mw, mh = model_size or (W, H)
    mf, mcx, mcy = intrinsics(mw, mh) if model_size is None else (0.9 * mw, 0.48 * mw, 0.52 * mh)
    mR, mt = model_pose or guess_pose
    md, mn = render(planes, mw, mh, mf, mcx, mcy, mR, mt)
    return dict(W=W, H=H, map=depth, fnormals=fn if with_normals else None, frame=T.frame(calib, *guess_pose, kind=kind),
                model=TR.model(mw, mh, mf, mcx, mcy, mR, mt), mdepth=md, mnormals=mn, params=TR.params(**kw), truth=true_pose, planes=planes)


A_POSE = pose(TC.rot(2.0, -3.0, 1.0), (0.05, -0.03, 0.1))
SMALL = pose(TC.rot(2.9, -4.2, 1.5), (0.065, -0.045, 0.115))     # about 1.6 degrees / 2.7 cm from A_POSE
LARGE = pose(TC.rot(4.0, -5.6, 2.0), (0.09, -0.07, 0.15))        # about 3.4 degrees / 7 cm
OTHER = pose(TC.rot(-1.0, 2.0, -0.5), (-0.1, 0.05, -0.2))

REACHES = {
    "converged_64x48": ("used", "CONVERGED"),
    "tail_37x23": ("used", "CONVERGED"),
    "blocks_256x192": ("used", "CONVERGED"),
    "stride2": ("used", "CONVERGED"),
    "stride3": ("used", "CONVERGED"),
    "other_view": ("used", "outside", "CONVERGED"),
    "disparity": ("used", "CONVERGED"),
    "bad_values": ("no_depth", "used", "CONVERGED"),
    "model_holes": ("no_model", "used", "CONVERGED"),
    "far_gate": ("too_far", "used"),
    "angle_gate": ("angle", "used"),
    "outside": ("outside", "used"),
    "out_of_range": ("out_of_range",),
    "damped": ("used", "MAX_ITERATIONS"),
    "lost": ("no_depth", "LOST"),
    "degenerate": ("used", "DEGENERATE"),
    "diverged": ("used", "DIVERGED"),
    "max_iterations": ("used", "MAX_ITERATIONS"),
}
CASE_NAMES = tuple(REACHES)
SIZES = ((64, 48), (37, 23), (256, 192))  # the frame sizes of the cases: a handle per size


@functools.lru_cache(maxsize=None)
def case(name):
    eps = dict(eps_rot=1.0e-4, eps_trans=1.0e-4, iterations=12)
    if name == "converged_64x48":
        return scene(64, 48, A_POSE, SMALL, **eps)
    if name == "tail_37x23":  # a width that is no multiple of the wave: tail lanes
        return scene(37, 23, A_POSE, SMALL, **eps)
    if name == "blocks_256x192":  # 192 workgroups' worth of pixels
        return scene(256, 192, A_POSE, LARGE, planes=CORNER4, max_dist=0.3, **eps)
    if name == "stride2":
        return scene(64, 48, A_POSE, LARGE, stride=2, max_dist=0.3, **eps)
    if name == "stride3":  # (a stride that divides neither side)
        return scene(64, 48, A_POSE, SMALL, stride=3, **eps)
    if name == "other_view":  # the model seen by another camera: size, intrinsics and a pose that is not the guess
        return scene(64, 48, A_POSE, SMALL, model_pose=OTHER, model_size=(80, 60), **eps)
    if name == "disparity":
        return scene(64, 48, A_POSE, SMALL, kind=T.FROM_DISPARITY, **eps)
    if name == "bad_values":  # 0, NaN, +-inf and negative depths; a z_far that cuts the back wall's far pixels
        c = dict(scene(64, 48, A_POSE, SMALL, z_far=2.45, **eps))
        m = c["map"].copy()
        m[5, 3:9] = (0.0, np.nan, np.inf, -np.inf, -1.5, -0.0)
        m[20:23, 40:44] = np.nan
        c["map"] = m
        return c
    if name == "model_holes":  # model pixels without depth, and pixels with depth whose normal is zeros
        c = dict(scene(64, 48, A_POSE, SMALL, **eps))
        md, mn = c["mdepth"].copy(), c["mnormals"].copy()
        md[10:20, 10:30] = 0
        mn[30:40, 35:50] = 0
        md[0, 0], mn[1, 1, 3] = np.nan, np.nan
        c["mdepth"], c["mnormals"] = md, mn
        return c
    if name == "far_gate":  # 2.7 cm of motion and 1.6 degrees at 2.5 m against a gate of 2 cm
        return scene(64, 48, A_POSE, SMALL, max_dist=0.02, iterations=3)
    if name == "angle_gate":  # frame normals: where the association crosses an edge of the corner the normals disagree
        return scene(64, 48, A_POSE, LARGE, with_normals=True, min_cos=0.9, max_dist=0.3, iterations=3)
    if name == "outside":  # the model view is narrower than the frame
        return scene(64, 48, A_POSE, SMALL, model_pose=A_POSE, model_size=(40, 30), iterations=3)
    if name == "out_of_range":  # the model camera stands 9.5 m behind the scene's: |Pm x nm| reaches 4 * z_far on the walls and the floor
        return scene(64, 48, A_POSE, SMALL, model_pose=pose(IDENTITY, (0.0, 0.0, -9.5)), model_size=(320, 240), z_far=2.6, iterations=2)
    if name == "damped":
        return scene(64, 48, A_POSE, SMALL, damping=0.5, eps_rot=0.0, eps_trans=0.0, iterations=4)
    if name == "lost":  # no pixel has depth: LOST in the first solve, the pose is the guess
        c = dict(scene(64, 48, A_POSE, SMALL))
        c["map"] = np.zeros_like(c["map"])
        return c
    if name == "degenerate":  # one fronto-parallel plane: the columns of omega_z, v_x and v_y are exactly zero, and so is the third pivot
        ident = (IDENTITY, (0.0, 0.0, 0.0))
        return scene(64, 48, ident, (IDENTITY, (0.0, 0.0, 0.03)), planes=CORNER3[:1])
    if name == "diverged":
        return scene(64, 48, A_POSE, LARGE, max_dist=0.3, max_trans=1.0e-3)
    if name == "max_iterations":
        return scene(64, 48, A_POSE, LARGE, max_dist=0.3, iterations=2)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return TR.track(c["map"], c["fnormals"], c["frame"], c["model"], c["mdepth"], c["mnormals"], c["params"])
