"""Checks of frame-to-model tracking that do not rest on the code under test: the scene is analytic (tests/tsdf_track_cases.py: planes of
a room corner), the true pose of the frame is known, and the measure is geometric -- the largest displacement of a visible scene point
between the recovered and the true pose: max over the frame's pixels with depth of |(Rr Pw + tr) - (Rt Pw + tt)|, Pw the scene point of
the pixel.  `track` is any implementation with the interface of tests/tsdf_track_ref.track (the numpy reference, the serial program,
the kernels).  profiles/tsdf_track_accuracy.md holds the measurements.

(a) check_analytic: analytic model maps at pose A, the frame rendered analytically at a known pose B, tracked from the guess A, with the
    frame's analytic normals (the angle gate keeps associations from crossing an edge of the corner).  Two motions, strides 1 and 2.
    MEASURED_Q is the final displacement measured on the numpy reference, in units of the residual quantum q = max_dist / 65536; the
    tests assert four times that (the float32 path against a float64 prototype that stayed within 4 q) and 1/100 of the initial one.
(b) check_chain: the analytic depth at A integrated three times by the reference integrator, ray cast from A by the reference ray
    caster as adc_tsdf_track casts it, the frame rendered analytically at B and tracked from the guess A.  Asserted: at most one
    voxel edge (the ray cast's own round-trip bound) and at most 1/10 of the initial displacement."""
import numpy as np

from tests import tsdf_raycast_ref as RR
from tests import tsdf_ref as T
from tests import tsdf_track_cases as KC
from tests import tsdf_track_ref as TR

F = np.float32
MOTIONS = ("small", "large")
TRUE_POSE = dict(small=KC.SMALL, large=KC.LARGE)  # about 1.6 degrees / 2.7 cm and 3.4 degrees / 7 cm from KC.A_POSE
MAX_DIST = dict(small=0.1, large=0.3)
# measured on tests/tsdf_track_ref.py (profiles/tsdf_track_accuracy.md), in units of q = max_dist / 65536
MEASURED_Q = {("small", 1): 0.146, ("small", 2): 0.229, ("large", 1): 0.112, ("large", 2): 0.0857}
# (b): a corner seen along its diagonal -- three mutually orthogonal planes through the apex (0, 0, 2.8), each met at about 55 degrees, so
# that the depth changes by about a third of a voxel from one pixel of the 256 x 192 frame to the next: the integrator reads the map
# at the nearest pixel, and on a surface whose depth steps by more than a voxel per pixel (the floor of the other scene at 64 x 48: 15 cm)
# the fused model is a staircase no tracker could align to better than that
APEX_Z = 2.8
DIAGONAL3 = tuple(((float(np.sqrt(2.0 / 3.0) * np.cos(a)), float(np.sqrt(2.0 / 3.0) * np.sin(a)), float(-1.0 / np.sqrt(3.0))), float(-APEX_Z / np.sqrt(3.0)))
                  for a in np.radians((90.0, 210.0, 330.0)))
CHAIN_SIZE = (256, 192)
CHAIN_VOLUME = (96, 76, 56, 0.04, (-1.9, -1.5, 0.8), 0.16)  # nx, ny, nz, voxel, origin, trunc: the corner as the two cameras see it


def displacement(c, R, t):
    """the largest displacement (metres) of a visible scene point between the pose (R, t) and the case's true pose"""
    focal, _, cx, cy, _ = c["frame"]["calib"]
    Rt, tt = (np.asarray(v, np.float64) for v in c["truth"])
    Rt = Rt.reshape(3, 3)
    Z, _ = KC.render(c["planes"], c["W"], c["H"], focal, cx, cy, *c["truth"])
    Z = Z.astype(np.float64)
    ys, xs = np.nonzero(Z > 0)
    Pc = np.stack([(xs - cx) / focal * Z[ys, xs], (ys - cy) / focal * Z[ys, xs], Z[ys, xs]], -1)
    Pw = (Pc - tt) @ Rt  # (R^T (Pc - t) per point, as rows)
    Pr = Pw @ np.asarray(R, np.float64).reshape(3, 3).T + np.asarray(t, np.float64)
    return float(np.sqrt(((Pr - Pc) ** 2).sum(-1)).max())


def _measure(c, r, **extra):
    q = float(F(c["params"]["max_dist"])) / 65536.0
    initial = displacement(c, c["frame"]["R"], c["frame"]["t"])
    final = displacement(c, r["R"], r["t"])
    return dict(status=TR.STATUS_NAMES[r["status"]], solves=r["solves"], used=r["counts"]["used"], initial=initial, final=final, final_q=final / q,
                ratio=final / initial, **extra)


def analytic_case(motion, stride):
    return KC.scene(64, 48, KC.A_POSE, TRUE_POSE[motion], with_normals=True, stride=stride, max_dist=MAX_DIST[motion], min_cos=0.9, iterations=10)


def check_analytic(track, motion, stride):
    c = analytic_case(motion, stride)
    r = track(c["map"], c["fnormals"], c["frame"], c["model"], c["mdepth"], c["mnormals"], c["params"])
    return _measure(c, r)


_chain = {}


def chain_case():
    """the case of (b), built once per process: the model maps come from the reference integrator and the reference ray caster"""
    if "case" not in _chain:
        W, H = CHAIN_SIZE
        c = dict(KC.scene(W, H, KC.A_POSE, KC.SMALL, planes=DIAGONAL3, iterations=10))
        focal, _, cx, cy, _ = c["frame"]["calib"]
        p = T.params(*CHAIN_VOLUME)
        at_a, _ = KC.render(c["planes"], W, H, focal, cx, cy, *KC.A_POSE)
        fr = T.frame(c["frame"]["calib"], *KC.A_POSE, kind=T.FROM_DEPTH)
        vol = T.empty(p)
        for _ in range(3):
            vol, _rep = T.integrate(vol, p, fr, at_a)
        voxel, trunc = F(p["voxel"]), F(p["trunc"])
        step = float(voxel * F(0.5))
        v = RR.view(W, H, focal, cx, cy, *KC.A_POSE, z_near=float(voxel), z_far=3.0e38, step=step, skip=max(float(trunc * F(0.5)), step), max_steps=16384)
        cast = RR.raycast(vol, p, v)
        c["model"] = TR.model(W, H, focal, cx, cy, *KC.A_POSE)
        c["mdepth"], c["mnormals"] = cast["depth"], cast["normals"]
        c["volume"], c["volume_params"], c["view"], c["depth_at_a"] = vol, p, v, at_a
        _chain["case"] = c
    return _chain["case"]


def check_chain(track):
    c = chain_case()
    r = track(c["map"], None, c["frame"], c["model"], c["mdepth"], c["mnormals"], c["params"])
    return _measure(c, r, voxel=float(F(c["volume_params"]["voxel"])), hits=int((c["mdepth"] > 0).sum()))
