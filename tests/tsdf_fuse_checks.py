"""Checks of the stereo-aware fusion that do not rest on the code under test: the scenes are analytic (tests/tsdf_track_cases.py: the
planes of a room corner), the truth is known, and only the integrator is exchanged -- `fuse` and `weights` are any implementation with
the interfaces of tests/tsdf_fuse_ref.fuse / .weights (the numpy reference, the kernels); the ray caster and the tracker are the numpy
references.  profiles/tsdf_fuse_accuracy.md holds the measurements.

(a) check_staircase: the scene the chain of tests/tsdf_track_checks.py could not use -- the axis-aligned corner at 64 x 48, whose floor
    steps by more than a voxel of depth per pixel.  Three frames at A into STAIR_VOLUME, ray cast as adc_tsdf_track casts, the frame
    rendered at SMALL tracked from the guess A with default parameters.  With nearest sampling the chain's criterion (at most one
    voxel edge and at most 1/10 of the initial displacement) FAILS; with the gated bilinear sampling (interp_gap 0.2 m) it holds.
(b) check_noise: the corner at 160 x 120 as a disparity map with Gaussian noise (sigma 0.25 px, default_rng(5)), two frames at A and
    six from 1.5 m further back; the ray cast of the fused volume from A against the analytic depth, rms over the pixels that hit.
    Asserted: rms(z4 weights, bilinear) / rms(uniform, nearest) <= NOISE_BOUND = 1.5 * NOISE_MEASURED_RATIO, the ratio measured on the
    numpy reference: the seed is fixed, so the margin only covers rounding choices of the rule, and it stays below 0.75."""
import numpy as np

from tests import tsdf_fuse_ref as FR
from tests import tsdf_raycast_ref as RR
from tests import tsdf_ref as T
from tests import tsdf_track_cases as KC
from tests import tsdf_track_checks as KK
from tests import tsdf_track_ref as TR

F = np.float32
STAIR_SIZE = (64, 48)
STAIR_VOLUME = (72, 56, 72, 0.04, (-1.7, -1.3, 0.0), 0.16)
STAIR_GAP = 0.2
NOISE_SIZE = (160, 120)
NOISE_VOLUME = (96, 76, 80, 0.04, (-2.6, -2.0, -0.5), 0.16)
NOISE_SIGMA, NOISE_SEED, NOISE_BACK = 0.25, 5, 1.5
NOISE_WEIGHTS = FR.weight_params((16, 4, 1, 0), 0.0, 0, 4, 1.5)
NOISE_GAP = 2.0  # disparities: eight sigma, the corner has creases and no depth discontinuity
NOISE_MEASURED_RATIO = 0.3434  # 0.017327 m / 0.050452 m, measured on tests/tsdf_fuse_ref.py (profiles/tsdf_fuse_accuracy.md)
NOISE_BOUND = 1.5 * NOISE_MEASURED_RATIO
assert NOISE_BOUND < 0.75


def _cast(vol, p, W, H, focal, cx, cy, pose):
    voxel, trunc = F(p["voxel"]), F(p["trunc"])
    step = float(voxel * F(0.5))
    v = RR.view(W, H, focal, cx, cy, *pose, z_near=float(voxel), z_far=3.0e38, step=step, skip=max(float(trunc * F(0.5)), step), max_steps=16384)
    return RR.raycast(vol, p, v)


def check_staircase(fuse, bilinear):
    W, H = STAIR_SIZE
    c = dict(KC.scene(W, H, KC.A_POSE, KC.SMALL))
    focal, _, cx, cy, _ = c["frame"]["calib"]
    p = T.params(*STAIR_VOLUME)
    at_a, _ = KC.render(c["planes"], W, H, focal, cx, cy, *KC.A_POSE)
    fr = T.frame(c["frame"]["calib"], *KC.A_POSE, kind=T.FROM_DEPTH)
    fp = FR.fuse_params(FR.FUSE_BILINEAR if bilinear else 0, STAIR_GAP if bilinear else 0.0)
    vol = T.empty(p)
    for _ in range(3):
        vol, rep = fuse(vol, p, fr, at_a, None, None, fp)
    cast = _cast(vol, p, W, H, focal, cx, cy, KC.A_POSE)
    c["model"] = TR.model(W, H, focal, cx, cy, *KC.A_POSE)
    r = TR.track(c["map"], None, c["frame"], c["model"], cast["depth"], cast["normals"], c["params"])
    initial = KK.displacement(c, c["frame"]["R"], c["frame"]["t"])
    final = KK.displacement(c, r["R"], r["t"])
    return dict(status=TR.STATUS_NAMES[r["status"]], solves=r["solves"], initial=initial, final=final, ratio=final / initial, voxel=float(F(p["voxel"])),
                interpolated=rep["interpolated"], updated=rep["updated"])


def chain_criterion(m):
    """the bounds of tests/tsdf_track_checks.check_chain's test"""
    return m["final"] <= m["voxel"] and m["final"] <= 0.1 * m["initial"]


_noise = {}


def noise_frames():
    """[(frame, noisy disparity map)] and the analytic depth at A, built once per process"""
    if "frames" not in _noise:
        W, H = NOISE_SIZE
        focal, cx, cy = KC.intrinsics(W, H)
        calib = (focal, 0.16, cx, cy, 0.0)
        rng = np.random.default_rng(NOISE_SEED)
        Ra, ta = KC.A_POSE
        back = (Ra, tuple(float(F(v)) for v in np.asarray(ta, np.float64) + np.array([0.0, 0.0, NOISE_BACK])))  # the camera NOISE_BACK further back along its axis
        frames = []
        for ps in (KC.A_POSE,) * 2 + (back,) * 6:
            z, _ = KC.render(KC.CORNER3, W, H, focal, cx, cy, *ps)
            with np.errstate(all="ignore"):
                d = np.where(z > 0, F(F(focal) * F(0.16)) / z, F(np.nan)).astype(np.float64)
            d = (d + rng.normal(0.0, NOISE_SIGMA, d.shape)).astype(F)
            d.setflags(write=False)
            frames.append((T.frame(calib, *ps, kind=T.FROM_DISPARITY), d))
        truth, _ = KC.render(KC.CORNER3, W, H, focal, cx, cy, *KC.A_POSE)
        _noise["frames"], _noise["truth"], _noise["intrinsics"] = frames, truth, (focal, cx, cy)
    return _noise["frames"], _noise["truth"], _noise["intrinsics"]


def noise_rms(fuse, weights, weighted, bilinear):
    """rms depth error (metres) of the ray cast of the fused volume against the analytic depth, and the number of pixels it is over"""
    frames, truth, (focal, cx, cy) = noise_frames()
    W, H = NOISE_SIZE
    p = T.params(*NOISE_VOLUME, max_weight=1024)
    fp = FR.fuse_params(FR.FUSE_BILINEAR if bilinear else 0, NOISE_GAP if bilinear else 0.0)
    vol = T.empty(p)
    for fr, d in frames:
        w = weights(d, fr, NOISE_WEIGHTS, None, None)[0] if weighted else None
        vol, _ = fuse(vol, p, fr, d, None, w, fp)
    cast = _cast(vol, p, W, H, focal, cx, cy, KC.A_POSE)
    hit = (cast["depth"] > 0) & (truth > 0)
    err = cast["depth"][hit].astype(np.float64) - truth[hit].astype(np.float64)
    return float(np.sqrt((err * err).mean())), int(hit.sum())


def check_noise(fuse, weights):
    base, n0 = noise_rms(fuse, weights, False, False)
    best, n1 = noise_rms(fuse, weights, True, True)
    return dict(uniform_nearest=base, z4_bilinear=best, ratio=best / base, pixels=(n0, n1))
