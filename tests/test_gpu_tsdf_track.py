"""GPU tier of frame-to-model tracking (adcensus_amd/csrc/k_tsdf_track.hip): the two kernels against tests/tsdf_track_ref.py bit for bit
on every case of tests/tsdf_track_cases.py -- the whole adc_track_result as raw bytes, from adc_get_track_result and from a poisoned
device buffer whose tail must stay poisoned, the input maps unchanged; a ray cast then a track with no wait between them; two tracks
back to back; a track with a Match behind it and one wait; a track refused while a Match is pending; the host entry point with a
larger frame after a smaller one; the accuracy checks of tests/tsdf_track_checks.py once on the kernels."""
import ctypes as C

import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases
from tests import tsdf_raycast_ref as RR
from tests import tsdf_track_cases as KC
from tests import tsdf_track_checks as K
from tests import tsdf_track_ref as TR
from tests.test_gpu_outputs import POISON, DeviceBuffers, _handle
from tests.test_tsdf_api import c_frame, c_params
from tests.test_tsdf_raycast_api import c_view
from tests.test_tsdf_track_api import c_model, c_track_params, cli_track_reference, result_dict

pytestmark = pytest.mark.gpu

F = np.float32
TAIL = 64  # poisoned bytes behind the result record
RESULT_BYTES = 960
OPT = pyoracle.Option(max_disparity=16)


class Inputs:
    """the four maps of a case on the device; unchanged() reads them back"""

    def __init__(self, dev, c):
        self.dev, self.host = dev, {k: None if c[k] is None else np.ascontiguousarray(c[k], F) for k in ("map", "fnormals", "mdepth", "mnormals")}
        self.ptr = {k: None if a is None else dev.new(a) for k, a in self.host.items()}

    def unchanged(self):
        return all(a is None or self.dev.get(self.ptr[k], a.shape, F).tobytes() == a.tobytes() for k, a in self.host.items())


def _enqueue(A, st, dev, c, inp, with_result=True):
    d_res = dev.alloc(RESULT_BYTES + TAIL, POISON) if with_result else None
    ok = st.track_device(inp.ptr["map"], c_frame(c["frame"]), c_model(c["model"]), inp.ptr["mdepth"], inp.ptr["mnormals"], c_track_params(c["params"]),
                         inp.ptr["fnormals"], d_res)
    assert ok, A.last_error()
    return d_res


def _check(what, st, dev, d_res, want):
    res = st.track_result()
    assert res is not None
    got, ref = bytes(res), TR.result_bytes(want)
    if got != ref:  # name the first field that differs
        g = result_dict(res)
        for k in ("status", "solves", "counts", "iteration", "H", "b", "R", "t"):
            assert g[k] == want[k], (what, k, g[k], want[k])
    assert got == ref, what
    if d_res is not None:
        raw = dev.get(d_res, RESULT_BYTES + TAIL, np.uint8)
        assert (raw[RESULT_BYTES:] == POISON).all(), "%s: written behind the record" % what
        assert raw[:RESULT_BYTES].tobytes() == ref, "%s: the device copy of the record differs" % what


@pytest.mark.parametrize("name", KC.CASE_NAMES)
def test_kernels_equal_the_reference(hip, name):
    A = hip
    c, want = KC.case(name), KC.reference(name)
    st, dev = _handle(A, c["W"], c["H"], OPT), DeviceBuffers(A)
    try:
        assert st.track_result() is None
        inp = Inputs(dev, c)
        d_res = _enqueue(A, st, dev, c, inp)
        assert st.wait(), A.last_error()
        _check(name, st, dev, d_res, want)
        assert inp.unchanged(), name
    finally:
        dev.free()
        st.Release()


def test_two_tracks_back_to_back_and_refusals_on_a_real_handle(hip):
    """two tracks enqueued with no wait between them: the result is the last one's, the first one's device record is its own; refused
    calls enqueue nothing and keep the result"""
    A = hip
    a, b = KC.case("converged_64x48"), KC.case("stride2")
    st, dev = _handle(A, 64, 48, OPT), DeviceBuffers(A)
    try:
        ia, ib = Inputs(dev, a), Inputs(dev, b)
        ra = _enqueue(A, st, dev, a, ia)
        rb = _enqueue(A, st, dev, b, ib)
        assert st.wait(), A.last_error()
        _check("the second of two", st, dev, rb, KC.reference("stride2"))
        assert dev.get(ra, RESULT_BYTES, np.uint8).tobytes() == TR.result_bytes(KC.reference("converged_64x48"))
        before = bytes(st.track_result())
        bad = dict(a["params"], iterations=33)
        pp = dev.alloc(RESULT_BYTES + TAIL, POISON)
        fr, mv, tp = c_frame(a["frame"]), c_model(a["model"]), c_track_params(a["params"])
        for call, why in ((lambda: st.track_device(ia.ptr["map"], fr, mv, ia.ptr["mdepth"], ia.ptr["mnormals"], c_track_params(bad), None, pp), "iterations"),
                          (lambda: st.track_device(ia.ptr["map"] + 2, fr, mv, ia.ptr["mdepth"], ia.ptr["mnormals"], tp, None, pp), "4-byte aligned"),
                          (lambda: st.track_device(ia.ptr["map"], fr, mv, ia.ptr["mdepth"], ia.ptr["mnormals"] + 8, tp, None, pp), "16-byte aligned"),
                          (lambda: st.track_device(ia.ptr["map"], fr, mv, ia.ptr["mdepth"], ia.ptr["mnormals"], tp, None, pp + 4), "8-byte aligned"),
                          (lambda: st.track_device(ia.ptr["map"], fr, None, ia.ptr["mdepth"], ia.ptr["mnormals"], tp, None, pp), "null model view")):
            assert not call() and why in A.last_error(), (why, A.last_error())
        assert st.wait() and bytes(st.track_result()) == before and (dev.get(pp, RESULT_BYTES + TAIL, np.uint8) == POISON).all()
        with pytest.raises(RuntimeError):  # (the host entry point needs a volume)
            st.tsdf_track(a["map"], fr)
        assert "no volume" in A.last_error()
    finally:
        dev.free()
        st.Release()


def test_a_match_behind_a_pending_track(hip, oracle):
    """adc_track_device and adc_match_device enqueued back to back with ONE adc_wait: the record and the Match's map are exact -- the
    record lies in pinned memory of its own, where no Match writes.  While the Match is pending a track is refused."""
    A = hip
    w, h = 160, 96
    left, right = workloads.structured_pair(w, h, 32, seed=5)
    opt = pyoracle.Option(max_disparity=32)
    want_d = oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    c = KC.scene(w, h, KC.A_POSE, KC.SMALL, eps_rot=1.0e-4, eps_trans=1.0e-4, iterations=8)
    want = TR.track(c["map"], None, c["frame"], c["model"], c["mdepth"], c["mnormals"], c["params"])
    assert want["status"] == TR.CONVERGED and want["solves"] < 8  # (surplus launches behind the terminal status)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * w * h, POISON)
        inp = Inputs(dev, c)
        d_res = _enqueue(A, st, dev, c, inp)
        assert st.match_device(dl, dr, dd), A.last_error()
        assert not st.track_device(inp.ptr["map"], c_frame(c["frame"]), c_model(c["model"]), inp.ptr["mdepth"], inp.ptr["mnormals"]) and "Match is pending" in A.last_error()
        assert st.wait(), A.last_error()
        _check("behind a match", st, dev, d_res, want)
        assert np.array_equal(dev.get(dd, (h, w), F).view(np.uint32), np.ascontiguousarray(want_d).view(np.uint32))
    finally:
        dev.free()
        st.Release()


def test_ray_cast_then_track_with_no_wait_and_the_whole_chain_on_the_kernels(hip):
    """tests/tsdf_track_checks.py (b) on the device: the analytic depth integrated three times at pose A by adc_tsdf_integrate_device,
    ray cast from A and tracked -- five calls enqueued with no wait between them, one adc_wait.  The kernels of the integrator and the
    ray caster equal their references bit for bit, so the record equals the reference chain's; the displacement is asserted as on the
    CPU: at most one voxel edge and 1/10 of the initial one."""
    A = hip
    c = K.chain_case()
    want = TR.track(c["map"], None, c["frame"], c["model"], c["mdepth"], c["mnormals"], c["params"])
    W, H = K.CHAIN_SIZE
    st, dev = _handle(A, W, H, OPT), DeviceBuffers(A)
    try:
        assert st.tsdf_create(c_params(c["volume_params"])), A.last_error()
        d_at_a, d_map = dev.new(np.ascontiguousarray(c["depth_at_a"], F)), dev.new(np.ascontiguousarray(c["map"], F))
        d_depth, d_normals = dev.alloc(4 * W * H + TAIL, POISON), dev.alloc(16 * W * H + TAIL, POISON)
        d_res = dev.alloc(RESULT_BYTES + TAIL, POISON)
        fr_a = c_frame(dict(c["frame"], R=KC.A_POSE[0], t=KC.A_POSE[1]))
        for _ in range(3):
            assert st.tsdf_integrate_device(d_at_a, fr_a), A.last_error()
        view = c_view(c["view"])
        assert st.tsdf_raycast_device(view, d_depth, d_normals), A.last_error()
        assert st.track_device(d_map, c_frame(c["frame"]), view, d_depth, d_normals, c_track_params(c["params"]), None, d_res), A.last_error()
        assert st.wait(), A.last_error()
        assert dev.get(d_depth, (H, W), F).tobytes() == c["mdepth"].tobytes() and dev.get(d_normals, (H, W, 4), F).tobytes() == c["mnormals"].tobytes()
        _check("chain", st, dev, d_res, want)
        m = K._measure(c, result_dict(st.track_result()), voxel=float(F(c["volume_params"]["voxel"])))
        print("chain on the kernels:", m)
        assert m["final"] <= m["voxel"] and m["final"] <= m["initial"] / 10.0, m
    finally:
        dev.free()
        st.Release()


def test_host_entry_point_with_a_larger_frame_after_a_smaller_one(hip):
    """adc_tsdf_track at 64 x 48 and then at 256 x 192 (a handle has one geometry, so each size has its handle and its scratch is
    allocated by its first call), each against the reference chain -- the reference ray cast of the handle's own view from the guess,
    then the reference tracker --, twice per handle; then with NULL parameters."""
    A = hip
    big = K.chain_case()
    p, vol = big["volume_params"], big["volume"]
    for W, H in ((64, 48), K.CHAIN_SIZE):
        c = big if (W, H) == K.CHAIN_SIZE else KC.scene(W, H, KC.A_POSE, KC.SMALL, planes=K.DIAGONAL3, iterations=10)
        focal, _, cx, cy, _ = c["frame"]["calib"]
        v = dict(big["view"], width=W, height=H, focal_px=focal, cx=cx, cy=cy)
        cast = RR.raycast(vol, p, v)
        want = TR.track(c["map"], None, c["frame"], TR.model(W, H, focal, cx, cy, *KC.A_POSE), cast["depth"], cast["normals"], c["params"])
        st = _handle(A, W, H, OPT)
        try:
            assert st.tsdf_create(c_params(p)), A.last_error()
            st.tsdf_upload(*vol)
            for _ in range(2):
                res = st.tsdf_track(c["map"], c_frame(c["frame"]), c_track_params(c["params"]))
                assert bytes(res) == TR.result_bytes(want) == bytes(st.track_result()), (W, H)
            d = st.tsdf_track(c["map"], c_frame(c["frame"]))  # (NULL parameters: the defaults)
            assert 1 <= d.solves <= 10 and d.pixels == W * H and C.sizeof(d) == RESULT_BYTES
            assert st.tsdf_raycast_report().rays == W * H
        finally:
            st.Release()


@pytest.mark.parametrize("motion,stride", (("small", 2), ("large", 1)))
def test_analytic_scene_on_the_kernels(hip, motion, stride):
    """tests/tsdf_track_checks.py (a) once per motion on the kernels: four times the displacement measured on the reference, and 1/100
    of the initial one"""
    A = hip

    def track(depth_map, fnormals, fr, mdl, mdepth, mnormals, p):
        H, W = depth_map.shape
        c = dict(W=W, H=H, map=depth_map, fnormals=fnormals, frame=fr, model=mdl, mdepth=mdepth, mnormals=mnormals, params=p)
        st, dev = _handle(A, W, H, OPT), DeviceBuffers(A)
        try:
            _enqueue(A, st, dev, c, Inputs(dev, c), with_result=False)
            assert st.wait(), A.last_error()
            return result_dict(st.track_result())
        finally:
            dev.free()
            st.Release()
    m = K.check_analytic(track, motion, stride)
    print("analytic %s stride %d on the kernels: %s" % (motion, stride, m))
    assert m["final_q"] <= 4.0 * K.MEASURED_Q[(motion, stride)] and m["final"] < m["initial"] / 100.0, m


def test_cli_cone_track(hip, tmp_path):
    """adcensus_cli on the Cone pair with --tsdf and --tsdf-track: the run's own map as the second frame (so the true pose is the pose the
    map was fused at, the identity) from a perturbed guess.  <out>-track.txt and the report line equal the reference pipeline on the
    run's own files (the reference integrator, the reference ray cast from the guess, the reference tracker with the CLI's z_far); every
    other file equals a run without the flag.  tests/tsdf_track_checks.py (c): the displacement of the map's points between the
    recovered and the true pose is smaller than the initial one.  Measured on the reference: 0.409 m against 0.463 m, a ratio of 0.88
    (one disparity step of this calibration is 0.28 m of depth, the volume holds a quarter of the map's pixels, and max_dist is the
    default 0.1 m), so the assertion is the ratio's cap alone: below 1."""
    import os
    import subprocess
    from PIL import Image
    from tests import tsdf_raycast_cases as RC
    from tests import tsdf_ref as T
    from tests.test_gpu_outputs import CONE_CALIB
    from tests.test_tsdf_api import read_pfm
    A = hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "adcensus_amd", "bin", "adcensus_cli")
    left, right, opt = cases.make_case("cone")
    h, w = left.shape[:2]
    Image.fromarray(np.ascontiguousarray(left[:, :, ::-1])).save(tmp_path / "l.png")
    Image.fromarray(np.ascontiguousarray(right[:, :, ::-1])).save(tmp_path / "r.png")
    nx, ny, nz, voxel, origin, trunc = RC.CONE_VOLUME
    spec = "%d,%d,%d,%.9g,%.9g,%.9g,%.9g,%.9g" % (nx, ny, nz, voxel, origin[0], origin[1], origin[2], trunc)
    calib_arg = ["--calib", ",".join("%.9g" % x for x in CONE_CALIB)]
    guess = KC.pose(KC.TC.rot(0.05, -0.08, 0.03), (0.01, -0.008, 0.015))
    (tmp_path / "guess.txt").write_text("\n".join("%.9g" % v for v in guess[0] + guess[1]))

    def run(pref, *extra):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), str(opt.min_disparity), str(opt.max_disparity), str(tmp_path / pref), *calib_arg,
                            "--tsdf", spec, *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    run("plain")
    out = run("track", "--tsdf-track", str(tmp_path / "plain.pfm") + "," + str(tmp_path / "guess.txt"))
    names = sorted(f[len("plain"):] for f in os.listdir(tmp_path) if f.startswith("plain-") or f.startswith("plain."))
    assert len(names) >= 5 and "-tsdf.ply" in names and "-track.txt" not in names
    for suffix in names:
        assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / "track") + suffix, "rb").read(), suffix
    # the reference pipeline on the run's own map
    disp = read_pfm(str(tmp_path / "track.pfm"))
    want, want_text, line = cli_track_reference(disp, left, CONE_CALIB, RC.CONE_VOLUME, None, guess)
    text = (tmp_path / "track-track.txt").read_text()
    assert text == want_text, (text, want["R"], want["t"])
    assert line in out, (line, out[-600:])
    # (c): the map's own points between the recovered and the true pose (the identity)
    Z, valid = T.RR.source_z(disp, T.FROM_DISPARITY, CONE_CALIB)
    ys, xs = np.nonzero(valid)
    Zv = Z[ys, xs].astype(np.float64)
    Pc = np.stack([(xs - CONE_CALIB[2]) / CONE_CALIB[0] * Zv, (ys - CONE_CALIB[3]) / CONE_CALIB[0] * Zv, Zv], -1)

    def moved(R, t):
        return float(np.sqrt((((Pc @ np.asarray(R, np.float64).reshape(3, 3).T + np.asarray(t, np.float64)) - Pc) ** 2).sum(-1)).max())
    initial, final = moved(*guess), moved([float(x) for x in text.split()[:9]], [float(x) for x in text.split()[9:]])
    print("cone through the CLI: initial %.4f m, final %.4f m, ratio %.3f, %s after %d solves, %d used" % (initial, final, final / initial, line.split(":")[1].split(" after")[0],
                                                                                                      want["solves"], want["counts"]["used"]))
    assert want["counts"]["used"] > 10000 and final < initial, (initial, final)
