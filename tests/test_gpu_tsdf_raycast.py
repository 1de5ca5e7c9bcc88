"""GPU tier of the TSDF volume's ray cast (adcensus_amd/csrc/k_tsdf_raycast.hip): the kernel against tests/tsdf_raycast_ref.py bit for
bit on every case of tests/tsdf_raycast_cases.py -- depth, normals, colour and status as raw words into poisoned buffers whose bytes
behind the last pixel must stay poisoned, the report word for word; each output alone; refusals that need a real handle; integrate
then ray-cast without a wait, two ray casts of different view sizes back to back, a Match enqueued behind a pending ray cast; the host
entry point (scratch on first use, a smaller view after a larger one); the geometric checks of tests/tsdf_raycast_checks.py once on
the kernel; the Cone pair through the CLI."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from tests import cases
from tests import tsdf_raycast_cases as RC
from tests import tsdf_raycast_checks as K
from tests import tsdf_raycast_ref as RR
from tests import tsdf_ref as T
from tests.test_gpu_outputs import CONE_CALIB, POISON, DeviceBuffers, _handle
from tests.test_tsdf_api import c_frame, c_params, read_pfm
from tests.test_tsdf_raycast_api import c_view, rep_words

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TAIL = 64  # poisoned bytes behind every output buffer
BYTES = dict(depth=4, normals=16, bgr=3, status=1)
OUTPUTS = ("depth", "normals", "bgr", "status")


def _open(A, p, volume, size=(48, 36)):
    st = _handle(A, size[0], size[1], pyoracle.Option(max_disparity=16))
    assert st.tsdf_create(c_params(p)), A.last_error()
    st.tsdf_upload(*volume)
    return st


def _enqueue(A, st, dev, v, which):
    """adc_tsdf_raycast_device into fresh poisoned buffers -> {output: device address}"""
    P = v["width"] * v["height"]
    ptr = {k: dev.alloc(BYTES[k] * P + TAIL, POISON) for k in which}
    assert st.tsdf_raycast_device(c_view(v), *[ptr.get(k) for k in OUTPUTS]), A.last_error()
    return ptr


def _collect(dev, v, ptr, what):
    """the outputs as bytes; everything behind the last pixel must still be poisoned"""
    P = v["width"] * v["height"]
    got = {}
    for k, p in ptr.items():
        raw = dev.get(p, BYTES[k] * P + TAIL, np.uint8)
        assert (raw[BYTES[k] * P:] == POISON).all(), "%s: written behind the last pixel of %s" % (what, k)
        got[k] = raw[:BYTES[k] * P].tobytes()
    return got


def _check(what, got, want, rep):
    for k, b in got.items():
        assert b == want[k].tobytes(), "%s: %s differs on %d bytes" % (what, k, int((np.frombuffer(b, np.uint8) != np.frombuffer(want[k].tobytes(), np.uint8)).sum()))
    assert rep_words(rep) == RR.report_words(want["report"]) + [0] * 8, (what, rep_words(rep), want["report"])


def _outputs_of(c):
    return tuple(k for k in OUTPUTS if k != "bgr" or c["volume"][1] is not None)


@pytest.mark.parametrize("name", RC.CASE_NAMES)
def test_kernel_equals_the_reference(hip, name):
    A = hip
    c, want = RC.case(name), RC.reference(name)
    st, dev = _open(A, c["params"], c["volume"]), DeviceBuffers(A)
    try:
        assert st.tsdf_raycast_report() is None
        ptr = _enqueue(A, st, dev, c["view"], _outputs_of(c))
        assert st.wait(), A.last_error()
        _check(name, _collect(dev, c["view"], ptr, name), want, st.tsdf_raycast_report())
        after = st.tsdf_download()
        assert after[0].tobytes() == c["volume"][0].tobytes()  # (the volume is only read)
    finally:
        dev.free()
        st.Release()


def test_each_output_alone_and_refusals(hip):
    """every output alone and all together on a colour volume; refused calls write nothing and keep the report; bgr without a colour
    volume is refused, not ignored"""
    A = hip
    name = "rotated"
    c, want = RC.case(name), RC.reference(name)
    v = c["view"]
    st, dev = _open(A, c["params"], c["volume"]), DeviceBuffers(A)
    try:
        for which in [(k,) for k in OUTPUTS] + [OUTPUTS, ("depth", "status"), ("normals", "bgr")]:
            ptr = _enqueue(A, st, dev, v, which)
            assert st.wait(), A.last_error()
            _check("%s %s" % (name, which), _collect(dev, v, ptr, str(which)), want, st.tsdf_raycast_report())
        before = bytes(st.tsdf_raycast_report())
        pp = dev.alloc(16 * v["width"] * v["height"] + TAIL, POISON)
        bad = dict(v, max_steps=0)
        for call, why in ((lambda: st.tsdf_raycast_device(c_view(v)), "no output"), (lambda: st.tsdf_raycast_device(c_view(v), pp + 2), "4-byte aligned"),
                          (lambda: st.tsdf_raycast_device(c_view(v), None, pp + 8), "16-byte aligned"), (lambda: st.tsdf_raycast_device(c_view(bad), pp), "max_steps"),
                          (lambda: st.tsdf_raycast_device(None, pp), "null params")):
            assert not call() and why in A.last_error(), (why, A.last_error())
        assert st.wait() and bytes(st.tsdf_raycast_report()) == before and (dev.get(pp, 16 * v["width"] * v["height"] + TAIL, np.uint8) == POISON).all()
        plain = RC.case("inside")
        assert st.tsdf_create(c_params(plain["params"])), A.last_error()
        st.tsdf_upload(*plain["volume"])
        assert not st.tsdf_raycast_device(c_view(plain["view"]), None, None, pp) and "colour volume" in A.last_error()
        with pytest.raises(RuntimeError):
            st.tsdf_raycast(c_view(plain["view"]), bgr=True)
        assert (dev.get(pp, 64, np.uint8) == POISON).all()
        assert st.tsdf_destroy() and not st.tsdf_raycast_device(c_view(v), pp) and "no volume" in A.last_error()
    finally:
        dev.free()
        st.Release()


def test_host_entry_point_scratch_and_a_smaller_view_after_a_larger_one(hip):
    A = hip
    big, small = RC.case("scene_256x192"), RC.case("scene_37x23")  # (the same volume)
    st = _open(A, big["params"], big["volume"])
    try:
        for c, name in ((big, "scene_256x192"), (small, "scene_37x23"), (big, "scene_256x192")):
            want = RC.reference(name)
            d, n, b, s, rep = st.tsdf_raycast(c_view(c["view"]), bgr=True)
            _check(name, dict(depth=d.tobytes(), normals=n.tobytes(), bgr=b.tobytes(), status=s.tobytes()), want, rep)
            assert bytes(st.tsdf_raycast_report()) == bytes(rep)
        d, n, b, s, rep = st.tsdf_raycast(c_view(small["view"]), normals=False, status=False)
        assert n is None and b is None and s is None and d.tobytes() == RC.reference("scene_37x23")["depth"].tobytes()
    finally:
        st.Release()


def test_back_to_back_and_a_match_behind_a_pending_ray_cast(hip, oracle):
    """adc_tsdf_integrate_device then adc_tsdf_raycast_device without a wait; two ray casts of different view sizes back to back (the
    report is that of the last); adc_tsdf_raycast_device and adc_match_device enqueued back to back with ONE adc_wait: the maps, the
    report and the Match's map are exact -- the report words lie where no Match writes.  While the Match is pending a ray cast is refused."""
    A = hip
    left, right, opt = cases.make_case("cone")
    h, w = left.shape[:2]
    want_d = oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    p = T.params(*RC.CONE_VOLUME, flags=T.COLOR)
    fr = T.frame(CONE_CALIB)
    vol, _ = T.integrate(T.empty(p), p, fr, want_d, left)
    v1 = RR.view(w // 4, h // 4, CONE_CALIB[0] / 4, CONE_CALIB[2] / 4, CONE_CALIB[3] / 4, z_near=1.0, z_far=40.0, step=0.02, skip=0.08)
    v2 = RR.view(77, 53, 500.0, 38.0, 26.0, *RC.pose(RC.TC.rot(1.0, -2.0, 0.5), (0.1, 0.0, 0.5)), z_near=1.0, z_far=40.0, step=0.02, skip=0.08)
    want1, want2 = RR.raycast(vol, p, v1), RR.raycast(vol, p, v2)
    assert want1["report"]["hit"] > 1000 and want2["report"]["hit"] > 300  # (the inputs are worth casting)
    st, dev = _handle(A, w, h, opt), DeviceBuffers(A)
    try:
        dl, dr, dm, dd = dev.new(left), dev.new(right), dev.new(want_d), dev.alloc(4 * w * h, POISON)
        assert st.tsdf_create(c_params(p)), A.last_error()
        assert st.tsdf_integrate_device(dm, c_frame(fr), dl), A.last_error()
        p1 = _enqueue(A, st, dev, v1, OUTPUTS)  # (no wait behind the integration)
        p2 = _enqueue(A, st, dev, v2, OUTPUTS)
        assert st.wait(), A.last_error()
        _check("second of two", _collect(dev, v2, p2, "v2"), want2, st.tsdf_raycast_report())
        got1 = _collect(dev, v1, p1, "v1")
        assert all(got1[k] == want1[k].tobytes() for k in OUTPUTS)
        p1 = _enqueue(A, st, dev, v1, OUTPUTS)
        assert st.match_device(dl, dr, dd), A.last_error()
        assert not st.tsdf_raycast_device(c_view(v1), p1["depth"]) and "Match is pending" in A.last_error()
        assert st.wait(), A.last_error()
        _check("behind a match", _collect(dev, v1, p1, "v1 again"), want1, st.tsdf_raycast_report())
        assert np.array_equal(dev.get(dd, (h, w), F).view(np.uint32), np.ascontiguousarray(want_d).view(np.uint32))
    finally:
        dev.free()
        st.Release()


def _gpu_cast(A):
    def cast(volume, p, v):
        st = _open(A, p, volume)
        try:
            d, n, _, s, rep = st.tsdf_raycast(c_view(v))
            return dict(depth=d, normals=n, status=s, report=rep)
        finally:
            st.Release()
    return cast


def test_geometric_checks_on_the_kernel(hip):
    """tests/tsdf_raycast_checks.py once on the GPU: the plane (one rotated pose, skip = 4 * step), the sphere at the middle voxel size,
    the round trip with adc_tsdf_integrate ON THE DEVICE (the integrator under test is the kernel's, the bound is the same)."""
    A = hip
    cast = _gpu_cast(A)
    print("plane:", K.check_plane(cast, 1, 4.0))
    print("sphere:", K.check_sphere(cast, K.SPHERE_VOXELS[1]))

    def integrate(vol, p, fr, Z):
        st = _handle(A, Z.shape[1], Z.shape[0], pyoracle.Option(max_disparity=16))
        try:
            assert st.tsdf_create(c_params(p)), A.last_error()
            st.tsdf_upload(*vol)
            st.tsdf_integrate(Z, c_frame(fr))
            return st.tsdf_download()
        finally:
            st.Release()
    m = K.check_roundtrip(cast, integrate)
    assert m["depth"] <= m["voxel"]


def test_cli_cone_round_trip(hip, tmp_path):
    """adcensus_cli on the Cone pair with --tsdf and --tsdf-raycast of the camera's own view, the round trip map -> volume -> map through
    the files.  <out>-ray.pfm equals, bit for bit, the reference's ray cast of the reference's integration of the run's .pfm; the report
    line and <out>-ray-n.png (the host's encoding of the reference's normals) likewise; every other file equals a run without the flag.

    Then the round trip's own check (tests/tsdf_raycast_checks.py, Round trip) on this real, noisy map.  In this volume a voxel
    (0.04 m) spans 3740 * 0.04 / 11.42 = 13.1 pixels at the nearest depth of the map, so a pixel is ruled out, from the run's .pfm
    and the calibration alone, when it has no depth or lies within 14 + 2 = 16 pixels of a depth step (4-neighbours more than one
    voxel edge apart in depth, or one of them without depth) or of the image border: 167792 of 168750 pixels, 99.4 % -- one disparity
    step of this calibration is 0.28 m of depth, seven voxels, so almost every 33 x 33 window of a real map holds a step; the share is
    capped at 99.5 %.  At every one of the 958 other pixels the status is HIT and the depth is within one voxel edge of the input
    depth (the largest difference on the reference: 0.0267 m).  With the two-pixel radius of the synthetic scene, whose premise (a
    voxel below one pixel) does not hold here, 67.3 % are ruled out, 27996 of 36511 others HIT, largest difference 1.82 m."""
    A = hip
    from PIL import Image
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    left, right, opt = cases.make_case("cone")
    h, w = left.shape[:2]
    Image.fromarray(np.ascontiguousarray(left[:, :, ::-1])).save(tmp_path / "l.png")
    Image.fromarray(np.ascontiguousarray(right[:, :, ::-1])).save(tmp_path / "r.png")
    nx, ny, nz, voxel, origin, trunc = RC.CONE_VOLUME
    spec = "%d,%d,%d,%.9g,%.9g,%.9g,%.9g,%.9g" % (nx, ny, nz, voxel, origin[0], origin[1], origin[2], trunc)
    calib_arg = ["--calib", ",".join("%.9g" % x for x in CONE_CALIB)]
    view_arg = "%d,%d,%.9g,%.9g,%.9g" % (w, h, CONE_CALIB[0], CONE_CALIB[2], CONE_CALIB[3])

    def run(pref, *extra):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), str(opt.min_disparity), str(opt.max_disparity), str(tmp_path / pref), *calib_arg,
                            "--tsdf", spec, *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    run("plain")
    out = run("ray", "--tsdf-raycast", view_arg)
    names = sorted(f[len("plain"):] for f in os.listdir(tmp_path) if f.startswith("plain-") or f.startswith("plain."))
    assert len(names) >= 5 and "-tsdf.ply" in names
    for suffix in names:
        assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / "ray") + suffix, "rb").read(), suffix
    disp = read_pfm(str(tmp_path / "ray.pfm"))
    p = T.params(nx, ny, nz, voxel, origin, trunc, flags=T.COLOR)
    vol, _ = T.integrate(T.empty(p), p, T.frame(CONE_CALIB), disp, left)
    step = float(F(voxel) * F(0.5))
    half = float(F(trunc) * F(0.5))
    v = RR.view(w, h, CONE_CALIB[0], CONE_CALIB[2], CONE_CALIB[3], z_near=float(F(voxel)), z_far=3.0e38, step=step, skip=max(half, step), max_steps=16384)
    want = RR.raycast(vol, p, v)
    got = read_pfm(str(tmp_path / "ray-ray.pfm"))
    assert got.shape == (h, w) and got.tobytes() == want["depth"].tobytes()
    assert "TSDF raycast: %u rays, %u miss, %u hit, %u no surface, %u behind, %u exhausted, " % tuple(RR.report_words(want["report"])[:6]) in out, out
    png = np.asarray(Image.open(tmp_path / "ray-ray-n.png"))
    has = want["normals"][..., 3] > 0
    enc = np.where(has[..., None], (np.rint(want["normals"][..., :3] * F(127.0)).astype(np.int64) + 128).astype(np.uint8), 0).astype(np.uint8)
    assert png.shape == (h, w, 3) and np.array_equal(png, enc)
    # the round trip's check on the run's own map
    Z, valid = T.RR.source_z(disp, T.FROM_DISPARITY, CONE_CALIB)
    Zin = np.where(valid, Z, np.inf).astype(F)
    h_v = float(F(voxel))
    radius = int(np.ceil(h_v * CONE_CALIB[0] / float(Zin[valid].min()))) + 2
    ruled = K.roundtrip_ruled_out(Zin, h_v, radius)
    c, dw, _ = K.geometry(p, v)
    inside = K.inner(p, c + np.where(np.isfinite(Zin), Zin, 0.0)[..., None].astype(np.float64) * dw, 2.0)
    judged = ~ruled & inside
    hit = want["status"] == RR.HIT
    err = np.abs(got.astype(np.float64) - Zin.astype(np.float64))
    print("cone round trip: radius %d, %d of %d pixels ruled out by the input (%.2f %%), %d judged, %d of them HIT, max |dZ| %.4f m (voxel %.2f m)"
          % (radius, ruled.sum(), ruled.size, 100 * ruled.mean(), judged.sum(), (judged & hit).sum(), float(err[judged & hit].max()) if (judged & hit).any() else -1, voxel))
    assert radius == 16 and abs(int(ruled.sum()) - 167792) <= 100 and ruled.mean() <= 0.995 and judged.sum() >= 900  # (what the map itself rules out)
    assert (hit | ~judged).all(), int((judged & ~hit).sum())
    assert (err[judged] <= h_v).all(), float(err[judged].max())
