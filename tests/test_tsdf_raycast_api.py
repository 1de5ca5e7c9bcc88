"""CPU tier of the TSDF volume's ray cast: the header the kernel includes (adcensus_amd/csrc/tsdf_ray.h), compiled alone under g++ into
a serial program (tests/emul/emul_tsdf_raycast.cpp) and held to tests/tsdf_raycast_ref.py bit for bit on every case of
tests/tsdf_raycast_cases.py, once more under ASAN + UBSAN as its own executable; properties of the cases (each reaches the branch it is
there for); the checks of tests/tsdf_raycast_checks.py whose bounds come from geometry (plane, sphere, round trip with the integrator),
on the reference and on the serial program; and the new surface of the C ABI, the Python mirror, the facade and the CLI -- declared,
exported, every refusal before a HIP call, --tsdf-raycast without --tsdf."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import tsdf_raycast_cases as RC
from tests import tsdf_raycast_checks as K
from tests import tsdf_raycast_ref as RR
from tests import tsdf_ref as T
from tests.test_tsdf_api import SAN_ENV, c_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
F = np.float32


def c_view(v):
    return A.TsdfRaycastParams(v["width"], v["height"], v["focal_px"], v["cx"], v["cy"], v["R"], v["t"], v["z_near"], v["z_far"], v["step"], v["skip"],
                               v["min_weight"], v["max_steps"])


def rep_words(rep):
    return [getattr(rep, k) for k in RR.REPORT_FIELDS] + list(rep.reserved_)


# ---------------------------------------------------------------------------------------------- the cases and the reference alone
@pytest.mark.parametrize("name", RC.CASE_NAMES)
def test_cases_reach_their_branches(name):
    c, r = RC.case(name), RC.reference(name)
    rep, v = r["report"], c["view"]
    assert sum(rep[k] for k in RR.STATUS_NAMES) == rep["rays"] == v["width"] * v["height"]
    assert rep["samples_lo"] + (rep["samples_hi"] << 32) == int(r["samples"].sum()) and r["samples"].max() <= v["max_steps"]
    for status in RC.REACHES[name]:
        assert rep[status] > 0, (name, status)
    hit = r["status"] == RR.HIT
    assert (r["depth"][~hit] == 0).all() and (r["normals"][~hit] == 0).all() and (r["samples"][r["status"] == RR.MISS] == 0).all()
    assert (r["depth"][hit] >= F(v["z_near"])).all() and (r["depth"][hit] <= F(v["z_far"])).all()
    if name == "t_zero":  # f == 0 exactly at a sample: the hit lies ON that sample, on the layer of voxel centres whose t is 0
        assert (r["depth"][hit] == F(1.03125)).all() and hit.all()
    if name == "holes":   # a hit in a cell with an unseen corner: depth kept, normal zeros; hits whose nearest voxel has no colour
        zero = (r["normals"][hit] == 0).all(-1)
        assert 0 < zero.sum() < hit.sum() and ((r["bgr"][hit] == 0).all(-1)).sum() > 0
    if name == "exhausted":
        assert (r["samples"][r["status"] == RR.EXHAUSTED] == v["max_steps"]).all()
    if name in ("look_x", "look_y", "look_z"):  # the hit lies in the last cell of the looked-along axis
        axis = "xyz".index(name[-1])
        _, dw, _ = K.geometry(c["params"], v)
        cc = K.geometry(c["params"], v)[0]
        g = K.grid_of(c["params"], cc + r["depth"][..., None].astype(np.float64) * dw)[hit]
        n = (c["params"]["nx"], c["params"]["ny"], c["params"]["nz"])[axis]
        assert (np.floor(g[:, axis]) == n - 2).all()
        assert abs(dw[2, 3, (axis + 1) % 3]) == 0 and abs(dw[2, 3, (axis + 2) % 3]) == 0  # (the principal ray: two exactly zero components)


def test_skip_changes_the_cost_not_the_surface():
    """skip > step on a volume with saturated free space: fewer samples; the same rays hit, within the interpolation's reach"""
    a, b = RC.reference("skip_eq_step"), RC.reference("skip_gt_step")
    assert int(b["samples"].sum()) < int(a["samples"].sum())
    assert np.array_equal(a["status"], b["status"])
    hit = a["status"] == RR.HIT
    assert np.abs(a["depth"][hit] - b["depth"][hit]).max() < 0.05 * 0.05  # (a twentieth of a voxel)


# ---------------------------------------------------------------------------------------------- the shared header, serially
def _build_emul(tmp, sanitize):
    exe = os.path.join(tmp, "emul_tsdf_raycast_san" if sanitize else "emul_tsdf_raycast")
    cmd = ["g++", "-std=c++17", "-O1" if sanitize else "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "emul", "emul_tsdf_raycast.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emul_tsdf_raycast(tmp_path_factory):
    return _build_emul(str(tmp_path_factory.mktemp("emul_tsdf_raycast")), False)


def run_emul(exe, volume, p, v, d):
    """the serial program on (volume, params, view) in directory d -> the dict of tsdf_raycast_ref.raycast (without samples)"""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "case.bin"), "wb") as f:
        f.write(bytes(c_params(p)) + bytes(c_view(v)))
    np.ascontiguousarray(volume[0], np.uint32).tofile(os.path.join(d, "tsdf.bin"))
    if volume[1] is not None:
        np.ascontiguousarray(volume[1], np.uint32).tofile(os.path.join(d, "color.bin"))
    run = subprocess.run([exe, d, d], env=SAN_ENV, capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr and "LeakSanitizer" not in run.stderr, run.stderr[-3000:]
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    H, W = v["height"], v["width"]
    return dict(depth=np.fromfile(os.path.join(d, "depth.bin"), F).reshape(H, W), normals=np.fromfile(os.path.join(d, "normals.bin"), F).reshape(H, W, 4),
                status=np.fromfile(os.path.join(d, "status.bin"), np.uint8).reshape(H, W),
                bgr=None if volume[1] is None else np.fromfile(os.path.join(d, "bgr.bin"), np.uint8).reshape(H, W, 3),
                report=np.fromfile(os.path.join(d, "report.bin"), np.uint32).tolist())


def _emul_case(exe, name, tmp):
    c, want = RC.case(name), RC.reference(name)
    got = run_emul(exe, c["volume"], c["params"], c["view"], os.path.join(tmp, name))
    for k in ("depth", "normals", "status"):
        assert got[k].tobytes() == want[k].tobytes(), (name, k)
    assert (got["bgr"] is None) == (want["bgr"] is None) and (got["bgr"] is None or got["bgr"].tobytes() == want["bgr"].tobytes()), (name, "bgr")
    assert got["report"] == RR.report_words(want["report"]) + [0] * 8, name
    return os.path.join(tmp, name)


@pytest.mark.parametrize("name", RC.CASE_NAMES)
def test_shared_header_equals_the_reference(emul_tsdf_raycast, name, tmp_path):
    _emul_case(emul_tsdf_raycast, name, str(tmp_path))


def test_shared_header_under_sanitizers(tmp_path):
    """The same program built once with ASAN + UBSAN and run as its own executable: a read outside the volume, an overflowing integer,
    a float that does not fit its integer and a leak are reports, and a report is a failure."""
    exe = _build_emul(str(tmp_path), True)
    for name in RC.CASE_NAMES:
        d = _emul_case(exe, name, str(tmp_path))
    assert subprocess.run([exe], env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe, str(tmp_path / "absent"), str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2
    blob = bytearray(open(os.path.join(d, "case.bin"), "rb").read())
    blob[64:68] = (0).to_bytes(4, "little")  # width 0
    open(os.path.join(d, "case.bin"), "wb").write(bytes(blob))
    assert subprocess.run([exe, d, str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------- checks that rest on geometry
def _serial_cast(exe, tmp):
    count = [0]

    def cast(volume, p, v):
        count[0] += 1
        return run_emul(exe, volume, p, v, os.path.join(tmp, "check%d" % count[0]))
    return cast


@pytest.mark.parametrize("pose_index", (0, 1, 2))
def test_plane_depth_and_normal_within_the_derived_bounds(emul_tsdf_raycast, tmp_path, pose_index):
    """tests/tsdf_raycast_checks.py (Plane): every HIT within (q + r_pos + r_lerp) / s + r_z of the analytic intersection, every normal
    component within 2 * 1.05 * sqrt(3) / M + 1e-6, every ray that meets the plane more than a cell inside the box a HIT; three poses,
    the smallest |cos| of ray against normal at a judged pixel is above 0.5 (asserted); skip = step and skip = 4 * step."""
    for skip_factor in (1.0, 4.0):
        for cast in (RR.raycast, _serial_cast(emul_tsdf_raycast, str(tmp_path))):
            m = K.check_plane(cast, pose_index, skip_factor)
            print("plane pose %d skip %.0f: %s" % (pose_index, skip_factor, m))
            assert m["judged"] > 200 and m["min_cos"] >= K.MIN_COS


@pytest.mark.parametrize("voxel", K.SPHERE_VOXELS)
def test_sphere_depth_and_normal_within_the_derived_bounds(emul_tsdf_raycast, tmp_path, voxel):
    """tests/tsdf_raycast_checks.py (Sphere): radius 0.3 m on cells of 0.04, 0.02 and 0.0125 m.  Measured on the reference (depth in
    metres, share of the pixel's own bound; normal component): 2.44e-3 (0.55 of the bound) / 0.0706; 6.45e-4 (0.70) / 0.0380; 2.24e-4
    (0.75) / 0.0228, against normal bounds of 0.349, 0.130 and 0.075 -- profiles/tsdf_raycast_accuracy.md."""
    for cast in (RR.raycast, _serial_cast(emul_tsdf_raycast, str(tmp_path))):
        m = K.check_sphere(cast, voxel)
        print("sphere voxel %.4f: %s" % (voxel, m))
        assert m["judged"] > 400


def test_round_trip_with_the_integrator(emul_tsdf_raycast, tmp_path):
    """tests/tsdf_raycast_checks.py (round trip): a tilted plane behind a sphere integrated three times from a pose with the reference
    integrator, cast from the same pose: outside the pixels the INPUT map rules out (no depth, within two pixels of a depth step or of
    the image border: 1458 of 4800, the share the scene itself gives) every pixel is a HIT within one voxel edge of the input depth."""
    for cast in (RR.raycast, _serial_cast(emul_tsdf_raycast, str(tmp_path))):
        m = K.check_roundtrip(cast, lambda vol, p, fr, Z: T.integrate(vol, p, fr, Z)[0])
        assert abs(m["ruled_out"] - 1458) <= 2 and m["depth"] <= m["voxel"]  # (1458 of 4800: what the input map itself rules out)


# ---------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name in A.TSDF_RAYCAST_ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    for phrase in ("no ray takes more", "ray parameter IS the camera-frame depth Z", "the slab method", "refused without a\n * colour volume",
                   "the sign\n *   convention of adc_normals", "Not a product of adc_products or the farm"):
        assert phrase in text, phrase
    for lib in (A.LIB_PATH, os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(A.TSDF_RAYCAST_ENTRY_POINTS) <= names, lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d %d", sizeof(adc_tsdf_raycast_params), offsetof(adc_tsdf_raycast_params, z_near),\n'
                   'offsetof(adc_tsdf_raycast_params, max_steps), sizeof(adc_tsdf_raycast_report), offsetof(adc_tsdf_raycast_report, samples_lo),\n'
                   'ADC_TSDF_RAY_MISS, ADC_TSDF_RAY_HIT, ADC_TSDF_RAY_NO_SURFACE, ADC_TSDF_RAY_BEHIND, ADC_TSDF_RAY_EXHAUSTED); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    P, R = A.TsdfRaycastParams, A.TsdfRaycastReport
    assert got == [C.sizeof(P), P.z_near.offset, P.max_steps.offset, C.sizeof(R), R.samples_lo.offset, A.TSDF_RAY_MISS, A.TSDF_RAY_HIT, A.TSDF_RAY_NO_SURFACE,
                   A.TSDF_RAY_BEHIND, A.TSDF_RAY_EXHAUSTED] == [128, 68, 88, 64, 24, 0, 1, 2, 3, 4]
    assert [f[0] for f in R._fields_] == list(RR.REPORT_FIELDS) + ["reserved_"]
    assert (RR.MISS, RR.HIT, RR.NO_SURFACE, RR.BEHIND, RR.EXHAUSTED) == (0, 1, 2, 3, 4)


def _good_view():
    return A.TsdfRaycastParams(37, 23, 30.0, 18.0, 11.0, None, None, 0.05, 10.0, 0.025, 0.05, 1, 4096)


def test_every_refusal_comes_before_a_hip_call():
    """No device here: each of these returns 1 with a message without touching HIP.  A block of ones stands in for a handle that has a
    (colour) volume and a Match pending (every flag nonzero): the last check, so everything in front of it is reached on it; a zeroed
    block for an idle handle without a volume that has completed nothing."""
    L = A.lib()
    vp = C.c_void_p
    idle = C.cast(C.create_string_buffer(1 << 20), vp)
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), vp)
    dev = vp(4096)
    rep = A.TsdfRaycastReport()
    nan, inf = float("nan"), float("inf")

    def refused(rc, *words):
        msg = A.last_error()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    def device(h, p, d=dev, n=dev, c=dev, s=dev):
        return L.adc_tsdf_raycast_device(h, None if p is None else C.byref(p), d, n, c, s)

    def host(h, p, d=dev, n=dev, c=dev, s=dev):
        return L.adc_tsdf_raycast(h, None if p is None else C.byref(p), d, n, c, s, C.byref(rep))

    for who, call in (("adc_tsdf_raycast_device", device), ("adc_tsdf_raycast", host)):
        refused(call(None, _good_view()), who, "null handle")
        refused(call(busy, None), who, "null params")
        for field, values, word in (("width", (0, -1, 8193), "width, height"), ("height", (0, -5, 8193), "width, height"), ("focal_px", (0.0, -1.0, nan, inf), "focal_px"),
                                    ("cx", (nan, inf), "cx, cy"), ("cy", (nan, -inf), "cx, cy"), ("z_near", (0.0, -1.0, nan, 10.0, 11.0), "z_near"),
                                    ("z_far", (nan, inf, 0.01), "z_near"), ("step", (0.0, -0.1, nan, inf), "step"), ("skip", (0.02, nan, inf), "skip"),
                                    ("min_weight", (0, 65536), "min_weight"), ("max_steps", (0, 16385, 2 ** 32 - 1), "max_steps"), ("flags", (1, 2 ** 31), "flag")):
            for value in values:
                p = _good_view()
                setattr(p, field, value)
                refused(call(busy, p), who, word)
        for k in range(9):
            p = _good_view()
            p.R[k] = nan
            refused(call(busy, p), who, "R has a non-finite")
        for k in range(3):
            p = _good_view()
            p.t[k] = inf
            refused(call(busy, p), who, "t has a non-finite")
        for k in range(8):
            p = _good_view()
            p.reserved_[k] = 1
            refused(call(busy, p), who, "reserved")
        refused(call(busy, _good_view(), None, None, None, None), who, "no output requested")
        refused(call(idle, _good_view()), who, "no volume")
        for outs in ((dev, dev, dev, dev), (dev, None, None, None), (None, None, None, dev)):
            refused(call(busy, _good_view(), *outs), who, "Match is pending")
    for bad in (4097, 4098, 4099):
        refused(device(busy, _good_view(), vp(bad), None, None, None), "adc_tsdf_raycast_device", "d_depth must be 4-byte aligned")
    for bad in (4096 + 4, 4096 + 8, 4096 + 1):
        refused(device(busy, _good_view(), None, vp(bad), None, None), "adc_tsdf_raycast_device", "d_normals must be 16-byte aligned")
    refused(L.adc_get_tsdf_raycast_report(None, C.byref(rep)), "null")
    refused(L.adc_get_tsdf_raycast_report(idle, None), "null")
    refused(L.adc_get_tsdf_raycast_report(idle, C.byref(rep)), "no ray cast")
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    assert st.tsdf_raycast_device(_good_view(), 4096) is False and st.tsdf_raycast_report() is None
    with pytest.raises(RuntimeError):
        st.tsdf_raycast(_good_view())
    with pytest.raises(ValueError):
        st.tsdf_raycast(_good_view(), depth=False, normals=False, bgr=False, status=False)


CALLER = r'''
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
int main() {
    ADCensusStereo s; ADCensusOption o;
    uint8 img[96] = {0};
    float32 d[32] = {0};
    TsdfRaycastParams v = {};
    v.width = 4; v.height = 2; v.focal_px = 4.0f; v.R[0] = v.R[4] = v.R[8] = 1.0f;
    v.z_near = 0.1f; v.z_far = 2.0f; v.step = 0.01f; v.skip = 0.02f; v.min_weight = 1; v.max_steps = 64;
    adc_tsdf_raycast_report rep;
    float32 depth[8], normals[32];
    uint8 bgr[24], status[8];
    // before Initialize there is no matcher underneath: everything is refused
    bool ok = !s.TsdfRaycast(&v, depth, normals, bgr, status, &rep) && !s.TsdfRaycast(&v, depth, nullptr, nullptr, nullptr, nullptr) && !s.GetTsdfRaycastReport(&rep);
    return (ok && sizeof(TsdfRaycastParams) == sizeof(adc_tsdf_raycast_params) && !s.Match(img, img, d) && !s.Initialize(0, 0, o)) ? 0 : 1;
}
'''


def test_facade_compiles_and_exports_the_members(tmp_path):
    src = tmp_path / "caller.cpp"
    src.write_text(CALLER)
    libdir = os.path.join(ROOT, "adcensus_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libadcensus.so")):
        pytest.fail("libadcensus.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "caller"),
                    "-L", libdir, "-ladcensus", "-ladcensus_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(libdir, "libadcensus.so")], capture_output=True, text=True, check=True).stdout
    for member in ("TsdfRaycast(adc_tsdf_raycast_params const*, float*, float*, unsigned char*, unsigned char*, adc_tsdf_raycast_report*)",
                   "GetTsdfRaycastReport(adc_tsdf_raycast_report*)"):
        assert "ADCensusStereo::" + member in out, member
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def test_cli_rejects_tsdf_raycast_without_tsdf_and_bad_specs(tmp_path):
    """Checked while the arguments are parsed: the images named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    base = [cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "0", "64", str(tmp_path / "out")]
    calib = ["--calib", "100,0.16,40,20,0"]
    spec = ["--tsdf-raycast", "64,48,100,32,24"]
    tsdf = ["--tsdf", "8,8,8,0.1,0,0,1"]
    for args in (base + spec, base + calib + spec, [base[0]] + spec + base[1:] + calib, base + calib + spec + ["--view-pose", str(tmp_path / "p.txt")]):
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and r.stdout.startswith("--tsdf-raycast refused: it needs --tsdf") and "Image Loading" not in r.stdout, r.stdout
    r = subprocess.run(base + calib + tsdf + ["--view-pose", str(tmp_path / "p.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.stdout.startswith("--view-pose refused: it needs --tsdf-raycast") and "Image Loading" not in r.stdout, r.stdout
    for bad in ("64,48,100,32", "0,48,100,32,24", "64,48,-1,32,24", "64,48,100,32,24,0", "64,48,100,32,24,0.02,0.01", "64,48,100,32,24,0.02,0.04,9", "a,b,c,d,e"):
        r = subprocess.run(base + calib + tsdf + ["--tsdf-raycast", bad], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--tsdf-raycast refused" in r.stdout and "Image Loading" not in r.stdout, (bad, r.stdout)
    for args in (base + calib + tsdf + spec, base + calib + tsdf + ["--tsdf-raycast", "64,48,100,32,24,0.02,0.06"]):
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Image Loading" in r.stdout and "refused" not in r.stdout, r.stdout  # (well-formed: gets as far as the images)


def test_cli_tsdf_raycast_under_sanitizers(tmp_path):
    """<out>-ray.pfm and <out>-ray-n.png in the ASAN / UBSAN build on the stub C ABI, whose ray cast is tsdf_ray.h run serially: the
    depth map equals tests/tsdf_raycast_ref.py on the reference's integration of the run's .pfm, the image is the host's encoding of
    the reference's normals; the camera's own view (the pose of --pose) and a view of another size from --view-pose with STEP and SKIP
    given; every other file of the run is byte-identical to a run without the flag."""
    from PIL import Image
    from tests import tsdf_cases as TC
    from tests.test_tsdf_api import read_pfm
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "adcensus_amd", "host"), "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cli = os.path.join(ROOT, "adcensus_amd", "build", "asan", "adcensus_cli_asan")
    rng = np.random.default_rng(12)
    w, h = 83, 57
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "l.png")
    Image.fromarray(rgb[:, ::-1].copy()).save(tmp_path / "r.png")
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    calib = (70.0, 0.16, 41.3, 28.2, 1.25)
    calib_arg = ["--calib", ",".join("%.9g" % v for v in calib)]
    R, t = TC.rot(3.0, -4.0, 2.0), (0.02, -0.01, 0.03)
    (tmp_path / "pose.txt").write_text("\n".join("%.9g" % v for v in R + t))
    Rv, tv = RC.pose(TC.rot(-2.0, 5.0, 1.0), (0.05, 0.02, -0.1))
    (tmp_path / "view.txt").write_text("\n".join("%.9g" % v for v in Rv + tv))

    def run(pref, *extra):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "-3", "29", str(tmp_path / pref), *extra], env=SAN_ENV,
                           capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, r.stdout
        return r.stdout

    hits = 0
    for pref, spec, pose, ray, view_pose in (("r1", "32,24,32,0.04,-0.64,-0.48,0.35", False, "%d,%d,%.9g,%.9g,%.9g" % ((w, h) + calib[:1] + calib[2:4]), False),
                                             ("r2", "36,20,28,0.05,-0.9,-0.5,0.3,0.2,1", True, "45,31,40,22.5,15,0.02,0.07", True)):
        tsdf_args = ["--tsdf", spec, *calib_arg, *(["--pose", str(tmp_path / "pose.txt")] if pose else [])]
        run(pref + "_plain", *tsdf_args)
        out = run(pref, "--tsdf-raycast", ray, *(["--view-pose", str(tmp_path / "view.txt")] if view_pose else []), *tsdf_args)
        names = sorted(f[len(pref + "_plain"):] for f in os.listdir(tmp_path) if f.startswith(pref + "_plain-") or f.startswith(pref + "_plain."))
        assert len(names) >= 5 and "-tsdf.ply" in names and "-ray.pfm" not in names
        for suffix in names:
            assert open(str(tmp_path / (pref + "_plain")) + suffix, "rb").read() == open(str(tmp_path / pref) + suffix, "rb").read(), (pref, suffix)
        s = spec.split(",")
        voxel = float(s[3])
        trunc = float(F(3.0) * F(voxel)) if len(s) == 7 else float(s[7])
        p = T.params(int(s[0]), int(s[1]), int(s[2]), voxel, [float(x) for x in s[4:7]], trunc, flags=T.COLOR)
        fr = T.frame(calib, R, t) if pose else T.frame(calib)
        vol, _ = T.integrate(T.empty(p), p, fr, read_pfm(str(tmp_path / pref) + ".pfm"), bgr)
        a = ray.split(",")
        step = float(a[5]) if len(a) > 5 else float(F(voxel) * F(0.5))
        half = float(F(trunc) * F(0.5))
        skip = float(a[6]) if len(a) > 6 else max(half, step)
        vR, vt = (Rv, tv) if view_pose else (fr["R"], fr["t"])
        v = RR.view(int(a[0]), int(a[1]), float(a[2]), float(a[3]), float(a[4]), vR, vt, z_near=voxel, z_far=3.0e38, step=step, skip=skip, max_steps=16384)
        want = RR.raycast(vol, p, v)
        got = read_pfm(str(tmp_path / pref) + "-ray.pfm")
        assert got.shape == (v["height"], v["width"]) and got.tobytes() == want["depth"].tobytes(), pref
        png = np.asarray(Image.open(str(tmp_path / pref) + "-ray-n.png"))
        has = want["normals"][..., 3] > 0
        enc = np.where(has[..., None], (np.rint(want["normals"][..., :3] * F(127.0)).astype(np.int64) + 128).astype(np.uint8), 0).astype(np.uint8)
        assert np.array_equal(png, enc), pref
        rep = want["report"]
        assert "TSDF raycast: %u rays, %u miss, %u hit, %u no surface, %u behind, %u exhausted, %u samples\n" % (
            tuple(RR.report_words(rep)[:6]) + (rep["samples_lo"] + (rep["samples_hi"] << 32),)) in out, out
        hits += rep["hit"]
    assert hits > 300
