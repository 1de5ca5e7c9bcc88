"""CPU tier of the surface normals from a disparity map: properties of tests/normals_ref.py (the definition the GPU tests hold the
kernel to) on analytic planes and constructed maps; the header the kernel includes (adcensus_amd/csrc/normals_fit.h), compiled alone
under g++ into a serial program (tests/emul/emul_normals.cpp) and held to the reference bit for bit on every case of
tests/normals_cases.py, once more under ASAN + UBSAN; and the new surface of the C ABI, the Python mirror, the facade and the CLI --
declared, exported, struct layouts, every refusal before a HIP call, malformed --normals, the sanitizer build of the CLI on the stub."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import normals_cases as NC
from tests import normals_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
ENTRY_POINTS = ["adc_normals_device", "adc_normals", "adc_get_normals_report"]
F = np.float32
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

# analytic planes n0 . P = h (n0 is normalised; h in the unit of the baseline), rendered at 64 x 48 with f = 800, B = 0.16
PLANES = [((0.3, 0.1, 1.0), 2.0), ((-0.5, 0.4, 1.0), 3.0), ((0.0, -0.7, 1.0), 2.5), ((0.8, 0.0, 0.6), 4.0), ((0.05, -0.02, 1.0), 1.5)]
PLANE_SIZE = (64, 48)
# the largest component error |reference + n0| over the interior pixels of every plane and both doffs, per radius, as measured from
# the reference (profiles/normals_accuracy.md); asserted at twice these
MEASURED_PLANE_ERROR = {1: 6.54e-3, 3: 8.60e-4, 7: 3.01e-4}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def plane_map(W, H, n0, h, calib):
    """The disparity a camera (calib) sees of the plane n0 . P = h, in float64, rounded once to float32; and the unit n0."""
    f, B, cx, cy, doffs = (float(v) for v in calib)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    n0 = np.asarray(n0, np.float64)
    n0 = n0 / np.linalg.norm(n0)
    d = f * B * (n0[0] * (x - cx) / f + n0[1] * (y - cy) / f + n0[2]) / h - doffs
    return d.astype(F), n0


def plane_errors():
    """{radius: the largest component error over the interior of every plane of PLANES, doffs 0 and 1.3}"""
    W, H = PLANE_SIZE
    worst = {}
    for r in (1, 3, 7):
        worst[r] = 0.0
        for doffs in (0.0, 1.3):
            calib = NC.calib_for(W, H, doffs)
            for n0, h in PLANES:
                d, n = plane_map(W, H, n0, h, calib)
                assert d.min() > 1.0
                out, _, rep = N.normals(d, calib, r, 64.0, 3)
                assert rep["fitted"] == W * H, rep
                inner = out[r:H - r, r:W - r, :3].astype(np.float64)
                worst[r] = max(worst[r], float(np.abs(inner + n).max()))  # (the normal faces the camera: -n0)
    return worst


# ---------------------------------------------------------------------------------------------- properties of the reference alone
def test_reference_recovers_analytic_planes():
    """Five planes, doffs 0 and 1.3, 64 x 48, f = 800: every interior normal of the reference agrees with -n0.  Largest component
    error measured from the reference: 6.54e-3 at r = 1, 8.60e-4 at r = 3, 3.01e-4 at r = 7 (the fixed-point step of 1/1024 pixel over a
    window of 3, 7, 15 pixels); asserted at twice the measured value, and strictly falling with the radius."""
    worst = plane_errors()
    print("largest component error on planes:", worst)
    for r, measured in MEASURED_PLANE_ERROR.items():
        assert worst[r] <= 2 * measured, (r, worst[r])
    assert worst[1] > worst[3] > worst[7] > 0


def test_fronto_parallel_plane_is_exactly_minus_z():
    W, H = 40, 30
    for doffs in (0.0, 1.3):
        calib = NC.calib_for(W, H, doffs)
        d, _ = plane_map(W, H, (0, 0, 1), 2.0, calib)
        for r in (1, 3, 7):
            out, out8, rep = N.normals(d, calib, r, 1.0, 3)
            assert rep == dict(usable=W * H, fitted=W * H, few_points=0, degenerate=0)
            assert (out[..., 0] == 0).all() and (out[..., 1] == 0).all() and (out[..., 2] == -1).all()
            assert (out8 == np.array([128, 128, 1, 255], np.uint8)).all()


def test_unit_length_and_support_count():
    """Every valid normal has | ||n|| - 1 | <= 2^-22; w is the support count; where there is no normal everything is 0."""
    for name in NC.CASE_NAMES:
        c = NC.case(name)
        out, out8, rep = NC.reference(name)
        s, usable, _ = N.sums(c["map"], c["radius"], c["max_diff"])
        valid = out8[..., 3] == 255
        assert int(valid.sum()) == rep["fitted"] and not (valid & ~usable).any()
        norm = np.sqrt((out[..., :3].astype(np.float64) ** 2).sum(axis=-1))
        assert (np.abs(norm[valid] - 1) <= 2.0 ** -22).all(), name
        assert np.array_equal(out[..., 3][valid], s["n"][valid].astype(F)) and (s["n"][valid] >= c["min_points"]).all()
        assert (s["n"][usable] >= 1).all()  # (the centre is always a tap)
        assert (bits(out)[~valid] == 0).all() and (out8[~valid] == 0).all()
        # facing the camera: the normal dotted with the pixel's viewing ray is -s / L < 0 (up to the rounding of the float32 components)
        H, W = usable.shape
        f, _, cx, cy, _ = c["calib"]
        y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        o = out.astype(np.float64)
        dot = o[..., 0] * (x - cx) / f + o[..., 1] * (y - cy) / f + o[..., 2]
        assert (dot[valid] < 1e-5).all(), (name, dot[valid].max())


def test_a_step_edge_changes_no_normal():
    """Two slanted planes 10 pixels of disparity apart, max_diff = 1: the normals of each side are those of the side fitted alone."""
    W, H = 48, 30
    calib = NC.calib_for(W, H, 0.5)
    d = NC.slanted(W, H, d0=20.0, gx=0.1, gy=-0.05, noise=0.02)
    d[:, 24:] += F(10)
    for r in (1, 3, 7):
        both = N.normals(d, calib, r, 1.0, 3)[0]
        left, right = d.copy(), d.copy()
        left[:, 24:] = np.inf
        right[:, :24] = np.inf
        assert np.array_equal(bits(both[:, :24]), bits(N.normals(left, calib, r, 1.0, 3)[0][:, :24])), r
        assert np.array_equal(bits(both[:, 24:]), bits(N.normals(right, calib, r, 1.0, 3)[0][:, 24:])), r
        # ... and a gate that reaches across the step does change them
        assert not np.array_equal(bits(both), bits(N.normals(d, calib, r, 16.0, 3)[0]))


def test_cases_are_what_they_are_named():
    for name in NC.MIXED_ALL_CLASSES:
        rep = NC.reference(name)[2]
        assert rep["fitted"] > 0 and rep["few_points"] > 0 and rep["degenerate"] > 0, (name, rep)
    assert NC.reference("one_1x1")[2] == dict(usable=1, fitted=0, few_points=1, degenerate=0)
    assert NC.reference("two_2x2_full")[2]["fitted"] == 0 and NC.reference("window_9x7_r7_full")[2]["fitted"] == 0
    for name in ("row_1x40", "column_40x1"):  # collinear taps
        rep = NC.reference(name)[2]
        assert rep["fitted"] == 0 and rep["usable"] == 40 == rep["degenerate"] + rep["few_points"], rep
    assert NC.reference("window_9x7_r7")[2]["fitted"] == 63
    m = NC.mixed_map()
    a = np.abs(m)
    assert np.isposinf(m).any() and np.isneginf(m).any() and np.isnan(m).any() and (a[np.isfinite(a)] >= 32768).any() and (m < 0).any()
    assert {NC.case(n)["radius"] for n in NC.CASE_NAMES} >= {1, 3, 7}
    assert {N.gate(NC.case(n)["max_diff"]) for n in NC.CASE_NAMES} >= {0, 1024, 65536}
    assert any(NC.case(n)["min_points"] == (2 * NC.case(n)["radius"] + 1) ** 2 for n in NC.CASE_NAMES)
    assert NC.case("tiles_r7")["size"] == (131, 70)


# ---------------------------------------------------------------------------------------------- the shared header, serially
def _build_emul(tmp, sanitize):
    exe = os.path.join(tmp, "emul_normals_san" if sanitize else "emul_normals")
    cmd = ["g++", "-std=c++17", "-O1" if sanitize else "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "emul", "emul_normals.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emul_normals(tmp_path_factory):
    return _build_emul(str(tmp_path_factory.mktemp("emul_normals")), False)


def _run_emul(exe, name, tmp):
    c = NC.case(name)
    ind, outd = os.path.join(tmp, "in"), os.path.join(tmp, "out")
    os.makedirs(ind, exist_ok=True)
    os.makedirs(outd, exist_ok=True)
    c["map"].tofile(os.path.join(ind, "map.bin"))
    W, H = c["size"]
    f, _, cx, cy, doffs = c["calib"]
    r = subprocess.run([exe, str(W), str(H)] + ["%.9g" % v for v in (f, cx, cy, doffs)] + [str(c["radius"]), "%.9g" % c["max_diff"], str(c["min_points"]), ind, outd],
                       env=SAN_ENV, capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out, out8, rep = NC.reference(name)
    got = np.fromfile(os.path.join(outd, "normals.bin"), F).reshape(H, W, 4)
    assert np.array_equal(bits(got), bits(out)), (name, int((bits(got) != bits(out)).sum()))
    assert np.array_equal(np.fromfile(os.path.join(outd, "normals8.bin"), np.uint8).reshape(H, W, 4), out8), name
    assert np.fromfile(os.path.join(outd, "report.bin"), np.uint32).tolist() == N.report_words(rep), name


@pytest.mark.parametrize("name", NC.CASE_NAMES)
def test_shared_header_equals_the_reference(emul_normals, name, tmp_path):
    _run_emul(emul_normals, name, str(tmp_path))


def test_shared_header_under_sanitizers(tmp_path):
    """The same program built once with ASAN + UBSAN: signed overflow in the sums or the determinants, an out-of-range float-to-int
    conversion and reads outside the map are reports, and a report is a failure."""
    exe = _build_emul(str(tmp_path), True)
    for name in NC.CASE_NAMES:
        _run_emul(exe, name, str(tmp_path))
    assert subprocess.run([exe], env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe, "4", "4", "100", "2", "2", "0", "1", "1", "3", str(tmp_path / "absent"), str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe, "4", "4", "100", "2", "2", "0", "8", "1", "3", str(tmp_path), str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    assert re.search(r"#define\s+ADC_NORMALS_MAX_RADIUS\s+7\b", text) and A.NORMALS_MAX_RADIUS == N.MAX_RADIUS == 7
    for phrase in ("(int32)rintf(max_diff * 1024.0f)", "a < 32768.0f", "Gram determinant", "ONE rounding to nearest even", "always faces the camera"):
        assert phrase in text, phrase
    for lib in (A.LIB_PATH, os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(ENTRY_POINTS) <= names, lib
    # the struct layouts, asked of a C compiler; the existing structs keep theirs
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(adc_normals_params), offsetof(adc_normals_params, max_diff),\n'
                   ' offsetof(adc_normals_params, min_points), offsetof(adc_normals_params, flags), offsetof(adc_normals_params, reserved_),\n'
                   ' sizeof(adc_normals_report), offsetof(adc_normals_report, degenerate), sizeof(adc_calib), sizeof(adc_outputs), sizeof(adc_products)); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    P, Rp = A.NormalsParams, A.NormalsReport
    assert got == [C.sizeof(P), P.max_diff.offset, P.min_points.offset, P.flags.offset, P.reserved_.offset, C.sizeof(Rp), Rp.degenerate.offset, C.sizeof(A.Calib),
                   C.sizeof(A.Outputs), C.sizeof(A.Products)]
    assert got[0] == 32 and got[5] == 16 and got[7:] == [20, 48, 80]
    p = A.NormalsParams()
    assert (p.radius, p.max_diff, p.min_points, p.flags, list(p.reserved_)) == (2, 1.0, 5, 0, [0, 0, 0, 0])
    p = A.NormalsParams(radius=7, max_diff=0.5, min_points=225)
    assert (p.radius, p.max_diff, p.min_points) == (7, 0.5, 225)


def test_every_refusal_comes_before_a_hip_call():
    """No device here: each of these returns 1 with a message without touching HIP.  A block of ones stands in for a handle with a
    Match pending (every flag nonzero): the last check of all, so everything in front of it is reached on it; a zeroed block for an
    idle handle that has completed nothing."""
    L = A.lib()
    vp = C.c_void_p
    assert L.adc_normals_device.argtypes == [vp, vp, C.POINTER(A.Calib), C.POINTER(A.NormalsParams), vp, vp]
    assert L.adc_normals.argtypes == [vp, vp, C.POINTER(A.Calib), C.POINTER(A.NormalsParams), vp, vp, C.POINTER(A.NormalsReport)]
    idle = C.cast(C.create_string_buffer(1 << 20), vp)
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), vp)
    dev = vp(4096)
    good = A.Calib(100.0, 0.16, 10.0, 5.0, 0.0)
    rep = A.NormalsReport()

    def refused(rc, *words):
        msg = A.last_error()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    calls = {
        "adc_normals_device": lambda h, m, c, p=None, a=dev, b=dev: L.adc_normals_device(h, m, c, None if p is None else C.byref(p), a, b),
        "adc_normals": lambda h, m, c, p=None, a=dev, b=dev: L.adc_normals(h, m, c, None if p is None else C.byref(p), a, b, C.byref(rep)),
    }
    for who, call in calls.items():
        refused(call(None, dev, C.byref(good)), who, "null handle")
        refused(call(busy, None, C.byref(good)), who, "null map")
        refused(call(busy, dev, None), who, "null calibration")
        for k in range(5):
            for v in (float("nan"), float("inf")):
                vals = [100.0, 0.16, 10.0, 5.0, 0.0]
                vals[k] = v
                refused(call(busy, dev, C.byref(A.Calib(*vals))), "non-finite")
        for f in (0.0, -100.0):
            refused(call(busy, dev, C.byref(A.Calib(f, 0.16, 10.0, 5.0, 0.0))), "focal_px must be positive")
        for r in (0, -1, 8, 2 ** 31 - 1, -2 ** 31):
            refused(call(busy, dev, C.byref(good), A.NormalsParams(radius=r)), who, "radius")
        for md in (0.0, -1.0, 64.5, float("nan"), float("inf"), -float("inf")):
            refused(call(busy, dev, C.byref(good), A.NormalsParams(max_diff=md)), who, "max_diff")
        for r, mp in ((1, 2), (1, 10), (2, 26), (7, 226), (3, 0), (3, -5)):
            refused(call(busy, dev, C.byref(good), A.NormalsParams(radius=r, min_points=mp)), who, "min_points")
        for flags in (1, 2, 0x80000000, 0xFFFFFFFF):
            refused(call(busy, dev, C.byref(good), A.NormalsParams(flags=flags)), who, "unknown flag")
        for k in range(4):
            p = A.NormalsParams()
            p.reserved_[k] = 1
            refused(call(busy, dev, C.byref(good), p), who, "reserved")
        refused(call(busy, dev, C.byref(good), None, None, None), who, "no output requested")
        # everything in range passes the argument checks and reaches the handle's state
        for p in (None, A.NormalsParams(1, 64.0, 9), A.NormalsParams(7, 2.0 ** -12, 225), A.NormalsParams(3, 1.0, 3)):
            refused(call(busy, dev, C.byref(good), p), who, "Match is pending")
        refused(call(busy, dev, C.byref(good), None, dev, None), "Match is pending")
        refused(call(busy, dev, C.byref(good), None, None, dev), "Match is pending")
    for bad in (4096 + 4, 4096 + 8, 4096 + 1):
        refused(calls["adc_normals_device"](busy, dev, C.byref(good), None, vp(bad), dev), "adc_normals_device", "16-byte aligned")
    for bad in (4096 + 1, 4096 + 2, 4096 + 3):
        refused(calls["adc_normals_device"](busy, dev, C.byref(good), None, dev, vp(bad)), "adc_normals_device", "4-byte aligned")
        refused(calls["adc_normals_device"](busy, vp(bad), C.byref(good), None, dev, dev), "adc_normals_device", "4-byte aligned")
    refused(L.adc_get_normals_report(None, C.byref(rep)), "null")
    refused(L.adc_get_normals_report(idle, None), "null")
    refused(L.adc_get_normals_report(idle, C.byref(rep)), "no normals call")
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    st.width, st.height = 8, 4
    with pytest.raises(RuntimeError):
        st.normals(np.zeros((4, 8), F), good)
    with pytest.raises(RuntimeError):
        st.normals_report()
    assert st.normals_device(4096, good, d_normals=4096) is False


CALLER = r'''
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
int main() {
    ADCensusStereo s; ADCensusOption o;
    uint8 img[96] = {0}, n8[128];
    float32 d[32] = {0}, n[128];
    adc_calib c = {100.f, 0.16f, 4.f, 2.f, 0.f};
    adc_normals_params p = {1, 1.0f, 3, 0u, {0u, 0u, 0u, 0u}};
    adc_normals_report rep;
    // before Initialize there is no matcher underneath: everything is refused
    bool ok = !s.Normals(d, &c, &p, n, n8, &rep) && !s.Normals(d, &c, nullptr, n, nullptr, nullptr) && !s.GetNormalsReport(&rep);
    return (ok && !s.Match(img, img, d) && !s.Initialize(0, 0, o)) ? 0 : 1;
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
    assert "ADCensusStereo::Normals(float const*, adc_calib const*, adc_normals_params const*, float*, unsigned char*, adc_normals_report*)" in out
    assert "ADCensusStereo::GetNormalsReport(adc_normals_report*)" in out
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def test_cli_rejects_malformed_normals_flags(tmp_path):
    """Checked while the arguments are parsed: the images named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    base = [cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "0", "64", str(tmp_path / "out"), "--calib", "100,0.16,40,20,0"]
    for bad in [["--normals"], ["--normals", ""], ["--normals", ","], ["--normals", "0"], ["--normals", "8"], ["--normals", "-1"], ["--normals", "two"],
                ["--normals", "2x"], ["--normals", "2,"], ["--normals", "2,0"], ["--normals", "2,-1"], ["--normals", "2,64.5"], ["--normals", "2,nan"],
                ["--normals", "2,inf"], ["--normals", "2,1,"], ["--normals", "2,1,2"], ["--normals", "2,1,26"], ["--normals", "1,1,10"], ["--normals", "2,1,5,0"],
                ["--normals", "2,1,5x"], ["--normals", "2.5"], ["--normals", "2,1x"]]:
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--normals refused" in r.stdout and "Image Loading" not in r.stdout, (bad, r.stdout)
    r = subprocess.run(base[:6] + ["--normals", "2"], capture_output=True, text=True, timeout=120)  # (without --calib)
    assert r.returncode != 0 and "--normals refused: it needs --calib" in r.stdout and "Image Loading" not in r.stdout
    for good in ("2", "7,64,225", "1,0.5", "3,1,49"):
        r = subprocess.run(base + ["--normals", good], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Image Loading" in r.stdout and "--normals refused" not in r.stdout, good  # (well-formed: gets as far as the images)


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = (int(v) for v in f.readline().split())
        f.readline()
        return np.ascontiguousarray(np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1])


def read_ply(path):
    """-> (has normals, structured array of the vertices)"""
    with open(path, "rb") as f:
        blob = f.read()
    head, body = blob.split(b"end_header\n", 1)
    n = int(re.search(rb"element vertex (\d+)", head).group(1))
    with_n = b"property float nx" in head
    fields = [("xyz", "<f4", 3)] + ([("n", "<f4", 3)] if with_n else []) + [("rgb", "u1", 3)]
    assert (b"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red" in head) == with_n
    return with_n, np.frombuffer(body, np.dtype(fields), n)


def check_cli_files(pref, plain_pref, calib, radius, max_diff, min_points):
    """<pref>-n.png and the normals of <pref>-cloud.ply against the reference on <pref>.pfm; the points are those of the plain run."""
    from PIL import Image
    disp = read_pfm(pref + ".pfm")
    out, out8, rep = N.normals(disp, calib, radius, max_diff, min_points)
    assert np.array_equal(np.array(Image.open(pref + "-n.png").convert("RGB")), out8[..., :3])
    a = np.abs(disp)
    ok = np.isfinite(a) & (a + F(calib[4]) > 0)
    with_n, ply = read_ply(pref + "-cloud.ply")
    plain_n, plain = read_ply(plain_pref + "-cloud.ply")
    assert with_n and not plain_n and len(ply) == len(plain) == int(ok.sum())
    assert np.array_equal(ply["xyz"].view(np.uint32), plain["xyz"].view(np.uint32)) and np.array_equal(ply["rgb"], plain["rgb"])
    assert np.array_equal(np.ascontiguousarray(ply["n"]).view(np.uint32), bits(out[..., :3][ok]))
    return rep


def test_cli_normals_under_sanitizers(tmp_path):
    """The flag's parsing, <out>-n.png and the cloud's normals in the ASAN / UBSAN build on the stub C ABI, whose normals are
    normals_fit.h run serially: the files equal tests/normals_ref.py; with --voxel the ply stays as it is."""
    from PIL import Image
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "adcensus_amd", "host"), "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cli = os.path.join(ROOT, "adcensus_amd", "build", "asan", "adcensus_cli_asan")
    rng = np.random.default_rng(11)
    w, h = 83, 57
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "l.png")
    Image.fromarray(rgb[:, ::-1].copy()).save(tmp_path / "r.png")
    calib = (70.0, 0.16, 41.3, 28.2, 1.25)

    def run(*extra):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "-3", "29", *extra, "--calib", ",".join("%.9g" % v for v in calib)], env=SAN_ENV,
                           capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        return r

    assert run(str(tmp_path / "plain")).returncode == 0
    assert not os.path.exists(str(tmp_path / "plain") + "-n.png")
    for pref, arg, params in (("n2", "2", (2, 1.0, 5)), ("n7", "7,64,3", (7, 64.0, 3)), ("n1", "1,0.25", (1, 0.25, 5))):
        r = run(str(tmp_path / pref), "--normals", arg)
        assert r.returncode == 0, r.stdout
        assert open(str(tmp_path / "plain") + ".pfm", "rb").read() == open(str(tmp_path / pref) + ".pfm", "rb").read()
        rep = check_cli_files(str(tmp_path / pref), str(tmp_path / "plain"), calib, *params)
        assert "%u usable pixels, %u fitted, %u with too few points, %u degenerate" % tuple(N.report_words(rep)) in r.stdout
    assert N.normals(read_pfm(str(tmp_path / "n7") + ".pfm"), calib, 7, 64.0, 3)[2]["fitted"] > 100
    # with --voxel the ply is the voxel cloud's, unchanged by --normals
    assert run(str(tmp_path / "vox"), "--voxel", "0.05").returncode == 0
    assert run(str(tmp_path / "voxn"), "--voxel", "0.05", "--normals", "2").returncode == 0
    assert open(str(tmp_path / "vox") + "-cloud.ply", "rb").read() == open(str(tmp_path / "voxn") + "-cloud.ply", "rb").read()
    assert os.path.exists(str(tmp_path / "voxn") + "-n.png")
