"""CPU tier of the registration of depth into a second camera: properties of tests/register_ref.py (the definition the GPU tests hold
the kernels to) on constructed scenes; the header the kernels include (adcensus_amd/csrc/reg_project.h), compiled alone under g++ into a
serial program (tests/emul/emul_register.cpp) and held to the reference bit for bit on every case of tests/register_cases.py, once
more under ASAN + UBSAN; and the new surface of the C ABI, the Python mirror, the facade and the CLI -- declared, exported, struct
layouts, every refusal before a HIP call, malformed --register, the sanitizer build of the CLI on the plain-C stub."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import register_cases as RC
from tests import register_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
ENTRY_POINTS = ["adc_set_register_target", "adc_clear_register_target", "adc_register_depth_device", "adc_align_color_device", "adc_register_depth",
                "adc_align_color", "adc_get_register_report"]
F = np.float32
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------- properties of the reference alone
def test_identity_returns_the_input():
    """R = I, t = 0, the source's own intrinsics, no distortion, FROM_DEPTH: depth is the input bit for bit at every valid pixel, index
    the raster index, nothing else is filled."""
    W, H = 80, 48
    m = RC.scene(W, H, R.FROM_DEPTH)
    m[np.isfinite(m) & (m > 1e30)] = F(np.inf)  # (3e38 is a valid depth whose X overflows: not part of the identity)
    calib = RC.calib_for(W, H)
    depth, index, rep = R.register(m, R.FROM_DEPTH, calib, RC.target("identity", W, H, W, H))
    valid = np.isfinite(m) & (m > 0)
    assert valid.sum() > 0.99 * m.size and (~valid).sum() >= 5
    assert np.array_equal(bits(depth)[valid], bits(m)[valid]) and np.isposinf(depth[~valid]).all()
    assert np.array_equal(index[valid], np.arange(W * H, dtype=np.int32).reshape(H, W)[valid]) and (index[~valid] == -1).all()
    assert rep["src_valid"] == rep["src_projected"] == rep["dst_filled"] == rep["candidates"] == int(valid.sum())
    # the same camera moved sideways: surfaces at different depths now meet in the target
    _, _, shifted = R.register(m, R.FROM_DEPTH, calib, RC.target("shift", W, H, W, H))
    print("shift on 80x48: %d candidates on %d pixels" % (shifted["candidates"], shifted["dst_filled"]))
    assert shifted["candidates"] > shifted["dst_filled"] > 0


def test_a_constant_plane_on_one_pixel_keeps_the_lowest_raster_index():
    W, H = 40, 24
    m = np.full((H, W), 5, F)
    m[0, :3] = [np.nan, np.inf, -1]  # (the first three pixels have no depth: index 3 is the lowest that has)
    calib = RC.calib_for(W, H)
    depth, index, rep = R.register(m, R.FROM_DEPTH, calib, RC.target("tiny", W, H, 3, 3), splat=False)
    assert rep["src_valid"] == rep["src_projected"] == rep["candidates"] == W * H - 3 and rep["dst_filled"] == 1 and rep["tied"] == 1
    assert index[1, 1] == 3 and depth[1, 1] == 5 and (np.delete(index.ravel(), 4) == -1).all()


def test_the_foreground_wins_wherever_both_land():
    """A near rectangle in front of a far plane under a sideways shift, against a dictionary built one footprint at a time."""
    W, H = 48, 30
    m = np.full((H, W), 40, F) + (np.arange(W, dtype=F) * F(0.01))[None, :]
    fg = np.zeros((H, W), bool)
    fg[8:20, 14:30] = True
    m[fg] = 8
    calib = RC.calib_for(W, H)
    T = RC.target("shift", W, H, W, H)
    depth, index, rep = R.register(m, R.FROM_DEPTH, calib, T)
    fp = R.footprints(m, R.FROM_DEPTH, calib, T)
    landed = {}
    for y in range(H):
        for x in range(W):
            if not fp["projected"][y, x]:
                continue
            for i in range(fp["i0"][y, x], fp["i1"][y, x] + 1):
                for j in range(fp["j0"][y, x], fp["j1"][y, x] + 1):
                    landed.setdefault((i, j), []).append((float(fp["zc"][y, x]), y * W + x))
    assert len(landed) == rep["dst_filled"] == int((index >= 0).sum())
    both = 0
    for (i, j), cands in landed.items():
        z, src = min(cands)
        assert depth[i, j] == F(z) and index[i, j] == src
        kinds = {bool(fg.ravel()[s]) for _, s in cands}
        if len(kinds) == 2:
            both += 1
            assert fg.ravel()[index[i, j]], (i, j, cands)
    assert both >= 12  # (the rectangle is 12 rows high and moves over the plane)


def test_collision_and_tie_cases_are_what_they_are_named():
    for name, splat in RC.COLLISION_CASES:
        rep = RC.reference(name, splat)[2]
        assert rep["candidates"] > rep["dst_filled"] > 0, (name, rep)
    for name, splat in RC.TIE_CASES:
        rep = RC.reference(name, splat)[2]
        assert rep["tied"] > 0, (name, rep)
    assert RC.reference("behind")[2]["src_valid"] > 0 and RC.reference("behind")[2]["src_projected"] == 0
    assert RC.reference("huge")[2]["src_valid"] > 0 and RC.reference("huge")[2]["src_projected"] == 0
    fp = R.footprints(RC.case("cap")["map"], R.FROM_DEPTH, RC.case("cap")["calib"], RC.case("cap")["target"])
    assert ((fp["j1"] - fp["j0"] + 1)[fp["projected"]].max() == R.MAX_SPLAT) and RC.reference("cap")[2]["src_projected"] > 0


# ---------------------------------------------------------------------------------------------- the shared header, serially
def _build_emul(tmp, sanitize):
    exe = os.path.join(tmp, "emul_register_san" if sanitize else "emul_register")
    cmd = ["g++", "-std=c++17", "-O1" if sanitize else "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "emul", "emul_register.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emul_register(tmp_path_factory):
    return _build_emul(str(tmp_path_factory.mktemp("emul_register")), False)


def _run_emul(exe, name, splat, tmp):
    c = RC.case(name)
    ind, outd = os.path.join(tmp, "in"), os.path.join(tmp, "out")
    os.makedirs(ind, exist_ok=True)
    os.makedirs(outd, exist_ok=True)
    c["map"].tofile(os.path.join(ind, "map.bin"))
    c["tbgr"].tofile(os.path.join(ind, "tbgr.bin"))
    with open(os.path.join(ind, "target.bin"), "wb") as f:
        f.write(bytes(c["target"]))
    (W, H), (Wt, Ht) = c["size"], c["tsize"]
    r = subprocess.run([exe, str(W), str(H), str(c["kind"]), str(int(splat))] + ["%.9g" % v for v in c["calib"]] + [ind, outd], env=SAN_ENV,
                       capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    depth, index, rep = RC.reference(name, splat)
    aligned, valid = RC.reference_align(name)
    got = np.fromfile(os.path.join(outd, "depth.bin"), F).reshape(Ht, Wt)
    assert np.array_equal(bits(got), bits(depth)), (name, splat)
    assert np.array_equal(np.fromfile(os.path.join(outd, "index.bin"), np.int32).reshape(Ht, Wt), index), (name, splat)
    assert np.fromfile(os.path.join(outd, "report.bin"), np.uint32).tolist() == R.report_words(rep), (name, splat)
    assert np.array_equal(np.fromfile(os.path.join(outd, "aligned.bin"), np.uint8).reshape(H, W, 3), aligned), name
    assert np.array_equal(np.fromfile(os.path.join(outd, "valid.bin"), np.uint8).reshape(H, W), valid), name


@pytest.mark.parametrize("name", RC.CASE_NAMES)
def test_shared_header_equals_the_reference(emul_register, name, tmp_path):
    for splat in (True, False):
        _run_emul(emul_register, name, splat, str(tmp_path))


def test_shared_header_under_sanitizers(tmp_path):
    """The same program built once with ASAN + UBSAN: out-of-range float-to-int conversions, signed overflow in the clip and reads or
    writes outside the z-buffer, the maps or the colour image are reports, and a report is a failure."""
    exe = _build_emul(str(tmp_path), True)
    for name in ("rot5_small", "tiny_3x3", "cap", "row_widest", "column_1x1", "huge", "behind", "shift_1x1"):
        for splat in (True, False):
            _run_emul(exe, name, splat, str(tmp_path))
    assert subprocess.run([exe], env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe, "4", "4", "0", "1", "1", "1", "0", "0", "0", str(tmp_path / "absent"), str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    for name, value in (("ADC_REG_FROM_DISPARITY", "0"), ("ADC_REG_FROM_DEPTH", "1"), ("ADC_REG_NO_SPLAT", "1u"), ("ADC_REG_MAX_SPLAT", "8")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), text), name
    assert (A.REG_FROM_DISPARITY, A.REG_FROM_DEPTH, A.REG_NO_SPLAT, A.REG_MAX_SPLAT) == (R.FROM_DISPARITY, R.FROM_DEPTH, 1, R.MAX_SPLAT)
    assert "cracks" in text and "tile the target only approximately" in text  # (the header says that footprints tile only approximately)
    for lib in (A.LIB_PATH, os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(ENTRY_POINTS) <= names, lib
    # the struct layouts, asked of a C compiler; the existing structs keep theirs
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(adc_reg_target), offsetof(adc_reg_target, fx), offsetof(adc_reg_target, k1),\n'
                   ' offsetof(adc_reg_target, R), offsetof(adc_reg_target, t), sizeof(adc_reg_report), offsetof(adc_reg_report, dst_filled),\n'
                   ' sizeof(adc_calib), sizeof(adc_outputs), sizeof(adc_products)); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    T, Rp = A.RegTarget, A.RegReport
    assert got == [C.sizeof(T), T.fx.offset, T.k1.offset, T.R.offset, T.t.offset, C.sizeof(Rp), Rp.dst_filled.offset, C.sizeof(A.Calib), C.sizeof(A.Outputs),
                   C.sizeof(A.Products)]
    assert got[0] == 92 and got[5] == 16 and got[7:] == [20, 48, 80]
    t = A.RegTarget(width=3, height=2, fx=1.5, R=np.arange(9), t=[7, 8, 9])
    assert (t.width, t.height, t.fx, list(t.R), list(t.t)) == (3, 2, 1.5, list(range(9)), [7, 8, 9]) and list(A.RegTarget().R) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    with pytest.raises(AttributeError):
        A.RegTarget(focal=1)


def test_every_refusal_comes_before_a_hip_call():
    """No device here: each of these returns 1 with a message without touching HIP.  A zeroed block stands in for an idle handle without a
    target; a block of ones for a handle with a target set and a Match pending (every flag nonzero)."""
    L = A.lib()
    vp = C.c_void_p
    assert L.adc_register_depth_device.argtypes == [vp, vp, C.c_int, C.POINTER(A.Calib), C.c_uint32, vp, vp]
    assert L.adc_align_color_device.argtypes == [vp, vp, C.c_int, C.POINTER(A.Calib), vp, vp, vp]
    idle = C.cast(C.create_string_buffer(1 << 20), vp)
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), vp)
    dev = vp(4096)
    good = A.Calib(100.0, 0.16, 10.0, 5.0, 0.0)
    rep = A.RegReport()

    def refused(rc, *words):
        msg = A.last_error()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    ok_t = A.RegTarget(width=8, height=4, fx=100, fy=100)
    refused(L.adc_set_register_target(None, C.byref(ok_t)), "adc_set_register_target", "null handle")
    refused(L.adc_set_register_target(idle, None), "null target")
    for w, h in ((0, 4), (8, 0), (-1, 4), (32768, 4), (8, 32768)):
        refused(L.adc_set_register_target(idle, C.byref(A.RegTarget(width=w, height=h, fx=100, fy=100))), "[1, 32767]")
    for field in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3"):
        for v in (float("nan"), float("inf"), -float("inf")):
            refused(L.adc_set_register_target(idle, C.byref(A.RegTarget(**dict(dict(width=8, height=4, fx=100, fy=100), **{field: v})))), "non-finite")
    for k in range(9):
        Rm = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        Rm[k] = float("nan")
        refused(L.adc_set_register_target(idle, C.byref(A.RegTarget(width=8, height=4, fx=100, fy=100, R=Rm))), "non-finite")
    refused(L.adc_set_register_target(idle, C.byref(A.RegTarget(width=8, height=4, fx=100, fy=100, t=[0, float("inf"), 0]))), "non-finite")
    refused(L.adc_set_register_target(idle, C.byref(A.RegTarget(width=8, height=4, fx=0, fy=100))), "fx and fy")
    refused(L.adc_set_register_target(idle, C.byref(A.RegTarget(width=8, height=4, fx=100, fy=-0.0))), "fx and fy")
    refused(L.adc_set_register_target(busy, C.byref(ok_t)), "Match is pending")
    refused(L.adc_clear_register_target(None), "null handle")
    refused(L.adc_clear_register_target(busy), "Match is pending")
    assert L.adc_clear_register_target(idle) == 0
    calls = {
        "adc_register_depth_device": lambda h, m, kind, c, flags=0, a=dev, b=dev: L.adc_register_depth_device(h, m, kind, c, flags, a, b),
        "adc_register_depth": lambda h, m, kind, c, flags=0, a=dev, b=dev: L.adc_register_depth(h, m, kind, c, flags, a, b, C.byref(rep)),
        "adc_align_color_device": lambda h, m, kind, c, flags=0, a=dev, b=dev: L.adc_align_color_device(h, m, kind, c, a, b, None),
        "adc_align_color": lambda h, m, kind, c, flags=0, a=dev, b=dev: L.adc_align_color(h, m, kind, c, a, b, None),
    }
    for who, call in calls.items():
        refused(call(None, dev, 0, C.byref(good)), who, "null handle")
        refused(call(busy, None, 0, C.byref(good)), who, "null map")
        refused(call(busy, dev, 0, None), who, "null calibration")
        for kind in (-1, 2, 77):
            refused(call(busy, dev, kind, C.byref(good)), "unknown input kind")
        for k in range(5):
            for v in (float("nan"), float("inf")):
                vals = [100.0, 0.16, 10.0, 5.0, 0.0]
                vals[k] = v
                refused(call(busy, dev, 1, C.byref(A.Calib(*vals))), "non-finite")
        for f in (0.0, -100.0):
            refused(call(busy, dev, 0, C.byref(A.Calib(f, 0.16, 10.0, 5.0, 0.0))), "focal_px must be positive")
        refused(call(idle, dev, 0, C.byref(good)), "no target set")
        refused(call(busy, dev, 1, C.byref(good)), "Match is pending")
    for who in ("adc_register_depth_device", "adc_register_depth"):
        for flags in (4, 8, 0x80000000, 0xFFFFFFFF):
            refused(calls[who](busy, dev, 0, C.byref(good), flags), who, "unknown flag")
        refused(calls[who](busy, dev, 0, C.byref(good), 0, None, None), who, "no output requested")
        refused(calls[who](idle, dev, 0, C.byref(good), A.REG_NO_SPLAT, dev, None), "no target set")  # (a known flag and one output pass the argument checks)
    for who in ("adc_align_color_device", "adc_align_color"):
        refused(calls[who](busy, dev, 0, C.byref(good), 0, None, dev), who, "null target image")
        refused(calls[who](busy, dev, 0, C.byref(good), 0, dev, None), who, "no output requested")
    refused(L.adc_get_register_report(None, C.byref(rep)), "null")
    refused(L.adc_get_register_report(idle, None), "null")
    refused(L.adc_get_register_report(idle, C.byref(rep)), "no registration")
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    st.width, st.height = 8, 4
    with pytest.raises(RuntimeError):
        st.set_register_target(ok_t)
    with pytest.raises(RuntimeError):
        st.clear_register_target()
    with pytest.raises(RuntimeError):
        st.register_depth(np.zeros((4, 8), F), good)
    with pytest.raises(RuntimeError):
        st.align_color(np.zeros((4, 8), F), good, np.zeros((4, 8, 3), np.uint8))
    with pytest.raises(RuntimeError):
        st.register_report()
    assert st.register_depth_device(4096, good, d_depth=4096) is False and st.align_color_device(4096, good, 4096, 4096) is False


CALLER = r'''
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
int main() {
    ADCensusStereo s; ADCensusOption o;
    uint8 img[96] = {0}, out[96], valid[32];
    float32 d[32] = {0}, depth[32];
    sint32 index[32];
    adc_calib c = {100.f, 0.16f, 4.f, 2.f, 0.f};
    adc_reg_target t = {8, 4, 100.f, 100.f, 4.f, 2.f, 0.f, 0.f, 0.f, 0.f, 0.f, {1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
    adc_reg_report rep;
    // before Initialize there is no matcher underneath: everything is refused
    bool ok = !s.SetRegisterTarget(&t) && !s.ClearRegisterTarget() && !s.RegisterDepth(d, ADC_REG_FROM_DEPTH, &c, ADC_REG_NO_SPLAT, depth, index, &rep) &&
              !s.AlignColor(d, ADC_REG_FROM_DISPARITY, &c, img, out, valid);
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
    assert "ADCensusStereo::SetRegisterTarget(adc_reg_target const*)" in out and "ADCensusStereo::ClearRegisterTarget()" in out
    assert "ADCensusStereo::RegisterDepth(float const*, int, adc_calib const*, unsigned int, float*, int*, adc_reg_report*)" in out
    assert "ADCensusStereo::AlignColor(float const*, int, adc_calib const*, unsigned char const*, unsigned char*, unsigned char*)" in out
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def _target_text(t):
    vals = [t.width, t.height, t.fx, t.fy, t.cx, t.cy, t.k1, t.k2, t.p1, t.p2, t.k3] + list(t.R) + list(t.t)
    return "\n".join("%d" % v if k < 2 else "%.9g" % v for k, v in enumerate(vals)) + "\n"


def test_cli_rejects_malformed_register_flags(tmp_path):
    """Checked while the arguments are parsed: the images named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    base = [cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "0", "64", str(tmp_path / "out"), "--calib", "100,0.16,40,20,0"]
    good = _target_text(A.RegTarget(width=83, height=57, fx=100, fy=100, cx=40, cy=20))
    nums = good.split()
    files = {"good.txt": good, "short.txt": " ".join(nums[:-1]), "long.txt": good + "1\n", "word.txt": good.replace(nums[5], "forty"), "nan.txt": good.replace(nums[4], "nan", 1),
             "inf.txt": " ".join(nums[:12] + ["inf"] + nums[13:]), "zero_fx.txt": " ".join(nums[:2] + ["0"] + nums[3:]), "wide.txt": " ".join(["32768"] + nums[1:]),
             "flat.txt": " ".join(nums[:1] + ["0"] + nums[2:]), "frac.txt": " ".join(["83.5"] + nums[1:]), "big.txt": " ".join(nums[:6] + ["1e39"] + nums[7:]), "empty.txt": ""}
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    for bad in [["--register"], ["--register", ""], ["--register", ","], ["--register", ",c.png"], ["--register", str(tmp_path / "good.txt") + ","],
                ["--register", str(tmp_path / "good.txt") + ",a.png,b.png"], ["--register", str(tmp_path / "absent.txt")]] + \
            [["--register", str(tmp_path / n)] for n in files if n != "good.txt"]:
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--register refused" in r.stdout and "Image Loading" not in r.stdout, (bad, r.stdout)
    r = subprocess.run(base[:6] + ["--register", str(tmp_path / "good.txt")], capture_output=True, text=True, timeout=120)  # (without --calib)
    assert r.returncode != 0 and "--register refused: it needs --calib" in r.stdout and "Image Loading" not in r.stdout
    r = subprocess.run(base + ["--register", str(tmp_path / "good.txt") + ",c.png"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Image Loading" in r.stdout and "--register refused" not in r.stdout  # (well-formed: gets as far as the images)


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = (int(v) for v in f.readline().split())
        f.readline()
        return np.ascontiguousarray(np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1])


def test_cli_register_under_sanitizers(tmp_path):
    """The flag's parsing, the target file, the colour image, <out>-reg.pfm, <out>-aligned.png and the recoloured cloud in the ASAN /
    UBSAN build on the stub C ABI, whose registration is the header's definition in plain C: the files equal tests/register_ref.py."""
    from PIL import Image
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "adcensus_amd", "host"), "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cli = os.path.join(ROOT, "adcensus_amd", "build", "asan", "adcensus_cli_asan")
    rng = np.random.default_rng(11)
    w, h, wt, ht = 83, 57, 120, 70
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "l.png")
    Image.fromarray(rgb[:, ::-1].copy()).save(tmp_path / "r.png")
    colour = rng.integers(1, 256, (ht, wt, 3), dtype=np.uint8)
    Image.fromarray(colour).save(tmp_path / "colour.png")
    calib = (70.0, 0.16, 41.3, 28.2, 1.25)
    T = A.RegTarget(width=wt, height=ht, fx=100, fy=98, cx=60.2, cy=35.1, R=RC.rot(1.0, 3.0), t=[-0.05, 0.01, 0.0], k1=-0.1, k2=0.02, p1=0.001, p2=-0.0005, k3=0.001)
    (tmp_path / "target.txt").write_text(_target_text(T))

    def run(*extra):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "-3", "29", *extra, "--calib", ",".join("%.9g" % v for v in calib)], env=SAN_ENV,
                           capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        return r

    assert run(str(tmp_path / "plain")).returncode == 0
    r = run(str(tmp_path / "reg"), "--register", "%s,%s" % (tmp_path / "target.txt", tmp_path / "colour.png"))
    assert r.returncode == 0, r.stdout
    disp = read_pfm(str(tmp_path / "reg") + ".pfm")
    assert open(str(tmp_path / "plain") + ".pfm", "rb").read() == open(str(tmp_path / "reg") + ".pfm", "rb").read()
    depth, _, rep = R.register(disp, R.FROM_DISPARITY, calib, T)
    assert rep["dst_filled"] > 100
    assert np.array_equal(bits(read_pfm(str(tmp_path / "reg") + "-reg.pfm")), bits(depth))
    assert "%d valid source pixels, %d projected, %d target pixels filled" % (rep["src_valid"], rep["src_projected"], rep["dst_filled"]) in r.stdout
    aligned, valid = R.align(disp, R.FROM_DISPARITY, calib, T, colour[:, :, ::-1])
    assert valid.sum() > 100 and np.array_equal(np.array(Image.open(str(tmp_path / "reg") + "-aligned.png").convert("RGB")), aligned[:, :, ::-1])
    # the cloud: the points of the plain run with the colours of the aligned image
    def ply(path):
        with open(path, "rb") as f:
            blob = f.read()
        head, body = blob.split(b"end_header\n", 1)
        n = int(re.search(rb"element vertex (\d+)", head).group(1))
        return np.frombuffer(body, np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]), n)
    plain, reg = ply(str(tmp_path / "plain") + "-cloud.ply"), ply(str(tmp_path / "reg") + "-cloud.ply")
    a = np.abs(disp)
    ok = np.isfinite(a) & (a + F(calib[4]) > 0)
    assert len(reg) == len(plain) == int(ok.sum()) and np.array_equal(reg["xyz"].view(np.uint32), plain["xyz"].view(np.uint32))
    assert np.array_equal(reg["rgb"], aligned[:, :, ::-1][ok])
    assert not os.path.exists(str(tmp_path / "plain") + "-reg.pfm")
    # without a colour image: the registered depth alone; refused behind the images: a colour image of another size
    r = run(str(tmp_path / "depth_only"), "--register", str(tmp_path / "target.txt"))
    assert r.returncode == 0 and not os.path.exists(str(tmp_path / "depth_only") + "-aligned.png")
    assert np.array_equal(bits(read_pfm(str(tmp_path / "depth_only") + "-reg.pfm")), bits(depth))
    r = run(str(tmp_path / "bad"), "--register", "%s,%s" % (tmp_path / "target.txt", tmp_path / "l.png"))
    assert r.returncode != 0 and "--register refused" in r.stdout and not os.path.exists(str(tmp_path / "bad") + ".pfm")
