"""CPU tier of the voxel-grid filter of the cloud: tests/voxel_ref.py (the definition the GPU tests hold the kernels to) against a
word-for-word loop over a dictionary of integer triples; the header the kernels include (adcensus_amd/csrc/voxel_point.h), compiled alone
under g++ into a serial program (tests/emul/emul_voxel.cpp) and held to the reference bit for bit on hand-picked floats, once more under
ASAN + UBSAN; and the new surface of the C ABI, the Python mirror, the facade and the CLI -- declared, exported, struct layouts, every
refusal before a HIP call, malformed --voxel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import voxel_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
ENTRY_POINTS = ["adc_set_cloud_voxel_grid", "adc_clear_cloud_voxel_grid", "adc_get_voxel_report", "adc_farm_set_cloud_voxel_grid"]
F = np.float32
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _map(w, h, seed):
    rng = np.random.default_rng(seed)
    v = (F(1) + rng.random((h, w), dtype=F) * F(59)).astype(F)
    v[:, : w // 2] = np.sort(v[:, : w // 2], axis=1)  # (half of every row smooth: pixels that share voxels)
    v[rng.random((h, w)) < 0.1] *= F(-1)
    flat = v.reshape(-1)
    flat[rng.random(flat.size) < 0.05] = F(np.inf)
    flat[3::41] = F(np.nan)
    flat[5::43] = F(-np.inf)
    flat[7::47] = F(0)
    return v, rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- the reference against the loop
@pytest.mark.parametrize("seed", range(4))
def test_numpy_definition_equals_the_loop(seed):
    w, h = 45 + seed, 23
    disp, left = _map(w, h, seed)
    a = np.deg2rad(20.0 + seed)
    pose = (np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], F), np.array([0.3, -7.0, -2.0], F))
    for calib in ((100.0, 0.5, w / 2.0, h / 2.0, 0.0), (80.0, 0.3, 3.25, -1.5, -20.0)):
        for g in (V.grid(0.5), V.grid(0.02), V.grid(1e8), V.grid(1e-7), V.grid(0.3, 1.0, 4.0), V.grid(0.3, pose=pose)):
            got, rep = V.voxel_cloud(disp, left, calib, g)
            want, want_rep = V.voxel_cloud_loop(disp, left, calib, g)
            assert rep == want_rep and got.tobytes() == want.tobytes(), (calib, g)
            assert rep["voxels"] == len(got) <= rep["points_kept"] <= rep["points_valid"] < w * h
    got, rep = V.voxel_cloud(disp, left, (100.0, 0.5, w / 2.0, h / 2.0, 0.0), V.grid(1e8))
    assert len(got) == 4 and int(got["pad"].astype(int).sum()) <= rep["points_kept"] == rep["points_valid"]  # (one voxel per sign octant)
    assert V.voxel_cloud(disp, left, (100.0, 0.5, w / 2.0, h / 2.0, 0.0), V.grid(1e-7))[1]["points_kept"] == 0


def test_axis_edges():
    """tiny negative u: f == 1.0 and q clamps; +-2^20 and its neighbours; NaN and the infinities"""
    two20 = F(1048576.0)
    w = np.array([-1e-30, -0.0, 0.0, 1e-30, two20, -two20, np.nextafter(two20, F(0)), np.nextafter(-two20, F(0)), np.nextafter(two20, F(np.inf)),
                  np.nan, np.inf, -np.inf, 0.99999994, -0.99999994, 1.5, -1.5], F)
    ok, cell, q = V.axis(w, F(1))
    assert ok.tolist() == [True, True, True, True, False, False, True, True, False, False, False, False, True, True, True, True]
    assert (cell[0] - V.BIAS, q[0]) == (-1, 65535) and (cell[1] - V.BIAS, q[1]) == (0, 0) and (cell[3] - V.BIAS, q[3]) == (0, 0)
    assert cell[6] - V.BIAS == (1 << 20) - 1 and cell[7] == 0 and cell[6] < (1 << 21)
    assert (cell[14] - V.BIAS, q[14], cell[15] - V.BIAS, q[15]) == (1, 32768, -2, 32768)


# ---------------------------------------------------------------------------------------------- the shared header, serially
def _build_emul(tmp, sanitize):
    exe = os.path.join(tmp, "emul_voxel_san" if sanitize else "emul_voxel")
    cmd = ["g++", "-std=c++17", "-O1" if sanitize else "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "emul", "emul_voxel.cpp"), "-o", exe], check=True)
    return exe


def _hex(a):
    return ["%08x" % v for v in np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)]


def _picked():
    two20 = F(1048576.0)
    base = [-1e-30, -1e-45, -0.0, 0.0, 1e-45, 1e-30, two20, -two20, np.nextafter(two20, F(0)), np.nextafter(-two20, F(0)), np.nextafter(two20, F(np.inf)),
            np.nextafter(-two20, F(-np.inf)), np.nan, np.inf, -np.inf, 3.4e38, -3.4e38, 0.99999994, -0.99999994, 1.0, -1.0, 0.5, -0.5, 123456.789, -123456.789]
    rng = np.random.default_rng(5)
    return np.concatenate([np.array(base, F), ((rng.random(200, dtype=F) - F(0.5)) * F(100)).astype(F), (rng.random(50, dtype=F) * F(1e-3) - F(5e-4)).astype(F)])


def _run(exe, args, text):
    r = subprocess.run([exe] + args, input=text, capture_output=True, text=True, timeout=120, env=SAN_ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return [line.split() for line in r.stdout.splitlines()]


def _check_emul(exe):
    w = _picked()
    for inv in (F(1), F(F(1) / F(0.05)), F(F(1) / F(1e8)), F(F(1) / F(1e-7)), F(65536.0)):
        ok, cell, q = V.axis(w, inv)
        rows = _run(exe, ["axis", _hex(inv)[0]], "\n".join(_hex(w)) + "\n")
        assert len(rows) == len(w)
        for k, row in enumerate(rows):
            want = [1, int(cell[k]), int(q[k])] if ok[k] else [0, 0, 0]
            assert [int(v) for v in row] == want, (float(inv), float(w[k]), row, want)
    # whole points through crop, pose and key: a 1 x N "image" whose camera puts pixel x at X = x * Z, Y = 0 is not needed -- the
    # reference's per-axis function and the packing are enough: key = cells at 42 / 21 / 0
    rng = np.random.default_rng(6)
    pts = ((rng.random((300, 3), dtype=F) - F(0.5)) * F(40)).astype(F)
    pts[:25, 0] = _picked()[:25]
    pts[25:50, 2] = _picked()[:25]
    a = np.deg2rad(33.0)
    R = np.array([np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)], F)
    t = np.array([0.25, -3.0, 1.5], F)
    for leaf, zmin, zmax, pose in ((F(0.05), F(-np.inf), F(np.inf), None), (F(0.7), F(-5.0), F(5.0), (R, t)), (F(1e8), F(0), F(np.inf), (R, t))):
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        with np.errstate(invalid="ignore", over="ignore"):
            kept = (zmin <= z) & (z <= zmax)
            world = [x, y, z] if pose is None else [(((R[3 * r] * x + R[3 * r + 1] * y).astype(F) + R[3 * r + 2] * z).astype(F) + t[r]).astype(F) for r in range(3)]
        inv = F(F(1) / leaf)
        key = np.zeros(len(pts), np.uint64)
        qs = []
        for ax, wa in enumerate(world):
            ok, cell, q = V.axis(wa, inv)
            kept &= ok
            key |= np.where(ok, cell, 0).astype(np.uint64) << np.uint64(42 - 21 * ax)
            qs.append(q)
        args = ["point", _hex(leaf)[0], _hex(zmin)[0], _hex(zmax)[0]] + ([] if pose is None else _hex(R) + _hex(t))
        rows = _run(exe, args, "\n".join(" ".join(_hex(p)) for p in pts) + "\n")
        assert len(rows) == len(pts) and 0 < kept.sum()
        for k, row in enumerate(rows):
            want = [1, int(key[k]), int(qs[0][k]), int(qs[1][k]), int(qs[2][k])] if kept[k] else [0, 0, 0, 0, 0]
            assert [int(v) for v in row] == want, (k, pts[k], row, want)
    # records: sums past 32 bits, n past 255, every cell's ends
    recs = [(0, 1, (0, 0, 0), (0, 0, 0)), ((2097151 << 42) | (2097151 << 21) | 2097151, 3, (3 * 65535, 100, 7), (765, 1, 2)),
            ((V.BIAS - 1) << 42 | V.BIAS << 21 | (V.BIAS + 17), 1 << 30, (65535 << 30, 1 << 45, 12345678901), (255 << 30, 128 << 30, 1)),
            ((V.BIAS + 5) << 42 | (V.BIAS - 9) << 21 | V.BIAS, 256, (256 * 32768 + 127, 256 * 32768 + 128, 5), (127, 128, 129))]
    for leaf in (F(0.05), F(1e8), F(1e-7)):
        rows = _run(exe, ["record", _hex(leaf)[0]], "".join("%d %d %d %d %d %d %d %d\n" % ((k, n) + sq + sc) for k, n, sq, sc in recs))
        for (k, n, sq, sc), row in zip(recs, rows):
            cells = np.array([(k >> 42) & 0x1FFFFF, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF], np.int64)
            mq = np.array([(s + n // 2) // n for s in sq], np.int64)
            xyz = V.record_xyz(cells, mq, leaf)
            rgb = [(s + n // 2) // n for s in sc]
            want = _hex(xyz) + ["%08x" % (rgb[0] | rgb[1] << 8 | rgb[2] << 16 | min(n, 255) << 24)]
            assert row == want, (float(leaf), k, n, row, want)


def test_shared_header_equals_the_reference(tmp_path):
    _check_emul(_build_emul(str(tmp_path), False))


def test_shared_header_under_sanitizers(tmp_path):
    """The same program built with ASAN + UBSAN: an out-of-range float-to-int conversion or a signed overflow in the cell arithmetic is
    a report, and a report is a failure."""
    _check_emul(_build_emul(str(tmp_path), True))


# ---------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_(handle|farm)\s*\*" % name, text), name
    assert re.search(r"#define\s+ADC_VOXEL_POSE\s+\(0x1u\)", text) and A.VOXEL_POSE == 1
    for lib in (A.LIB_PATH, os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(ENTRY_POINTS) <= names, lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(adc_voxel_grid), offsetof(adc_voxel_grid, z_min),\n'
                   ' offsetof(adc_voxel_grid, z_max), offsetof(adc_voxel_grid, flags), offsetof(adc_voxel_grid, R), offsetof(adc_voxel_grid, t),\n'
                   ' offsetof(adc_voxel_grid, reserved), sizeof(adc_voxel_report), offsetof(adc_voxel_report, voxels), sizeof(adc_point), sizeof(adc_outputs),\n'
                   ' sizeof(adc_products)); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    G, Rp = A.VoxelGrid, A.VoxelReport
    assert got == [C.sizeof(G), G.z_min.offset, G.z_max.offset, G.flags.offset, G.R.offset, G.t.offset, G.reserved_.offset, C.sizeof(Rp), Rp.voxels.offset,
                   A.POINT_DTYPE.itemsize, C.sizeof(A.Outputs), C.sizeof(A.Products)]
    assert got[0] == 80 and got[7] == 12 and got[9:] == [16, 48, 80]  # (the existing structs keep their sizes)
    g = A.VoxelGrid(0.05)
    assert (g.leaf, g.z_min, g.z_max, g.flags, list(g.R)) == (F(0.05), 0.0, float("inf"), 0, [1, 0, 0, 0, 1, 0, 0, 0, 1])
    g = A.VoxelGrid(0.5, 1.0, 2.0, pose=(np.arange(9).reshape(3, 3), [7, 8, 9]))
    assert (g.flags, list(g.R), list(g.t), list(g.reserved_)) == (A.VOXEL_POSE, list(range(9)), [7, 8, 9], [0, 0, 0, 0])


def test_every_refusal_comes_before_a_hip_call():
    """No device here: each of these returns 1 with a message without touching HIP.  A zeroed block stands in for an idle handle, a
    block of ones for a handle with a Match pending (every flag nonzero)."""
    L = A.lib()
    vp = C.c_void_p
    assert L.adc_set_cloud_voxel_grid.argtypes == [vp, C.POINTER(A.VoxelGrid)] and L.adc_farm_set_cloud_voxel_grid.argtypes == [vp, C.POINTER(A.VoxelGrid)]
    idle = C.cast(C.create_string_buffer(1 << 20), vp)
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), vp)
    good = A.VoxelGrid(0.05)
    rep = A.VoxelReport()

    def refused(rc, *words):
        msg = A.last_error()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    refused(L.adc_set_cloud_voxel_grid(None, C.byref(good)), "adc_set_cloud_voxel_grid", "null handle")
    refused(L.adc_set_cloud_voxel_grid(idle, None), "null grid")
    for leaf in (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        refused(L.adc_set_cloud_voxel_grid(idle, C.byref(A.VoxelGrid(leaf))), "leaf")
    for zmin, zmax in ((1.0, 0.5), (float("nan"), 1.0), (0.0, float("nan")), (float("inf"), 0.0)):
        refused(L.adc_set_cloud_voxel_grid(idle, C.byref(A.VoxelGrid(0.05, zmin, zmax))), "z_min <= z_max")
    for k in range(12):
        for v in (float("nan"), float("inf")):
            vals = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
            vals[k] = v
            refused(L.adc_set_cloud_voxel_grid(idle, C.byref(A.VoxelGrid(0.05, pose=(vals[:9], vals[9:])))), "pose", "non-finite")
    g = A.VoxelGrid(0.05)
    g.flags = 2
    refused(L.adc_set_cloud_voxel_grid(idle, C.byref(g)), "unknown flags")
    g = A.VoxelGrid(0.05)
    g.reserved_[3] = 1
    refused(L.adc_set_cloud_voxel_grid(idle, C.byref(g)), "reserved")
    refused(L.adc_set_cloud_voxel_grid(busy, C.byref(good)), "Match is pending")
    refused(L.adc_clear_cloud_voxel_grid(None), "null handle")
    refused(L.adc_clear_cloud_voxel_grid(busy), "Match is pending")
    assert L.adc_clear_cloud_voxel_grid(idle) == 0
    refused(L.adc_get_voxel_report(None, C.byref(rep)), "null")
    refused(L.adc_get_voxel_report(idle, None), "null")
    refused(L.adc_farm_set_cloud_voxel_grid(None, C.byref(good)), "null farm")
    refused(L.adc_farm_set_cloud_voxel_grid(None, None), "null farm")
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    with pytest.raises(RuntimeError):
        st.set_cloud_voxel_grid(0.05)
    with pytest.raises(RuntimeError):
        st.clear_cloud_voxel_grid()
    with pytest.raises(RuntimeError):
        st.voxel_report()


CALLER = r'''
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
int main() {
    ADCensusStereo s; ADCensusOption o;
    uint8 img[96] = {0};
    float32 d[32] = {0};
    adc_voxel_grid g = {0.05f, 0.f, 10.f, 0u, {1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}, {0, 0, 0, 0}};
    adc_voxel_report rep;
    // before Initialize there is no matcher underneath: everything is refused
    bool ok = !s.SetCloudVoxelGrid(&g) && !s.ClearCloudVoxelGrid() && !s.GetVoxelReport(&rep);
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
    assert "ADCensusStereo::SetCloudVoxelGrid(adc_voxel_grid const*)" in out and "ADCensusStereo::ClearCloudVoxelGrid()" in out
    assert "ADCensusStereo::GetVoxelReport(adc_voxel_report*) const" in out
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def test_cli_rejects_malformed_voxel_flags(tmp_path):
    """Checked while the arguments are parsed: the images named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    base = [cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "0", "64", str(tmp_path / "out"), "--calib", "100,0.16,40,20,0"]
    for bad in (["--voxel"], ["--voxel", ""], ["--voxel", "0"], ["--voxel", "-0.05"], ["--voxel", "nan"], ["--voxel", "inf"], ["--voxel", "leaf"],
                ["--voxel", "0.05x"], ["--voxel", "0.05,"], ["--voxel", "0.05,1"], ["--voxel", "0.05,1,"], ["--voxel", "0.05,2,1"], ["--voxel", "0.05,1,2,3"],
                ["--voxel", "0.05,nan,2"], ["--voxel", "0.05,1,nan"], ["--voxel", ",1,2"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--voxel needs" in r.stdout and "Image Loading" not in r.stdout, (bad, r.stdout)
    r = subprocess.run(base[:6] + ["--voxel", "0.05"], capture_output=True, text=True, timeout=120)  # (without --calib)
    assert r.returncode != 0 and "--voxel refused: it needs --calib" in r.stdout and "Image Loading" not in r.stdout
    for good in ("0.05", "0.05,0.5,20", "1e-2,0,inf"):
        r = subprocess.run(base + ["--voxel", good], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Image Loading" in r.stdout and "--voxel" not in r.stdout, (good, r.stdout)  # (well-formed: gets as far as the images)
