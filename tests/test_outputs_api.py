"""CPU tier: the depth / point cloud / 8-bit image surface of the C ABI (adc_match_out, adc_match_device_out, adc_reproject_device,
adc_get_cloud_count) -- declared, exported, the same struct layouts in the header and in the Python mirror, the NULL-handle
contract -- the rules of tests/outputs_ref.py on hand-made maps (the definition the GPU tests compare the kernels with), and the
CLI's --calib writers under ASAN / UBSAN against the stub C ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import outputs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
ENTRY_POINTS = ["adc_match_out", "adc_match_device_out", "adc_reproject_device", "adc_get_cloud_count"]
F = np.float32
INF = F(np.inf)


def _header():
    with open(HEADER) as f:
        return f.read()


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = _header()
    for name in ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    out = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= names
    # sizeof(adc_point) == 16, asked of a C compiler
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(adc_point), offsetof(adc_point, z), offsetof(adc_point, r),\n'
                   ' offsetof(adc_point, pad), sizeof(adc_calib), sizeof(adc_outputs), offsetof(adc_outputs, depth), offsetof(adc_outputs, cloud_capacity),\n'
                   ' offsetof(adc_outputs, cloud_count), offsetof(adc_outputs, disp8)); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 16
    # the Python mirror's layouts equal the header's
    assert got == [C.sizeof(A.Point), A.Point.z.offset, A.Point.r.offset, A.Point.pad.offset, C.sizeof(A.Calib), C.sizeof(A.Outputs),
                   A.Outputs.depth.offset, A.Outputs.cloud_capacity.offset, A.Outputs.cloud_count.offset, A.Outputs.disp8.offset]
    assert A.POINT_DTYPE == outputs_ref.POINT_DTYPE and A.POINT_DTYPE.itemsize == 16
    assert [A.POINT_DTYPE.fields[n][1] for n in ("x", "y", "z", "r", "g", "b", "pad")] == [0, 4, 8, 12, 13, 14, 15]
    assert [f[0] for f in A.Calib._fields_] == re.search(r"typedef struct adc_calib \{\s*float ([^;]+);", text).group(1).replace(" ", "").split(",")


def test_null_handle_is_refused():
    L = A.lib()
    img = np.zeros(12, np.uint8)
    disp = np.zeros(4, np.float32)
    g = np.zeros(4, np.uint8)
    req = A.Outputs(None, None, None, 0, None, g.ctypes.data)
    assert L.adc_match_out(None, img.ctypes.data, img.ctypes.data, disp.ctypes.data, C.byref(req)) == 1
    assert L.adc_match_out(None, img.ctypes.data, img.ctypes.data, disp.ctypes.data, None) == 1
    assert L.adc_match_device_out(None, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.byref(req)) == 1
    assert L.adc_match_device_out(None, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), None) == 1
    assert L.adc_reproject_device(None, C.c_void_p(16), C.c_void_p(16), C.byref(req)) == 1
    n = C.c_uint64(7)
    assert L.adc_get_cloud_count(None, C.byref(n)) == 1 and n.value == 7
    st = A.ADCensusStereo()
    assert st.MatchOut(img, img, disp, disp8=g) is False  # (not initialised)


def _img(h, w, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_all_invalid_and_constant_maps():
    img = _img(3, 5)
    d = np.full((3, 5), INF, F)
    assert len(outputs_ref.cloud(d, img)) == 0 and len(outputs_ref.cloud(d, img, (100, 0.5, 2, 1, 0))) == 0
    assert not outputs_ref.disp8(d).any()
    assert np.all(outputs_ref.depth(d, (100, 0.5, 2, 1, 0))[0] == INF)
    d = np.full((3, 5), 3.25, F)  # (below W: mn starts from float(W))
    assert not outputs_ref.disp8(d).any()  # mx == mn: the reference divides 0 by 0, the project writes 0
    assert len(outputs_ref.cloud(d, img)) == 15
    d[1, 2] = INF  # a hole does not change that
    assert not outputs_ref.disp8(d).any() and len(outputs_ref.cloud(d, img)) == 14
    # one valid pixel among holes: a constant map again
    d = np.full((3, 5), INF, F)
    d[2, 4] = 3
    assert not outputs_ref.disp8(d).any() and len(outputs_ref.cloud(d, img)) == 1


def test_disp8_formula_and_magnitudes():
    d = np.array([[-8.0, 2.0, INF, 4.5, -0.0]], F)
    g = outputs_ref.disp8(d)
    a = np.abs(d[np.isfinite(d)])
    assert g.tolist() == [[255, int(F(2) / F(8) * F(255)), 0, int(F(4.5) / F(8) * F(255)), 0]]  # the cast truncates
    assert np.array_equal(outputs_ref.disp8(-d), g) and np.array_equal(outputs_ref.disp8(np.abs(d)), g)
    # min / max start from W and -W: a map whose valid values all exceed W keeps mn = W
    d = np.array([[10.0, 20.0, 30.0]], F)
    assert outputs_ref.disp8(d).tolist() == [[int((F(10) - F(3)) / (F(30) - F(3)) * F(255)), int((F(20) - F(3)) / F(27) * F(255)), 255]]
    assert a.min() == 0


def test_depth_and_cloud_rules():
    img = _img(2, 3)
    d = np.array([[-4.0, 0.0, INF], [2.0, 0.5, -1.0]], F)
    cal = (3740, 0.16, 1.5, 0.5, 0)
    fb = F(3740) * F(0.16)
    z, valid = outputs_ref.depth(d, cal)
    assert valid.tolist() == [[True, False, False], [True, True, True]]  # |d| + doffs <= 0 and +inf are invalid
    assert _u32(z).tolist() == _u32([[fb / F(4), INF, INF], [fb / F(2), fb / F(0.5), fb / F(1)]]).tolist()
    # the uncalibrated cloud keeps the zero (the reference's rows), the calibrated one drops it; raster order; colours swapped
    pts = outputs_ref.cloud(d, img)
    assert [(p["x"], p["y"], p["z"]) for p in pts] == [(0, 0, 4), (1, 0, 0), (0, 1, 2), (1, 1, 0.5), (2, 1, 1)]
    assert [(p["r"], p["g"], p["b"]) for p in pts] == [tuple(img[y, x, ::-1]) for y, x in ((0, 0), (0, 1), (1, 0), (1, 1), (1, 2))]
    assert not pts["pad"].any() and pts.tobytes()[15::16] == b"\0" * 5
    cp = outputs_ref.cloud(d, img, cal)
    assert len(cp) == 4 and _u32(cp["z"]).tolist() == _u32(z[valid]).tolist()
    assert _u32(cp["x"][0]) == _u32((F(0) - F(1.5)) * (fb / F(4)) / F(3740)) and _u32(cp["y"][3]) == _u32((F(1) - F(0.5)) * (fb / F(1)) / F(3740))
    # doffs moves the validity: negative doffs drops |d| <= -doffs, positive doffs admits the zero
    assert outputs_ref.depth(d, (3740, 0.16, 0, 0, -1))[1].tolist() == [[True, False, False], [True, False, False]]
    assert outputs_ref.depth(d, (3740, 0.16, 0, 0, 0.25))[1].tolist() == [[True, True, False], [True, True, True]]
    assert len(outputs_ref.cloud(d, img, (3740, 0.16, 0, 0, -1))) == 2


def test_one_ulp_apart():
    one = F(1)
    up = one + np.spacing(one)
    d = np.array([[one, up, F(3)]], F)
    cal = (F(1) / F(3), 1.0, 0, 0, 0)
    z = outputs_ref.depth(d, cal)[0]
    fb = F(F(1) / F(3)) * F(1)
    assert _u32(z)[0, 0] != _u32(z)[0, 1] and _u32(z).tolist() == [_u32([fb / one, fb / up, fb / F(3)]).tolist()]
    pts = outputs_ref.cloud(d, _img(1, 3), cal)
    assert _u32(pts["x"][2]) == _u32((F(2) * (fb / F(3))) / F(F(1) / F(3)))
    # f32 throughout: the same expression in double rounds differently somewhere on a ramp
    ramp = (np.arange(1, 2000, dtype=F) / F(7)).reshape(1, -1)
    z32 = outputs_ref.depth(ramp, (3740, 0.16, 0, 0, 0.1))[0]
    z64 = (np.float64(F(3740) * F(0.16)) / (ramp.astype(np.float64) + np.float64(F(0.1)))).astype(F)
    assert (_u32(z32) != _u32(z64)).any()


@pytest.fixture(scope="module")
def cli_asan():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "adcensus_amd", "host"), "asan"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("make asan failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    return os.path.join(ROOT, "adcensus_amd", "build", "asan", "adcensus_cli_asan")


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = (int(v) for v in f.readline().split())
        f.readline()
        return np.ascontiguousarray(np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1])


def read_ply(path):
    """(vertex count of the header, payload as an array of x y z f4 + red green blue u1 rows)"""
    raw = open(path, "rb").read()
    head, payload = raw.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    assert lines[3:] == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue"]
    n = int(re.fullmatch(r"element vertex (\d+)", lines[2]).group(1))
    rows = np.frombuffer(payload, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")]))
    return n, rows


def test_cli_calib_under_sanitizers(cli_asan, tmp_path):
    from PIL import Image
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    w, h = 83, 57
    rgb = _img(h, w, 5)
    Image.fromarray(rgb).save(tmp_path / "l.png")
    Image.fromarray(rgb[:, ::-1].copy()).save(tmp_path / "r.png")

    def run(*extra):
        r = subprocess.run([cli_asan, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "-3", "29", *extra], env=env, capture_output=True,
                           text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        return r

    assert run(str(tmp_path / "plain")).returncode == 0
    assert run(str(tmp_path / "cal"), "--calib", "3740,0.16,41.5,28.5,0.5").returncode == 0
    assert run("--calib", "100,0.5,0,0,-2", str(tmp_path / "cal2")).returncode == 0  # (the flag may stand anywhere)
    for suffix in ("-d.png", "-c.png", "-cloud.txt", ".pfm"):  # the existing outputs do not change with the flag
        assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / "cal") + suffix, "rb").read(), suffix
    assert not os.path.exists(str(tmp_path / "plain") + "-depth.pfm") and not os.path.exists(str(tmp_path / "plain") + "-cloud.ply")
    disp = read_pfm(str(tmp_path / "plain") + ".pfm")
    assert np.isinf(disp).any() and (disp < 0).any()  # (the stub's map has holes and negative values)
    bgr = rgb[:, :, ::-1]
    for pref, cal in (("cal", (3740, 0.16, 41.5, 28.5, 0.5)), ("cal2", (100, 0.5, 0, 0, -2))):
        want_z, want_pts, _ = outputs_ref.outputs(disp, bgr, cal)
        assert np.array_equal(_u32(read_pfm(str(tmp_path / pref) + "-depth.pfm")), _u32(want_z))
        n, rows = read_ply(str(tmp_path / pref) + "-cloud.ply")
        assert n == len(want_pts) == len(rows) and 0 < n < w * h
        for name in ("x", "y", "z"):
            assert np.array_equal(_u32(rows[name]), _u32(want_pts[name])), name
        assert all(np.array_equal(rows[c], want_pts[c]) for c in "rgb")
    # refusals of the flag itself
    assert run(str(tmp_path / "bad"), "--calib", "1,2,3").returncode != 0
    assert run(str(tmp_path / "bad"), "--calib", "0,1,0,0,0").returncode != 0  # (focal_px <= 0: MatchOut refuses)
    assert run(str(tmp_path / "bad"), "--calib", "1,1,0,0,0", "--extras").returncode != 0
