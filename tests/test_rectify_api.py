"""CPU tier of the rectification: tests/rectify_ref.py (the definition the GPU tests hold the kernels to) against scalar loops written
from the definition word for word, and the new surface of the C ABI, the Python mirror, the facade and the CLI -- declared, exported,
NULL-handle / bad-argument returns, a malformed --rectify refused before an image is loaded, the sanitizer build."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import rectify_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
HANDLE_ENTRY_POINTS = ["adc_set_rectify_maps", "adc_set_rectify_model", "adc_clear_rectify", "adc_get_rectify_maps", "adc_rectify_device"]
FARM_ENTRY_POINTS = ["adc_farm_set_rectify_maps", "adc_farm_set_rectify_model", "adc_farm_clear_rectify"]
F = np.float32


def brute_remap(src, ws, hs, pitch, fmt, mx, my):
    """The definition, one destination pixel and one tap at a time, on the raw bytes."""
    s = np.ascontiguousarray(src, np.uint8).reshape(-1)
    H, W = mx.shape
    out, valid = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8)
    bpp = RR.BPP[fmt]

    def pixel(y, x):
        p = s[y * pitch + x * bpp: y * pitch + x * bpp + bpp]
        if fmt == RR.GRAY8:
            return int(p[0]), int(p[0]), int(p[0])
        if fmt == RR.RGB8:
            return int(p[2]), int(p[1]), int(p[0])
        return int(p[0]), int(p[1]), int(p[2])

    for v in range(H):
        for u in range(W):
            fx, fy = F(mx[v, u]), F(my[v, u])
            if not (abs(fx) < F(32768.0)) or not (abs(fy) < F(32768.0)):
                continue
            X, Y = int(np.rint(F(fx * F(32.0)))), int(np.rint(F(fy * F(32.0))))
            xi, ax, yi, ay = X >> 5, X & 31, Y >> 5, Y & 31  # (Python's >> on a negative int is arithmetic)
            acc, ok = [0, 0, 0], True
            for ty, tx, w in ((yi, xi, (32 - ax) * (32 - ay)), (yi, xi + 1, ax * (32 - ay)), (yi + 1, xi, (32 - ax) * ay), (yi + 1, xi + 1, ax * ay)):
                inside = 0 <= tx < ws and 0 <= ty < hs
                if inside:
                    for c, p in enumerate(pixel(ty, tx)):
                        acc[c] += w * p
                elif w != 0:
                    ok = False
            out[v, u] = [(a + 512) >> 10 for a in acc]
            valid[v, u] = 1 if ok else 0
    return out, valid


def _random_case(rng, fmt):
    ws, hs = int(rng.integers(1, 23)), int(rng.integers(1, 17))
    W, H = int(rng.integers(1, 29)), int(rng.integers(1, 13))
    pitch = ws * RR.BPP[fmt] + int(rng.choice([0, 0, 1, 5, 16]))
    src = rng.integers(0, 256, (hs, pitch), dtype=np.uint8)
    kind = int(rng.integers(0, 4))
    if kind == 0:  # anywhere around the image, fractional
        mx = (rng.random((H, W)) * (ws + 6) - 3).astype(F)
        my = (rng.random((H, W)) * (hs + 6) - 3).astype(F)
    elif kind == 1:  # on the 1/32 grid and on its ties (x.5 / 32)
        mx = (rng.integers(-64, 32 * ws + 64, (H, W)) / 32.0 + rng.choice([0.0, 1.0 / 64.0], (H, W))).astype(F)
        my = (rng.integers(-64, 32 * hs + 64, (H, W)) / 32.0 + rng.choice([0.0, 1.0 / 64.0], (H, W))).astype(F)
    elif kind == 2:  # integer coordinates, the last row / column included
        mx = rng.integers(-2, ws + 2, (H, W)).astype(F)
        my = rng.integers(-2, hs + 2, (H, W)).astype(F)
    else:
        mx = (rng.random((H, W)) * ws).astype(F)
        my = (rng.random((H, W)) * hs).astype(F)
    for m in (mx, my):
        salt = rng.random((H, W))
        m[salt < 0.03] = np.nan
        m[(salt >= 0.03) & (salt < 0.05)] = np.inf
        m[(salt >= 0.05) & (salt < 0.07)] = -np.inf
        m[(salt >= 0.07) & (salt < 0.09)] = F(rng.choice([32768.0, -32768.0, 32767.99, -32767.99, 1e30, -3e38, 40000.5]))
    return src, ws, hs, pitch, mx, my


@pytest.mark.parametrize("fmt", [RR.BGR8, RR.RGB8, RR.GRAY8, RR.BGRA8])
def test_remap_against_the_scalar_definition(fmt):
    rng = np.random.default_rng(100 + fmt)
    for t in range(30):
        src, ws, hs, pitch, mx, my = _random_case(rng, fmt)
        got, want = RR.remap(src, ws, hs, pitch, fmt, mx, my), brute_remap(src, ws, hs, pitch, fmt, mx, my)
        assert np.array_equal(got[0], want[0]), "case %d: image" % t
        assert np.array_equal(got[1], want[1]), "case %d: valid" % t


def test_last_row_and_column_are_valid_with_zero_fraction():
    ws, hs = 7, 5
    src = np.random.default_rng(3).integers(0, 256, (hs, ws * 3), dtype=np.uint8)
    mx = np.array([[ws - 1, ws - 1, ws - 1 + 1 / 32.0, 0, -1 / 32.0, ws]], F)
    my = np.array([[hs - 1, hs - 1 + 1 / 32.0, hs - 1, 0, 0, 0]], F)
    out, valid = RR.remap(src, ws, hs, ws * 3, RR.BGR8, mx, my)
    assert valid.tolist() == [[1, 0, 0, 1, 0, 0]]
    img = src.reshape(hs, ws, 3)
    assert np.array_equal(out[0, 0], img[hs - 1, ws - 1]) and np.array_equal(out[0, 3], img[0, 0]) and not out[0, 5].any()
    b = brute_remap(src, ws, hs, ws * 3, RR.BGR8, mx, my)
    assert np.array_equal(out, b[0]) and np.array_equal(valid, b[1])


def test_identity_model_reproduces_the_image():
    rng = np.random.default_rng(7)
    for (w, h) in ((64, 40), (333, 57)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        mx, my = RR.model_maps(RR.identity_model(cx=w / 2.0, cy=h / 2.0, f=1000.0), w, h)
        out, valid = RR.remap(img, w, h, w * 3, RR.BGR8, mx, my)
        assert np.array_equal(out, img) and valid.all()
    w, h = 1920, 1080  # the maps are the pixel grid exactly
    mx, my = RR.model_maps(RR.identity_model(cx=w / 2.0, cy=h / 2.0, f=1734.0), w, h)
    _, xi, ax, yi, ay = RR.quantise(mx, my)
    assert np.array_equal(xi, np.broadcast_to(np.arange(w), (h, w))) and np.array_equal(yi, np.broadcast_to(np.arange(h)[:, None], (h, w)))
    assert not ax.any() and not ay.any()


def test_integer_shift_gives_a_shifted_image_with_a_zero_border():
    rng = np.random.default_rng(8)
    w, h, dx, dy = 50, 30, 7, -4
    img = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
    mx = np.broadcast_to(np.arange(w, dtype=F) + F(dx), (h, w)).copy()
    my = np.broadcast_to((np.arange(h, dtype=F) + F(dy))[:, None], (h, w)).copy()
    out, valid = RR.remap(img, w, h, w * 3, RR.BGR8, mx, my)
    want, wv = np.zeros_like(img), np.zeros((h, w), np.uint8)
    want[-dy:, :w - dx] = img[:h + dy, dx:]
    wv[-dy:, :w - dx] = 1
    assert np.array_equal(out, want) and np.array_equal(valid, wv)


def test_example_model_figures():
    """Most pixels of the example model are valid and have fractional taps (the hot kernel's general case)."""
    ws, hs, W, H = 480, 270, 480, 270
    mx, my = RR.model_maps(RR.example_model(ws, hs, W, H), W, H)
    outside, xi, ax, yi, ay = RR.quantise(mx, my)
    _, valid = RR.remap(np.zeros((hs, ws * 3), np.uint8), ws, hs, ws * 3, RR.BGR8, mx, my)
    print("valid %.2f %%, fractional %.2f %%" % (100.0 * valid.mean(), 100.0 * ((ax != 0) | (ay != 0)).mean()))
    assert valid.mean() > 0.9 and ((ax != 0) | (ay != 0)).mean() > 0.9 and not outside.any()


def test_model_maps_against_a_scalar_float32_loop():
    W, H = 37, 23
    for model in (RR.example_model(64, 48, W, H), RR.second_model(64, 48, W, H), RR.identity_model(3.0, 2.0, 50.0)):
        g = {k: F(v) for k, v in model.items() if k != "R"}
        R = [F(v) for v in model["R"]]
        mx, my = RR.model_maps(model, W, H)
        one, two = F(1), F(2)
        for v in range(H):
            for u in range(W):
                xn = F(F(F(u) - g["new_cx"]) / g["new_fx"])
                yn = F(F(F(v) - g["new_cy"]) / g["new_fy"])
                X = F(F(F(R[0] * xn) + F(R[3] * yn)) + R[6])
                Y = F(F(F(R[1] * xn) + F(R[4] * yn)) + R[7])
                Wc = F(F(F(R[2] * xn) + F(R[5] * yn)) + R[8])
                x, y = F(X / Wc), F(Y / Wc)
                x2, y2 = F(x * x), F(y * y)
                r2, xy = F(x2 + y2), F(x * y)
                rad = F(one + F(r2 * F(g["k1"] + F(r2 * F(g["k2"] + F(r2 * g["k3"]))))))
                xd = F(F(F(x * rad) + F(F(two * g["p1"]) * xy)) + F(g["p2"] * F(r2 + F(two * x2))))
                yd = F(F(F(y * rad) + F(g["p1"] * F(r2 + F(two * y2)))) + F(F(two * g["p2"]) * xy))
                wx, wy = F(F(g["fx"] * xd) + g["cx"]), F(F(g["fy"] * yd) + g["cy"])
                assert wx.tobytes() == mx[v, u].tobytes() and wy.tobytes() == my[v, u].tobytes(), (u, v)


def test_pack_source_round_trip():
    img = np.random.default_rng(9).integers(0, 256, (6, 11, 3), dtype=np.uint8)
    for fmt in (RR.BGR8, RR.RGB8, RR.BGRA8):
        raw = RR.pack_source(img, fmt, 11 * RR.BPP[fmt] + 3)
        assert np.array_equal(RR.source_bgr(raw, 11, 6, raw.shape[1], fmt), img)
    raw = RR.pack_source(img, RR.GRAY8, 16)
    assert np.array_equal(RR.source_bgr(raw, 11, 6, 16, RR.GRAY8), np.repeat(img[:, :, :1], 3, 2))


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    for name in HANDLE_ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    for name in FARM_ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_farm\s*\*" % name, text), name
    for name, value in (("ADC_PIX_BGR8", 0), ("ADC_PIX_RGB8", 1), ("ADC_PIX_GRAY8", 2), ("ADC_PIX_BGRA8", 3), ("ADC_SIDE_LEFT", 0), ("ADC_SIDE_RIGHT", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert (A.PIX_BGR8, A.PIX_RGB8, A.PIX_GRAY8, A.PIX_BGRA8, A.SIDE_LEFT, A.SIDE_RIGHT) == (0, 1, 2, 3, 0, 1)
    assert "typedef struct adc_raw_format" in text and "typedef struct adc_camera_model" in text
    assert C.sizeof(A.RawFormat) == 16 and C.sizeof(A.CameraModel) == 22 * 4
    out = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(HANDLE_ENTRY_POINTS + FARM_ENTRY_POINTS) <= names


def test_null_handle_and_bad_arguments_are_refused():
    """No device is needed: every refusal comes before the first HIP call and before the handle is looked at, so a zeroed block
    stands in for a handle in the bad-argument cases (the GPU tier repeats them on a real one, with the message)."""
    L = A.lib()
    raw = A.RawFormat(8, 4, 0, A.PIX_BGR8)
    model = A.CameraModel(fx=1, fy=1, new_fx=1, new_fy=1)
    m = np.zeros((4, 8), F)
    assert L.adc_set_rectify_maps(None, 0, C.byref(raw), m.ctypes.data, m.ctypes.data) == 1
    assert L.adc_set_rectify_model(None, 0, C.byref(raw), C.byref(model)) == 1
    assert L.adc_clear_rectify(None) == 1
    assert L.adc_get_rectify_maps(None, 0, m.ctypes.data, m.ctypes.data, None) == 1
    assert L.adc_rectify_device(None, 0, C.c_void_p(16), C.c_void_p(32)) == 1
    assert L.adc_farm_set_rectify_maps(None, 0, C.byref(raw), m.ctypes.data, m.ctypes.data) == 1
    assert L.adc_farm_set_rectify_model(None, 0, C.byref(raw), C.byref(model)) == 1
    assert L.adc_farm_clear_rectify(None) == 1
    fake = C.create_string_buffer(1 << 20)
    h, mp = C.cast(fake, C.c_void_p), m.ctypes.data
    for side in (-1, 2, 7):
        assert L.adc_set_rectify_maps(h, side, C.byref(raw), mp, mp) == 1 and L.adc_set_rectify_model(h, side, C.byref(raw), C.byref(model)) == 1
        assert L.adc_get_rectify_maps(h, side, mp, mp, None) == 1 and L.adc_rectify_device(h, side, C.c_void_p(16), C.c_void_p(32)) == 1
    assert L.adc_set_rectify_maps(h, 0, None, mp, mp) == 1 and L.adc_set_rectify_maps(h, 0, C.byref(raw), None, mp) == 1
    assert L.adc_set_rectify_maps(h, 0, C.byref(raw), mp, None) == 1 and L.adc_set_rectify_model(h, 0, None, C.byref(model)) == 1
    assert L.adc_set_rectify_model(h, 0, C.byref(raw), None) == 1
    assert L.adc_rectify_device(h, 0, None, C.c_void_p(32)) == 1 and L.adc_rectify_device(h, 0, C.c_void_p(16), None) == 1
    assert L.adc_get_rectify_maps(h, 0, mp, mp, None) == 1 and L.adc_rectify_device(h, 0, C.c_void_p(16), C.c_void_p(32)) == 1  # (side not set)
    bad_formats = [A.RawFormat(8, 4, 24, 4), A.RawFormat(8, 4, 24, -1), A.RawFormat(0, 4, 24, 0), A.RawFormat(8, 0, 24, 0), A.RawFormat(-3, 4, 24, 0),
                   A.RawFormat(32768, 4, 32768 * 3, 0), A.RawFormat(8, 32768, 24, 0), A.RawFormat(8, 4, 23, 0), A.RawFormat(8, 4, 31, 3),
                   A.RawFormat(8, 4, 7, 2), A.RawFormat(8, 4, -24, 0), A.RawFormat(30000, 30000, 90000, 0)]
    for bad in bad_formats:
        assert L.adc_set_rectify_maps(h, 0, C.byref(bad), mp, mp) == 1, (bad.width, bad.height, bad.pitch_bytes, bad.format)
        assert L.adc_set_rectify_model(h, 0, C.byref(bad), C.byref(model)) == 1 and A.last_error().startswith("adc_set_rectify_model")
    for key, value in (("fx", 0.0), ("fy", 0.0), ("new_fx", 0.0), ("new_fy", -0.0), ("k1", float("nan")), ("cx", float("inf")), ("new_cy", float("-inf")),
                       ("R", [1, 0, 0, 0, float("nan"), 0, 0, 0, 1])):
        bad = A.CameraModel(fx=1, fy=1, new_fx=1, new_fy=1)
        setattr(bad, key, (C.c_float * 9)(*value) if key == "R" else value)
        assert L.adc_set_rectify_model(h, 1, C.byref(raw), C.byref(bad)) == 1 and "finite" in A.last_error(), key
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    st.width, st.height = 8, 4
    with pytest.raises(RuntimeError):
        st.set_rectify_maps(A.SIDE_LEFT, raw, m, m)
    with pytest.raises(RuntimeError):
        st.set_rectify_model(A.SIDE_LEFT, raw, model)
    with pytest.raises(RuntimeError):
        st.clear_rectify()
    with pytest.raises(RuntimeError):
        st.rectify_maps(A.SIDE_LEFT)
    assert st.rectify_device(A.SIDE_LEFT, 16, 32) is False


def test_python_mirror_signatures():
    def params(f):
        return list(inspect.signature(f).parameters)
    for cls in (A.ADCensusStereo, A.PairFarm):
        assert params(cls.set_rectify_maps) == ["self", "side", "raw", "map_x", "map_y"]
        assert params(cls.set_rectify_model) == ["self", "side", "raw", "model"]
        assert params(cls.clear_rectify) == ["self"]
    assert params(A.ADCensusStereo.rectify_maps) == ["self", "side"]
    assert params(A.ADCensusStereo.rectify_device) == ["self", "side", "d_raw", "d_bgr_out"]
    assert params(A.ADCensusStereo.rectify) == ["self", "raw", "side"]
    L = A.lib()
    vp = C.c_void_p
    for prefix in ("adc_", "adc_farm_"):
        assert getattr(L, prefix + "set_rectify_maps").argtypes == [vp, C.c_int, C.POINTER(A.RawFormat), vp, vp]
        assert getattr(L, prefix + "set_rectify_model").argtypes == [vp, C.c_int, C.POINTER(A.RawFormat), C.POINTER(A.CameraModel)]
        assert getattr(L, prefix + "clear_rectify").argtypes == [vp]
    assert L.adc_get_rectify_maps.argtypes == [vp, C.c_int, vp, vp, vp] and L.adc_rectify_device.argtypes == [vp, C.c_int, vp, vp]
    r = A.RawFormat(10, 4, 0, A.PIX_BGRA8)
    assert (r.pitch_bytes, r.nbytes) == (40, 160) and A.RawFormat(10, 4, 48, A.PIX_GRAY8).nbytes == 192
    m = A.CameraModel(fx=2.5, R=range(9), new_cy=-1)
    assert (m.fx, list(m.R), m.new_cy, m.k1) == (2.5, [float(i) for i in range(9)], -1.0, 0.0)
    assert list(A.CameraModel().R) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    with pytest.raises(AttributeError):
        A.CameraModel(k4=1.0)
    # the size asserts of the entry points follow the raw geometry
    s = A._RectifyState()
    assert s.sizes(300) == (300, 300)
    s.set(0, A.RawFormat(10, 4, 0, A.PIX_BGRA8))
    assert not s.on() and s.sizes(300) == (300, 300)
    s.set(1, A.RawFormat(9, 5, 16, A.PIX_GRAY8))
    assert s.on() and s.sizes(300) == (160, 80)
    s.clear()
    assert s.sizes(300) == (300, 300)


CALLER = r'''
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
int main() {
    ADCensusStereo s; ADCensusOption o;
    adc_raw_format raw = {8, 4, 24, ADC_PIX_BGR8}, bad = {8, 4, 23, ADC_PIX_BGR8};
    adc_camera_model m = {100.f, 100.f, 4.f, 2.f, 0.f, 0.f, 0.f, 0.f, 0.f, {1, 0, 0, 0, 1, 0, 0, 0, 1}, 100.f, 100.f, 4.f, 2.f}, zero = m;
    zero.new_fx = 0.f;
    float32 mx[32] = {0}, my[32] = {0};
    uint8 img[96] = {0};
    bool ok = s.SetRectifyModel(ADC_SIDE_LEFT, &raw, &m) && s.SetRectifyMaps(ADC_SIDE_RIGHT, &raw, mx, my, 8, 4);
    ok = ok && !s.SetRectifyModel(2, &raw, &m) && !s.SetRectifyModel(ADC_SIDE_LEFT, &bad, &m) && !s.SetRectifyModel(ADC_SIDE_LEFT, &raw, &zero);
    ok = ok && !s.SetRectifyMaps(ADC_SIDE_LEFT, &raw, nullptr, my, 8, 4) && !s.SetRectifyMaps(ADC_SIDE_LEFT, &raw, mx, my, 0, 4);
    ok = ok && !s.Rectify(ADC_SIDE_LEFT, img, img) && s.ClearRectify();
    return (ok && !s.Match(img, img, mx) && !s.Initialize(0, 0, o)) ? 0 : 1;
}
'''


def test_facade_compiles_and_exports_the_members(tmp_path):
    """A caller of the facade's new members compiles against include/ alone and links against the facade library; before Initialize
    the setters only check and remember, so the program runs without a device."""
    src = tmp_path / "caller.cpp"
    src.write_text(CALLER)
    libdir = os.path.join(ROOT, "adcensus_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libadcensus.so")):
        pytest.fail("libadcensus.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "caller"),
                    "-L", libdir, "-ladcensus", "-ladcensus_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(libdir, "libadcensus.so")], capture_output=True, text=True, check=True).stdout
    assert "ADCensusStereo::SetRectifyMaps(int, adc_raw_format const*, float const*, float const*, int, int)" in out
    assert "ADCensusStereo::SetRectifyModel(int, adc_raw_format const*, adc_camera_model const*)" in out
    assert "ADCensusStereo::ClearRectify()" in out
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def camera_file(path, raw, model, extra="", drop=(), rect=None):
    """Writes one --rectify camera file; `drop`: keys to leave out, `extra`: lines appended."""
    fmt = {0: "BGR8", 1: "RGB8", 2: "GRAY8", 3: "BGRA8"}[raw[3]]
    kv = [("width", raw[0]), ("height", raw[1]), ("pitch", raw[2]), ("format", fmt)]
    kv += [(k, repr(float(model[k]))) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]
    kv += [("R", " ".join(repr(float(v)) for v in model["R"]))]
    kv += [(k, repr(float(model[k]))) for k in ("new_fx", "new_fy", "new_cx", "new_cy")]
    if rect:
        kv += [("rect_width", rect[0]), ("rect_height", rect[1])]
    with open(path, "w") as f:
        f.write("# one camera\n")
        for k, v in kv:
            if k not in drop:
                f.write("%s = %s\n" % (k, v))
        f.write(extra)
    return str(path)


def test_cli_rejects_malformed_rectify_flags_and_files(tmp_path):
    """Checked while the arguments are parsed: the images named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    model = RR.example_model(45, 31, 45, 31)
    good = camera_file(tmp_path / "good.txt", (45, 31, 45 * 3, 0), model)
    bad_files = {
        "missing": camera_file(tmp_path / "b1.txt", (45, 31, 135, 0), model, drop=("k3",)),
        "twice": camera_file(tmp_path / "b2.txt", (45, 31, 135, 0), model, extra="fx = 3\n"),
        "unknown": camera_file(tmp_path / "b3.txt", (45, 31, 135, 0), model, extra="k4 = 0\n"),
        "pitch": camera_file(tmp_path / "b4.txt", (45, 31, 134, 0), model),
        "nan": camera_file(tmp_path / "b5.txt", (45, 31, 135, 0), dict(model, k1=float("nan"))),
        "zero": camera_file(tmp_path / "b6.txt", (45, 31, 135, 0), dict(model, new_fy=0.0)),
        "r8": camera_file(tmp_path / "b7.txt", (45, 31, 135, 0), dict(model, R=model["R"][:8])),
        "noeq": camera_file(tmp_path / "b8.txt", (45, 31, 135, 0), model, extra="just words\n"),
        "tail": camera_file(tmp_path / "b9.txt", (45, 31, 135, 0), model, drop=("cx",), extra="cx = 3.5x\n"),
        "size": camera_file(tmp_path / "b10.txt", (45, 31, 135, 0), model, rect=(40, 30)),
        "width": camera_file(tmp_path / "b11.txt", (40000, 31, 120000, 0), model),
    }
    flags = [["--rectify"], ["--rectify", good], ["--rectify", good + ","], ["--rectify", "," + good], ["--rectify", good + "," + good + "," + good],
             ["--rectify", good + "," + str(tmp_path / "absent.txt")]]
    flags += [["--rectify", good + "," + b] for b in bad_files.values()] + [["--rectify", bad_files["missing"] + "," + good]]
    for bad in flags:
        r = subprocess.run([cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "0", "64", str(tmp_path / "out")] + bad,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--rectify refused" in r.stdout and "Image Loading" not in r.stdout, (bad, r.stdout)
    r = subprocess.run([cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "--rectify", good + "," + good], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Image Loading" in r.stdout and "--rectify refused" not in r.stdout  # (well-formed: gets as far as the images)


def test_cli_rectify_under_sanitizers(tmp_path):
    """The flag's parsing, the repacking of the loaded pixels and the facade's members in the ASAN / UBSAN build on the stub C ABI
    (which checks the arguments and copies nothing): runs with the flag complete cleanly and write the two extra images."""
    from PIL import Image
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "adcensus_amd", "host"), "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cli = os.path.join(ROOT, "adcensus_amd", "build", "asan", "adcensus_cli_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    rgb = np.random.default_rng(5).integers(0, 256, (31, 45, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "l.png")
    Image.fromarray(rgb[:, ::-1].copy()).save(tmp_path / "r.png")
    model = RR.example_model(45, 31, 45, 31)
    left = camera_file(tmp_path / "left.txt", (45, 31, 45 * 3 + 5, 0), model)
    right = camera_file(tmp_path / "right.txt", (45, 31, 45 * 4, 3), model)
    rgbf = camera_file(tmp_path / "rgb.txt", (45, 31, 45 * 3, 1), model, rect=(40, 30))

    def run(*extra):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "0", "16", *extra], env=env, capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        return r

    assert run(str(tmp_path / "plain")).returncode == 0
    assert run("--rectify", left + "," + right, str(tmp_path / "rect")).returncode == 0
    assert run(str(tmp_path / "rect2"), "--rectify", rgbf + "," + rgbf, "--speckle", "7,0", "--calib", "100,0.5,0,0,0").returncode == 0
    for pref, size in (("rect", (45, 31)), ("rect2", (40, 30))):
        for side in ("left", "right"):
            assert Image.open(str(tmp_path / pref) + "-rect-%s.png" % side).size == size
        assert os.path.exists(str(tmp_path / pref) + ".pfm")
    assert not os.path.exists(str(tmp_path / "plain") + "-rect-left.png")
    bad = camera_file(tmp_path / "bad.txt", (45, 31, 45 * 3, 0), dict(model, fx=math.inf))
    assert run(str(tmp_path / "bad"), "--rectify", left + "," + bad).returncode != 0 and not os.path.exists(str(tmp_path / "bad") + ".pfm")
    wrong = camera_file(tmp_path / "wrong.txt", (44, 31, 44 * 3, 0), model, rect=(45, 31))  # (not the size of the image)
    assert run(str(tmp_path / "wrong"), "--rectify", left + "," + wrong).returncode != 0 and not os.path.exists(str(tmp_path / "wrong") + ".pfm")


def test_integration_caller_compiles_as_printed(tmp_path):
    """The complete caller of INTEGRATION.md's rectification section compiles against include/ alone and links."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = text.index("/* cc caller.c -Iinclude")
    src = tmp_path / "caller.c"
    src.write_text(text[start:text.index("```", start)])
    libdir = os.path.join(ROOT, "adcensus_amd", "lib")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "caller"),
                    "-L", libdir, "-ladcensus_hip", "-Wl,-rpath," + libdir], check=True)
