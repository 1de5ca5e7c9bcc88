"""CPU tier of the camera layouts: tests/rawfmt_ref.py (the definition the GPU tests hold the kernels to) against scalar loops written
from the formulas word for word and against the properties the formulas imply, and the new surface of the C ABI, the Python mirror, the
facade and the CLI -- declared, exported, every argument rule refused without a device, --raw parsed, the sanitizer build."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import rawfmt_ref as RF
from tests import rectify_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
F = np.float32
CONSTANTS = {"GRAY16": 0x10, "BAYER_RGGB8": 0x20, "BAYER_GRBG8": 0x21, "BAYER_GBRG8": 0x22, "BAYER_BGGR8": 0x23, "BAYER_RGGB16": 0x30,
             "BAYER_GRBG16": 0x31, "BAYER_GBRG16": 0x32, "BAYER_BGGR16": 0x33, "YUYV": 0x40, "UYVY": 0x41, "NV12": 0x42}


# ---------------------------------------------------------------------------------------------- the numpy definition
def brute_decode(src, ws, hs, pitch, fmt, bits):
    """The formulas of the header, one pixel at a time, on the raw bytes."""
    s = [int(v) for v in np.ascontiguousarray(src, np.uint8).reshape(-1)]
    out = np.zeros((hs, ws, 3), np.int32)

    def clip8(v):
        return max(0, min(255, v))

    def sample(y, x, wide):
        if not wide:
            return s[y * pitch + x]
        return min(255, (s[y * pitch + 2 * x] | (s[y * pitch + 2 * x + 1] << 8)) >> (bits - 8))

    def reflect(i, n):
        return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)

    def yuv(Y, U, V):
        c, d, e = Y - 16, U - 128, V - 128
        return clip8((298 * c + 516 * d + 128) >> 8), clip8((298 * c - 100 * d - 208 * e + 128) >> 8), clip8((298 * c + 409 * e + 128) >> 8)

    for y in range(hs):
        for x in range(ws):
            if fmt == RF.GRAY16:
                out[y, x] = sample(y, x, True)
            elif fmt in RF.BAYER8 + RF.BAYER16:
                pat = RF.PATTERN[fmt & 3]

                def S(yy, xx):
                    return sample(reflect(yy, hs), reflect(xx, ws), fmt in RF.BAYER16)

                def colour(yy, xx):
                    return pat[2 * (yy & 1) + (xx & 1)]

                own = colour(y, x)
                px = {}
                if own in "RB":
                    px[own] = S(y, x)
                    px["G"] = (S(y - 1, x) + S(y + 1, x) + S(y, x - 1) + S(y, x + 1) + 2) >> 2
                    px["B" if own == "R" else "R"] = (S(y - 1, x - 1) + S(y - 1, x + 1) + S(y + 1, x - 1) + S(y + 1, x + 1) + 2) >> 2
                else:
                    px["G"] = S(y, x)
                    px[colour(y, x + 1)] = (S(y, x - 1) + S(y, x + 1) + 1) >> 1
                    px[colour(y + 1, x)] = (S(y - 1, x) + S(y + 1, x) + 1) >> 1
                out[y, x] = (px["B"], px["G"], px["R"])
            elif fmt == RF.YUYV:
                out[y, x] = yuv(s[y * pitch + 2 * x], s[y * pitch + 4 * (x >> 1) + 1], s[y * pitch + 4 * (x >> 1) + 3])
            elif fmt == RF.UYVY:
                out[y, x] = yuv(s[y * pitch + 2 * x + 1], s[y * pitch + 4 * (x >> 1)], s[y * pitch + 4 * (x >> 1) + 2])
            else:
                c = hs * pitch + (y >> 1) * pitch + 2 * (x >> 1)
                out[y, x] = yuv(s[y * pitch + x], s[c], s[c + 1])
    return out


@pytest.mark.parametrize("fmt", RF.NEW_FORMATS)
def test_decode_against_the_scalar_formulas(fmt):
    rng = np.random.default_rng(500 + fmt)
    (w0, h0), (sw, sh) = RF.min_size(fmt)
    for t in range(12):
        ws, hs = w0 + sw * int(rng.integers(0, 9)), h0 + sh * int(rng.integers(0, 7))
        bits = int(rng.integers(9, 17)) if fmt in RF.SIXTEEN else 0
        pitch = ws * RF.BPP[fmt] + 2 * int(rng.integers(0, 4)) + (int(rng.integers(0, 2)) if fmt not in RF.SIXTEEN else 0)
        src = RF.random_frame(rng, ws, hs, pitch, fmt, bits)
        assert src.size == RF.nbytes(hs, pitch, fmt)
        got = RF.decode(src, ws, hs, pitch, RF.pix_bits(fmt, bits))
        assert got.dtype == np.int32 and np.array_equal(got, brute_decode(src, ws, hs, pitch, fmt, bits or 16)), (t, ws, hs, pitch, bits)
        assert np.array_equal(got, RF.decode(src, ws, hs, pitch, fmt, bits))  # (the bits as an argument)


def test_a_constant_mosaic_decodes_to_that_constant():
    for fmt in RF.BAYER8 + RF.BAYER16:
        for ws in range(2, 6):
            for hs in range(2, 5):
                for value in (0, 1, 77, 255):
                    pitch = ws * RF.BPP[fmt] + 2
                    src = RF.pack(np.full((hs, ws, 3), value, np.uint8), fmt, pitch, 16)
                    got = RF.decode(src, ws, hs, pitch, fmt, 16)
                    assert got.shape == (hs, ws, 3) and (got == value).all(), (fmt, ws, hs, value)


def test_neutral_chroma_decodes_to_gray():
    Y = np.arange(256, dtype=np.uint8).reshape(2, 128)
    want = np.clip((298 * (Y.astype(np.int32) - 16) + 128) >> 8, 0, 255)
    half = np.full((2, 64), 128, np.uint8)
    for fmt, planes in ((RF.YUYV, (Y, half, half)), (RF.UYVY, (Y, half, half)), (RF.NV12, (Y, half[:1], half[:1]))):
        got = RF.decode(RF.pack(planes, fmt, 128 * RF.BPP[fmt] + 4), 128, 2, 128 * RF.BPP[fmt] + 4, fmt)
        assert all(np.array_equal(got[:, :, c], want) for c in range(3)), fmt
    assert want[0, 16] == 0 and want[1, 235 - 128] == 255 and want[0, 0] == 0 and want[1, 127] == 255


def test_twelve_bit_samples_reduce_by_four_bits():
    v = np.array([0, 15, 16, 17, 4079, 4080, 4095, 4096, 65535], np.int32)
    src = np.zeros((1, 2 * v.size), np.uint8)
    src[0, 0::2], src[0, 1::2] = v & 0xff, v >> 8
    got = RF.decode(src, v.size, 1, 2 * v.size, RF.pix_bits(RF.GRAY16, 12))
    assert np.array_equal(got[0, :, 0], np.minimum(255, v >> 4)) and got[0, :, 1].tolist() == [0, 0, 1, 1, 254, 255, 255, 255, 255]
    assert np.array_equal(RF.decode(src, v.size, 1, 2 * v.size, RF.GRAY16)[0, :, 2], v >> 8)  # (0 = 16 bits)


def test_the_identity_map_reproduces_decode():
    rng = np.random.default_rng(11)
    for fmt in RF.NEW_FORMATS + (RF.BGRA8,):
        ws, hs = 14, 10
        word = RF.pix_bits(fmt, 10) if fmt in RF.SIXTEEN else fmt
        pitch = ws * RF.BPP[fmt] + 6
        src = RF.random_frame(rng, ws, hs, pitch, word)
        out, valid = RF.remap(src, ws, hs, pitch, word, 0, *RF.identity_maps(ws, hs))
        assert valid.all() and np.array_equal(out, RF.decode(src, ws, hs, pitch, word)), fmt
    # the old layouts: rawfmt_ref.remap is rectify_ref.remap
    src = rng.integers(0, 256, (hs, ws * 3), dtype=np.uint8)
    mx, my = (rng.random((5, 9)) * 16 - 1).astype(F), (rng.random((5, 9)) * 12 - 1).astype(F)
    a, b = RF.remap(src, ws, hs, ws * 3, RF.RGB8, 0, mx, my), RR.remap(src, ws, hs, ws * 3, RR.RGB8, mx, my)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_reflection_is_inside_the_decode_not_the_border():
    """A tap outside the source contributes 0 even where a reflected sample exists; a tap on the last column reflects n -> n - 2."""
    ws, hs = 4, 4
    m = np.arange(16, dtype=np.uint8).reshape(4, 4) * 10 + 5
    src = m.reshape(-1)
    V = RF.decode(src, ws, hs, ws, RF.BAYER_RGGB8)
    assert V[0, 3, 1] == m[0, 3] and V[0, 3, 2] == (int(m[0, 2]) + int(m[0, 2]) + 1) >> 1  # green site of a red row: R from columns 2 and 4 -> 2
    mx, my = np.array([[3.5, 4.0, 3.0]], F), np.array([[0.0, 0.0, 0.0]], F)
    out, valid = RF.remap(src, ws, hs, ws, RF.BAYER_RGGB8, 0, mx, my)
    assert valid.tolist() == [[0, 0, 1]] and np.array_equal(out[0, 0], (V[0, 3] * 512 + 512) >> 10) and not out[0, 1].any() and np.array_equal(out[0, 2], V[0, 3])


def test_pack_round_trips():
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    for fmt in RF.BAYER8 + RF.BAYER16:
        m = RF._samples(RF.pack(img, fmt, 8 * RF.BPP[fmt] + 2, 12), 8, 6, 8 * RF.BPP[fmt] + 2, fmt in RF.BAYER16, 12)
        for y in range(2):
            for x in range(2):
                assert np.array_equal(m[y::2, x::2], img[y::2, x::2, "BGR".index(RF.PATTERN[fmt & 3][2 * y + x])]), (fmt, y, x)
    assert np.array_equal(RF.decode(RF.pack(img, RF.pix_bits(RF.GRAY16, 9), 20), 8, 6, 20, RF.GRAY16, 9)[:, :, 1], img[:, :, 0])
    for fmt in (RF.YUYV, RF.UYVY, RF.NV12):  # a gray image survives the forward and the backward matrix within their rounding
        gray = np.repeat(rng.integers(0, 256, (6, 8, 1), dtype=np.uint8), 3, 2)
        back = RF.decode(RF.pack(gray, fmt), 8, 6, 8 * RF.BPP[fmt], fmt)
        assert np.abs(back - gray).max() <= 2, fmt
        raw = RF.pack(gray, fmt, 8 * RF.BPP[fmt] + 3, fill=0xEE)
        assert raw.size == RF.nbytes(6, 8 * RF.BPP[fmt] + 3, fmt) and (raw.reshape(-1, 8 * RF.BPP[fmt] + 3)[:, -3:] == 0xEE).all()


# ---------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_library_exports_the_new_surface():
    text = open(HEADER).read()
    for name, value in CONSTANTS.items():
        assert re.search(r"#define\s+ADC_PIX_%s\s+0x%02x\b" % (name, value), text), name
        assert getattr(A, "PIX_" + name) == value and getattr(RF, name) == value
    assert re.search(r"#define\s+ADC_PIX_BITS\(fmt,\s*bits\)\s+\(\(fmt\)\s*\|\s*\(\(bits\)\s*<<\s*8\)\)", text)
    assert A.pix_bits(A.PIX_GRAY16, 12) == 0x0c10 and A.pix_bits(A.PIX_BAYER_BGGR16, 0) == 0x33
    assert re.search(r"int\s+adc_set_input_format\s*\(\s*adc_handle\s*\*\s*h,\s*int\s+side,\s*const\s+adc_raw_format\s*\*", text)
    assert re.search(r"int\s+adc_farm_set_input_format\s*\(\s*adc_farm\s*\*\s*f,\s*int\s+side,\s*const\s+adc_raw_format\s*\*", text)
    assert C.sizeof(A.RawFormat) == 16  # (the depth travels in the format word: the struct keeps its size)
    out = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"adc_set_input_format", "adc_farm_set_input_format"} <= names
    # the header compiles as C and the macro gives the documented word
    src = '#include "adcensus_c_api.h"\n_Static_assert(ADC_PIX_BITS(ADC_PIX_BAYER_GRBG16, 10) == 0x0a31, "bits");\nint main(void) { return 0; }\n'
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, text=True, check=True)


def test_raw_format_arithmetic_and_signatures():
    r = A.RawFormat(10, 4, 0, A.PIX_NV12)
    assert (r.pitch_bytes, r.nbytes) == (10, 60) and A.RawFormat(10, 4, 17, A.PIX_NV12).nbytes == 102
    assert A.RawFormat(10, 4, 0, A.pix_bits(A.PIX_BAYER_GBRG16, 12)).pitch_bytes == 20 and A.RawFormat(10, 4, 0, A.PIX_BAYER_GBRG8).pitch_bytes == 10
    assert A.RawFormat(10, 4, 0, A.PIX_YUYV).nbytes == 80 and A.RawFormat(10, 4, 0, A.PIX_UYVY).pitch_bytes == 20
    assert A.RawFormat(10, 4, 0, A.PIX_GRAY16).nbytes == 80 and A.RawFormat(10, 4, 0, A.PIX_BGRA8).nbytes == 160
    for code in RF.BPP:
        assert A.PIX_BYTES[code] == RF.BPP[code] and A.RawFormat(6, 4, 0, code).nbytes == RF.nbytes(4, 6 * RF.BPP[code], code)
    for cls in (A.ADCensusStereo, A.PairFarm):
        assert list(inspect.signature(cls.set_input_format).parameters) == ["self", "side", "raw"]
    L = A.lib()
    for name in ("adc_set_input_format", "adc_farm_set_input_format"):
        assert getattr(L, name).argtypes == [C.c_void_p, C.c_int, C.POINTER(A.RawFormat)]
    s = A._RectifyState()
    s.set(0, A.RawFormat(10, 4, 12, A.PIX_NV12))
    s.set(1, A.RawFormat(10, 4, 0, A.PIX_BAYER_RGGB16))
    assert s.on() and s.sizes(120) == (72, 80)


def test_refusals_that_need_no_device():
    """Every refusal comes before the first HIP call and before the handle is looked at, so a zeroed block stands in for a handle (the
    GPU tier repeats them on a real one, with the message)."""
    L = A.lib()
    good = A.RawFormat(8, 4, 0, A.PIX_NV12)
    model = A.CameraModel(fx=1, fy=1, new_fx=1, new_fy=1)
    assert L.adc_set_input_format(None, 0, C.byref(good)) == 1 and L.adc_farm_set_input_format(None, 0, C.byref(good)) == 1
    fake = C.create_string_buffer(1 << 20)
    h = C.cast(fake, C.c_void_p)
    mp = np.zeros((4, 8), F).ctypes.data
    assert L.adc_set_input_format(h, 0, None) == 1
    for side in (-1, 2):
        assert L.adc_set_input_format(h, side, C.byref(good)) == 1 and "side" in A.last_error()
    R = A.RawFormat
    bad = {
        "codes 4..15 and between the groups": [R(8, 4, 24, c) for c in list(range(4, 16)) + [0x11, 0x1f, 0x24, 0x2f, 0x34, 0x43, 0x50, 0xff, -1, 0x10000 | A.PIX_GRAY16]],
        "pitch below a row": [R(8, 4, 7, A.PIX_BAYER_RGGB8), R(8, 4, 15, A.PIX_BAYER_RGGB16), R(8, 4, 14, A.PIX_GRAY16), R(8, 4, 15, A.PIX_YUYV), R(8, 4, 15, A.PIX_UYVY),
                              R(8, 4, 7, A.PIX_NV12), R(8, 4, -8, A.PIX_NV12)],
        "larger than 2^31 - 1": [R(30000, 30000, 90000, A.PIX_BGR8), R(32000, 32766, 65600, A.PIX_GRAY16), R(32766, 32766, 50000, A.PIX_NV12)],
        "16-bit pitch odd": [R(8, 4, 17, A.PIX_GRAY16), R(8, 4, 19, A.PIX_BAYER_BGGR16)],
        "Bayer smaller than 2 x 2": [R(1, 4, 8, A.PIX_BAYER_GRBG8), R(8, 1, 8, A.PIX_BAYER_GRBG8), R(1, 4, 8, A.PIX_BAYER_GBRG16), R(8, 1, 16, A.PIX_BAYER_GBRG16)],
        "YUV width odd": [R(7, 4, 16, A.PIX_YUYV), R(7, 4, 16, A.PIX_UYVY), R(7, 4, 8, A.PIX_NV12)],
        "NV12 height odd": [R(8, 3, 8, A.PIX_NV12)],
        "bits on an 8-bit layout": [R(8, 4, 32, A.pix_bits(c, 8)) for c in (A.PIX_BGR8, A.PIX_GRAY8, A.PIX_BAYER_RGGB8, A.PIX_YUYV, A.PIX_UYVY, A.PIX_NV12)] +
                                   [R(8, 4, 32, A.pix_bits(A.PIX_NV12, 12))],
        "bits outside 9..16": [R(8, 4, 16, A.pix_bits(A.PIX_GRAY16, b)) for b in (1, 8, 17, 255)] + [R(8, 4, 16, A.pix_bits(A.PIX_BAYER_RGGB16, 8))],
        "width / height range": [R(0, 4, 8, A.PIX_NV12), R(8, 0, 8, A.PIX_NV12), R(32768, 4, 65536, A.PIX_GRAY16), R(8, 32768, 8, A.PIX_BAYER_RGGB8)],
    }
    for rule, formats in bad.items():
        for f in formats:
            what = (rule, f.width, f.height, f.pitch_bytes, hex(f.format))
            assert L.adc_set_input_format(h, 0, C.byref(f)) == 1 and A.last_error().startswith("adc_set_input_format"), what
            assert L.adc_set_rectify_maps(h, 1, C.byref(f), mp, mp) == 1 and A.last_error().startswith("adc_set_rectify_maps"), what
            assert L.adc_set_rectify_model(h, 1, C.byref(f), C.byref(model)) == 1, what
    # a well-formed layout of another geometry than the handle's (the zeroed block: 0 x 0)
    for f in (good, R(8, 4, 0, A.pix_bits(A.PIX_BAYER_RGGB16, 16)), R(2, 2, 0, A.PIX_NV12), R(8, 4, 0, A.pix_bits(A.PIX_GRAY16, 9)), R(8, 4, 0, A.PIX_BGR8)):
        assert L.adc_set_input_format(h, 0, C.byref(f)) == 1 and "handle" in A.last_error(), hex(f.format)
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    st.width, st.height = 8, 4
    with pytest.raises(RuntimeError):
        st.set_input_format(A.SIDE_LEFT, good)


CALLER = r'''
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
int main() {
    ADCensusStereo s; ADCensusOption o;
    adc_raw_format nv12 = {8, 4, 10, ADC_PIX_NV12}, bayer = {8, 4, 16, ADC_PIX_BITS(ADC_PIX_BAYER_GBRG16, 12)}, odd = {8, 3, 8, ADC_PIX_NV12};
    adc_raw_format bits = {8, 4, 8, ADC_PIX_BITS(ADC_PIX_NV12, 12)}, hole = {8, 4, 8, 0x24}, pitch = {8, 4, 17, ADC_PIX_GRAY16};
    adc_camera_model m = {100.f, 100.f, 4.f, 2.f, 0.f, 0.f, 0.f, 0.f, 0.f, {1, 0, 0, 0, 1, 0, 0, 0, 1}, 100.f, 100.f, 4.f, 2.f};
    float32 d[32] = {0};
    uint8 img[96] = {0};
    bool ok = s.SetInputFormat(ADC_SIDE_LEFT, &nv12) && s.SetInputFormat(ADC_SIDE_RIGHT, &bayer) && s.SetRectifyModel(ADC_SIDE_RIGHT, &bayer, &m);
    ok = ok && s.SetInputFormat(ADC_SIDE_RIGHT, &nv12);
    ok = ok && !s.SetInputFormat(2, &nv12) && !s.SetInputFormat(ADC_SIDE_LEFT, nullptr) && !s.SetInputFormat(ADC_SIDE_LEFT, &odd) && !s.SetInputFormat(ADC_SIDE_LEFT, &bits);
    ok = ok && !s.SetInputFormat(ADC_SIDE_LEFT, &hole) && !s.SetInputFormat(ADC_SIDE_LEFT, &pitch) && !s.SetRectifyModel(ADC_SIDE_LEFT, &odd, &m);
    ok = ok && !s.Rectify(ADC_SIDE_LEFT, img, img) && s.ClearRectify();
    return (ok && !s.Match(img, img, d) && !s.Initialize(0, 0, o)) ? 0 : 1;
}
'''


def test_facade_compiles_and_exports_the_member(tmp_path):
    """Before Initialize the setter only checks and remembers, so the program runs without a device."""
    src = tmp_path / "caller.cpp"
    src.write_text(CALLER)
    libdir = os.path.join(ROOT, "adcensus_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libadcensus.so")):
        pytest.fail("libadcensus.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "caller"),
                    "-L", libdir, "-ladcensus", "-ladcensus_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(libdir, "libadcensus.so")], capture_output=True, text=True, check=True).stdout
    assert "ADCensusStereo::SetInputFormat(int, adc_raw_format const*)" in out
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def test_cli_rejects_a_malformed_raw_flag(tmp_path):
    """Checked while the arguments are parsed: the frames named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    bad = [[], ["NV12"], ["NV12,8"], ["NV12,8,4,8,0,1"], ["NV13,8,4"], ["nv12,8,4"], ["NV12,8,x"], ["NV12,8,4,"], ["NV12,7,4"], ["NV12,8,3"], ["NV12,8,4,7"],
           ["NV12,8,4,8,12"], ["GRAY16,8,4,17"], ["GRAY16,8,4,16,8"], ["GRAY16,8,4,16,17"], ["BAYER_RGGB8,1,4"], ["BAYER_RGGB8,8,4,8,10"], ["YUYV,7,4"],
           ["UYVY,8,4,15"], ["BGR8,0,4"], ["BGR8,40000,4"], ["BGR8,8,-4"], ["BGR8,30000,30000"], ["4,8,4"]]
    for value in bad:
        r = subprocess.run([cli, str(tmp_path / "no_left.raw"), str(tmp_path / "no_right.raw"), "0", "64", str(tmp_path / "out"), "--raw"] + value,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--raw refused" in r.stdout and "Image Loading" not in r.stdout, (value, r.stdout)
    for value in ("NV12,8,4", "BAYER_GBRG16,9,5,20,12", "GRAY16,3,3,0,9", "UYVY,8,1", "BGRA8,5,5,23"):
        r = subprocess.run([cli, str(tmp_path / "no_left.raw"), str(tmp_path / "no_right.raw"), "--raw", value], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Image Loading" in r.stdout and "--raw refused" not in r.stdout, (value, r.stdout)  # (well-formed: gets as far as the frames)


def test_cli_raw_under_sanitizers(tmp_path):
    """The flag's parsing, the loading of headerless frames and the facade's SetInputFormat in the ASAN / UBSAN build on the stub C ABI
    (which checks the arguments and copies nothing): well-formed runs complete cleanly and write the map and the two converted images."""
    from PIL import Image
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "adcensus_amd", "host"), "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cli = os.path.join(ROOT, "adcensus_amd", "build", "asan", "adcensus_cli_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    rng = np.random.default_rng(6)
    ws, hs = 46, 30

    def frames(fmt, pitch, name):
        paths = []
        for side in "lr":
            p = tmp_path / ("%s_%s.raw" % (name, side))
            RF.random_frame(rng, ws, hs, pitch, fmt).tofile(p)
            paths.append(str(p))
        return paths

    def run(paths, *extra):
        r = subprocess.run([cli, paths[0], paths[1], "0", "16", *extra], env=env, capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        return r

    # (the stub's adc_match reads W * H * 3 bytes of whatever it is handed, so the frames carry a pitch that makes them at least that large)
    for name, fmt, pitch, flag in (("nv12", RF.NV12, 96, "NV12,46,30,96"), ("bayer", RF.pix_bits(RF.BAYER_GRBG16, 12), 140, "BAYER_GRBG16,46,30,140,12"),
                                   ("yuyv", RF.YUYV, 138, "YUYV,46,30,138"), ("gray", RF.GRAY16, 144, "GRAY16,46,30,144"), ("bgra", RF.BGRA8, 4 * ws, "BGRA8,46,30")):
        out = str(tmp_path / ("out_" + name))
        assert run(frames(fmt, pitch, name), out, "--raw", flag).returncode == 0, name
        assert os.path.exists(out + ".pfm") and Image.open(out + "-rect-left.png").size == (ws, hs) and Image.open(out + "-rect-right.png").size == (ws, hs)
    paths = frames(RF.NV12, ws, "short")
    assert run(paths, str(tmp_path / "short"), "--raw", "NV12,46,30,48").returncode != 0 and not os.path.exists(str(tmp_path / "short") + ".pfm")  # (a file too small)
    assert run(paths, str(tmp_path / "long"), "--raw", "NV12,46,28").returncode != 0 and not os.path.exists(str(tmp_path / "long") + ".pfm")  # (a file too large)
    assert run(paths, str(tmp_path / "bad"), "--raw", "NV12,46,31").returncode != 0
    # with --rectify the flag gives the raw geometry of both cameras (the stub of the rectification knows the 8-bit layouts)
    from tests.test_rectify_api import camera_file
    model = RR.example_model(ws, hs, ws, hs)
    cam = camera_file(tmp_path / "cam.txt", (ws, hs, ws * 3, 0), model, rect=(40, 28))
    out = str(tmp_path / "rect")
    assert run(frames(RF.BGRA8, 4 * ws + 8, "bgra1"), out, "--raw", "BGRA8,46,30,192", "--rectify", cam + "," + cam).returncode == 0
    assert Image.open(out + "-rect-left.png").size == (40, 28) and os.path.exists(out + ".pfm")
    r = run(frames(RF.BGRA8, 4 * ws, "bgra2"), str(tmp_path / "rect2"), "--rectify", cam + "," + cam, "--raw", "BGRA8,44,30")
    assert r.returncode != 0 and "--raw refused" in r.stdout
