"""The camera layouts' definition (include/adcensus_c_api.h: ADC_PIX_GRAY16, ADC_PIX_BAYER_*, ADC_PIX_YUYV / UYVY / NV12,
adc_set_input_format) in numpy, independent of the kernels; the GPU tests compare k_rectify.hip with it bit for bit.

decode    source bytes -> the virtual B, G, R image V [Hs][Ws][3] the remap takes its taps from.  All integer, >> arithmetic:
  16 bit    little-endian words; s = min(255, v >> (bits - 8)), bits 9..16 (0 = 16); everything below works on s
  GRAY16    B = G = R = s
  Bayer     the four letters of a pattern are the colours of pixels (0,0), (0,1), (1,0), (1,1).  S(y, x): the sample at coordinates
            reflected into the image without repeating the edge (-1 -> 1, n -> n - 2).  Red / blue site: own colour S(y,x), green
            (S(y-1,x) + S(y+1,x) + S(y,x-1) + S(y,x+1) + 2) >> 2, the other colour the same of the four diagonal neighbours.  Green site:
            green S(y,x), the colour of the left / right neighbours (S(y,x-1) + S(y,x+1) + 1) >> 1, of the upper / lower ones
            (S(y-1,x) + S(y+1,x) + 1) >> 1
  YUV       BT.601 limited range, the pixel's own chroma sample: c = Y - 16, d = U - 128, e = V - 128;
            R = clip8((298c + 409e + 128) >> 8), G = clip8((298c - 100d - 208e + 128) >> 8), B = clip8((298c + 516d + 128) >> 8).
            YUYV rows: Y0 U Y1 V per pixel pair, UYVY: U Y0 V Y1.  NV12: luma plane [Hs][pitch], at byte Hs * pitch the chroma plane
            [Hs / 2][pitch] of U, V pairs; pixel (y, x) reads U = C[y >> 1][2 * (x >> 1)] and V behind it
remap     rectify_ref.quantise and rectify_ref's four taps, weights, constant border, rounding and valid map on decode's image.
          Under the identity map it reproduces decode: (1024 p + 512) >> 10 = p.
The four 8-bit layouts of rectify_ref decode through rectify_ref.source_bgr."""
import numpy as np

from tests import rectify_ref as RR

BGR8, RGB8, GRAY8, BGRA8 = RR.BGR8, RR.RGB8, RR.GRAY8, RR.BGRA8
GRAY16 = 0x10
BAYER_RGGB8, BAYER_GRBG8, BAYER_GBRG8, BAYER_BGGR8 = 0x20, 0x21, 0x22, 0x23
BAYER_RGGB16, BAYER_GRBG16, BAYER_GBRG16, BAYER_BGGR16 = 0x30, 0x31, 0x32, 0x33
YUYV, UYVY, NV12 = 0x40, 0x41, 0x42
BAYER8 = (BAYER_RGGB8, BAYER_GRBG8, BAYER_GBRG8, BAYER_BGGR8)
BAYER16 = (BAYER_RGGB16, BAYER_GRBG16, BAYER_GBRG16, BAYER_BGGR16)
SIXTEEN = (GRAY16,) + BAYER16
NEW_FORMATS = (GRAY16,) + BAYER8 + BAYER16 + (YUYV, UYVY, NV12)
BPP = dict(RR.BPP)  # bytes per pixel of a row (NV12: of a luma row)
BPP.update({GRAY16: 2, YUYV: 2, UYVY: 2, NV12: 1})
BPP.update({f: 1 for f in BAYER8})
BPP.update({f: 2 for f in BAYER16})
PATTERN = {0: "RGGB", 1: "GRBG", 2: "GBRG", 3: "BGGR"}  # by the low two bits of a Bayer code
NAMES = {BGR8: "BGR8", RGB8: "RGB8", GRAY8: "GRAY8", BGRA8: "BGRA8", GRAY16: "GRAY16", YUYV: "YUYV", UYVY: "UYVY", NV12: "NV12"}
NAMES.update({f: "BAYER_%s8" % PATTERN[f & 3] for f in BAYER8})
NAMES.update({f: "BAYER_%s16" % PATTERN[f & 3] for f in BAYER16})


def pix_bits(fmt, bits):
    return fmt | (bits << 8)


def nbytes(height, pitch, fmt):
    return height * pitch * 3 // 2 if (fmt & 0xff) == NV12 else height * pitch


def min_size(fmt):
    """smallest legal (width, height) and their steps"""
    fmt &= 0xff
    if fmt in BAYER8 + BAYER16:
        return (2, 2), (1, 1)
    if fmt in (YUYV, UYVY):
        return (2, 1), (2, 1)
    if fmt == NV12:
        return (2, 2), (2, 2)
    return (1, 1), (1, 1)


def _samples(s, width, height, pitch, sixteen, bits):
    """-> int32 [Hs][Ws] 8-bit samples of a one-sample-per-pixel layout"""
    rows = s[:height * pitch].reshape(height, pitch)
    if not sixteen:
        return rows[:, :width].astype(np.int32)
    assert pitch % 2 == 0 and 9 <= bits <= 16
    v = rows[:, 0:2 * width:2].astype(np.int32) | (rows[:, 1:2 * width:2].astype(np.int32) << 8)  # little-endian
    return np.minimum(255, v >> (bits - 8))


def _reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _clip8(v):
    return np.clip(v, 0, 255)


def _yuv_bgr(Y, U, V):
    c, d, e = Y - 16, U - 128, V - 128
    r = _clip8((298 * c + 409 * e + 128) >> 8)
    g = _clip8((298 * c - 100 * d - 208 * e + 128) >> 8)
    b = _clip8((298 * c + 516 * d + 128) >> 8)
    return np.stack([b, g, r], axis=2).astype(np.int32)


def decode(src, width, height, pitch, fmt, bits=0):
    """Source bytes [nbytes] -> int32 [Hs][Ws][3] in B, G, R order.  `fmt` may carry the bits (pix_bits); `bits` 0 = 16."""
    bits = bits or ((fmt >> 8) & 0xff) or 16
    fmt &= 0xff
    s = np.ascontiguousarray(src, np.uint8).reshape(-1)
    assert pitch >= width * BPP[fmt] and s.size >= nbytes(height, pitch, fmt)
    if fmt in RR.BPP:
        return RR.source_bgr(s, width, height, pitch, fmt)
    if fmt == GRAY16:
        return np.repeat(_samples(s, width, height, pitch, True, bits)[:, :, None], 3, axis=2)
    if fmt in BAYER8 + BAYER16:
        assert width >= 2 and height >= 2
        m = _samples(s, width, height, pitch, fmt in BAYER16, bits)
        y, x = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
        ring = m[_reflect(np.arange(-1, height + 1), height)][:, _reflect(np.arange(-1, width + 1), width)]

        def S(dy, dx):
            return ring[1 + dy:1 + dy + height, 1 + dx:1 + dx + width]

        cross = (S(-1, 0) + S(1, 0) + S(0, -1) + S(0, 1) + 2) >> 2
        diag = (S(-1, -1) + S(-1, 1) + S(1, -1) + S(1, 1) + 2) >> 2
        horiz = (S(0, -1) + S(0, 1) + 1) >> 1
        vert = (S(-1, 0) + S(1, 0) + 1) >> 1
        pat = PATTERN[fmt & 3]
        site = np.array([[pat[0], pat[1]], [pat[2], pat[3]]])[y & 1, x & 1]       # colour of the site
        beside = np.array([[pat[1], pat[0]], [pat[3], pat[2]]])[y & 1, x & 1]     # colour of its left / right neighbours
        out = {}
        for colour, other in (("R", "B"), ("B", "R")):
            out[colour] = np.where(site == colour, m, np.where(site == other, diag, np.where(beside == colour, horiz, vert)))
        out["G"] = np.where(site == "G", m, cross)
        return np.stack([out["B"], out["G"], out["R"]], axis=2).astype(np.int32)
    assert width % 2 == 0
    x = np.arange(width)
    if fmt in (YUYV, UYVY):
        rows = s[:height * pitch].reshape(height, pitch).astype(np.int32)
        yo, uo = (0, 1) if fmt == YUYV else (1, 0)
        return _yuv_bgr(rows[:, 2 * x + yo], rows[:, 4 * (x >> 1) + uo], rows[:, 4 * (x >> 1) + uo + 2])
    assert fmt == NV12 and height % 2 == 0
    luma = s[:height * pitch].reshape(height, pitch).astype(np.int32)
    chroma = s[height * pitch:height * pitch * 3 // 2].reshape(height // 2, pitch).astype(np.int32)
    cy = np.arange(height) >> 1
    return _yuv_bgr(luma[:, :width], chroma[cy][:, 2 * (x >> 1)], chroma[cy][:, 2 * (x >> 1) + 1])


def remap(src, width, height, pitch, fmt, bits, mx, my):
    """-> (uint8 [H][W][3] B,G,R, valid uint8 [H][W]): rectify_ref.remap with decode's image as the source"""
    img = decode(src, width, height, pitch, fmt, bits)
    outside, xi, ax, yi, ay = RR.quantise(mx, my)
    acc = np.zeros(xi.shape + (3,), np.int32)
    valid = ~outside
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        w = (ax if dx else 32 - ax) * (ay if dy else 32 - ay)
        ty, tx = yi + dy, xi + dx
        inside = (tx >= 0) & (tx < width) & (ty >= 0) & (ty < height) & ~outside
        p = img[np.clip(ty, 0, height - 1), np.clip(tx, 0, width - 1)]
        acc += np.where(inside, w, 0)[..., None] * p
        valid &= inside | (w == 0)
    out = ((acc + 512) >> 10).astype(np.uint8)
    out[outside] = 0
    return out, valid.astype(np.uint8)


def identity_maps(width, height):
    return (np.ascontiguousarray(np.broadcast_to(np.arange(width, dtype=np.float32)[None, :], (height, width))),
            np.ascontiguousarray(np.broadcast_to(np.arange(height, dtype=np.float32)[:, None], (height, width))))


def _words(out, height, width, s, bits):
    """8-bit samples -> little-endian words of `bits` significant bits; the bits below the eight kept ones are filled with a pattern"""
    low = bits - 8
    y, x = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    v = (s.astype(np.int32) << low) | ((x * 7 + y * 3) & ((1 << low) - 1))
    out[:height, 0:2 * width:2] = (v & 0xff).astype(np.uint8)
    out[:height, 1:2 * width:2] = (v >> 8).astype(np.uint8)


def pack(bgr_or_planes, fmt, pitch=None, bits=0, fill=0xA5):
    """Encodes a test frame: uint8 [Hs][Ws][3] B,G,R -- or, for the YUV layouts, a tuple of planes (Y [Hs][Ws], U, V [Hs][Ws / 2] for
    YUYV / UYVY, [Hs / 2][Ws / 2] for NV12) -- -> uint8 [nbytes] in `fmt`, padding bytes = fill.  GRAY16 takes the B channel, a Bayer
    site its own colour, 16-bit samples are the 8-bit values shifted up with the low bits filled; BGR to YUV is the usual integer
    BT.601 forward matrix with the chroma of a pair / a 2 x 2 block averaged (test data, not part of the definition)."""
    bits = bits or ((fmt >> 8) & 0xff) or 16
    fmt &= 0xff
    if fmt in RR.BPP:
        return RR.pack_source(bgr_or_planes, fmt, pitch, fill).reshape(-1)
    planes = isinstance(bgr_or_planes, tuple)
    first = np.ascontiguousarray(bgr_or_planes[0] if planes else bgr_or_planes, np.uint8)
    hs, ws = first.shape[:2]
    pitch = ws * BPP[fmt] if pitch is None else pitch
    assert pitch >= ws * BPP[fmt]
    out = np.full((nbytes(hs, pitch, fmt) // pitch, pitch), fill, np.uint8)
    if fmt == GRAY16:
        _words(out, hs, ws, first[:, :, 0], bits)
    elif fmt in BAYER8 + BAYER16:
        y, x = np.meshgrid(np.arange(hs), np.arange(ws), indexing="ij")
        pat = PATTERN[fmt & 3]
        chan = np.array([["BGR".index(pat[0]), "BGR".index(pat[1])], ["BGR".index(pat[2]), "BGR".index(pat[3])]])[y & 1, x & 1]
        m = np.take_along_axis(first, chan[:, :, None], axis=2)[:, :, 0]
        if fmt in BAYER8:
            out[:, :ws] = m
        else:
            _words(out, hs, ws, m, bits)
    else:
        sub = 2 if fmt == NV12 else 1
        if planes:
            Y, U, V = (np.ascontiguousarray(p, np.uint8) for p in bgr_or_planes)
        else:
            b, g, r = (first[:, :, k].astype(np.int32) for k in range(3))
            Y = (((66 * r + 129 * g + 25 * b + 128) >> 8) + 16).astype(np.uint8)
            u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
            v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
            U = np.clip(u.reshape(hs // sub, sub, ws // 2, 2).sum(axis=(1, 3)) // (2 * sub), 0, 255).astype(np.uint8)
            V = np.clip(v.reshape(hs // sub, sub, ws // 2, 2).sum(axis=(1, 3)) // (2 * sub), 0, 255).astype(np.uint8)
        assert Y.shape == (hs, ws) and U.shape == V.shape == (hs // sub, ws // 2)
        if fmt == NV12:
            out[:hs, :ws] = Y
            out[hs:, 0:ws:2] = U
            out[hs:, 1:ws:2] = V
        else:
            yo, uo = (0, 1) if fmt == YUYV else (1, 0)
            out[:, yo:2 * ws:2] = Y
            out[:, uo:2 * ws:4] = U
            out[:, uo + 2:2 * ws:4] = V
    return out.reshape(-1)


def random_frame(rng, width, height, pitch, fmt, bits=0, fill=0xA5):
    """Random source bytes of a layout: every byte random, the words of a 16-bit layout masked to their significant bits with a few
    salted above them (the min(255, .) of the reduction), padding bytes = fill."""
    bits = bits or ((fmt >> 8) & 0xff) or 16
    fmt &= 0xff
    rows = nbytes(height, pitch, fmt) // pitch
    out = np.full((rows, pitch), fill, np.uint8)
    n = width * BPP[fmt]
    if fmt in SIXTEEN:
        v = rng.integers(0, 1 << bits, (rows, width)).astype(np.int32)
        v[rng.random((rows, width)) < 0.02] = 0xffff
        out[:, 0:n:2] = (v & 0xff).astype(np.uint8)
        out[:, 1:n:2] = (v >> 8).astype(np.uint8)
    else:
        out[:, :n] = rng.integers(0, 256, (rows, n), dtype=np.uint8)
    return out.reshape(-1)
