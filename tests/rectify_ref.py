"""The rectification's definition (include/adcensus_c_api.h: adc_set_rectify_maps / adc_set_rectify_model) in numpy, independent of
the kernels; the GPU tests compare k_rectify.hip with it bit for bit.

remap     per destination pixel, from float32 maps mx, my [H][W] and a source image [Hs][pitch] of one of four formats:
  outside   !(fabsf(mx) < 32768) or !(fabsf(my) < 32768) (NaN, +-inf included): B = G = R = 0, valid = 0
  fixed     X = (int)rintf(mx * 32), Y likewise (the product is exact, rounding is half to even); xi = X >> 5, ax = X & 31
            (arithmetic shift), yi / ay the same
  taps      (yi, xi), (yi, xi+1), (yi+1, xi), (yi+1, xi+1) with the integer weights (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax*ay
            (sum 1024); a tap outside [0, Ws) x [0, Hs) contributes 0
  output    per channel (sum of w * p + 512) >> 10
  valid     1 iff every tap with a nonzero weight is inside
model     the float32 maps of one camera (intrinsics, Brown-Conrady k1 k2 p1 p2 k3, rectifying rotation R, new intrinsics), one
          rounding per operation in the order written in model_maps below.

By construction these are the weights of OpenCV's INTER_LINEAR / BORDER_CONSTANT remap (INTER_BITS = 5; its 15-bit table is 32 times
these products) on maps shaped like initUndistortRectifyMap's: a derivation, not something the tests check."""
import numpy as np

BGR8, RGB8, GRAY8, BGRA8 = 0, 1, 2, 3
BPP = {BGR8: 3, RGB8: 3, GRAY8: 1, BGRA8: 4}
F = np.float32


def source_bgr(src, width, height, pitch, fmt):
    """Source bytes [Hs * pitch] (or [Hs][pitch]) -> int32 [Hs][Ws][3] in B, G, R order."""
    s = np.ascontiguousarray(src, np.uint8).reshape(-1)
    assert pitch >= width * BPP[fmt] and s.size >= height * pitch
    rows = s[:height * pitch].reshape(height, pitch)[:, :width * BPP[fmt]].reshape(height, width, BPP[fmt]).astype(np.int32)
    if fmt == GRAY8:
        return np.repeat(rows, 3, axis=2)
    if fmt == RGB8:
        return rows[:, :, ::-1].copy()
    return rows[:, :, :3].copy()


def quantise(mx, my):
    """-> (outside bool, xi, ax, yi, ay int32) [H][W]; the integer fields are 0 where outside."""
    mx, my = np.asarray(mx, F), np.asarray(my, F)
    with np.errstate(invalid="ignore", over="ignore"):
        outside = ~(np.abs(mx) < F(32768.0)) | ~(np.abs(my) < F(32768.0))
        X = np.rint(np.where(outside, F(0), mx) * F(32.0)).astype(np.int32)
        Y = np.rint(np.where(outside, F(0), my) * F(32.0)).astype(np.int32)
    return outside, X >> 5, X & 31, Y >> 5, Y & 31


def remap(src, width, height, pitch, fmt, mx, my):
    """-> (uint8 [H][W][3] B,G,R, valid uint8 [H][W])"""
    img = source_bgr(src, width, height, pitch, fmt)
    outside, xi, ax, yi, ay = quantise(mx, my)
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


def model_maps(model, W, H):
    """model: dict with fx fy cx cy k1 k2 p1 p2 k3, R (9 values, row-major), new_fx new_fy new_cx new_cy -> float32 mx, my [H][W]."""
    g = {k: F(model[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "new_fx", "new_fy", "new_cx", "new_cy")}
    R = [F(v) for v in model["R"]]
    one, two = F(1.0), F(2.0)
    u = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    v = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
    with np.errstate(all="ignore"):
        xn = (u - g["new_cx"]) / g["new_fx"]
        yn = (v - g["new_cy"]) / g["new_fy"]
        X = (R[0] * xn + R[3] * yn) + R[6]
        Y = (R[1] * xn + R[4] * yn) + R[7]
        Wc = (R[2] * xn + R[5] * yn) + R[8]
        x = X / Wc
        y = Y / Wc
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy = x * y
        rad = one + r2 * (g["k1"] + r2 * (g["k2"] + r2 * g["k3"]))
        xd = (x * rad + (two * g["p1"]) * xy) + g["p2"] * (r2 + two * x2)
        yd = (y * rad + g["p1"] * (r2 + two * y2)) + (two * g["p2"]) * xy
        mx = g["fx"] * xd + g["cx"]
        my = g["fy"] * yd + g["cy"]
    assert mx.dtype == F and my.dtype == F
    return np.ascontiguousarray(mx), np.ascontiguousarray(my)


def pack_source(bgr, fmt, pitch=None, fill=0xA5):
    """uint8 [Hs][Ws][3] B,G,R -> the source bytes [Hs][pitch] in `fmt` (GRAY8 takes the B channel; padding and alpha = fill)."""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    hs, ws = bgr.shape[:2]
    bpp = BPP[fmt]
    pitch = ws * bpp if pitch is None else pitch
    out = np.full((hs, pitch), fill, np.uint8)
    px = out[:, :ws * bpp].reshape(hs, ws, bpp)
    if fmt == GRAY8:
        px[:, :, 0] = bgr[:, :, 0]
    elif fmt == RGB8:
        px[:, :, :] = bgr[:, :, ::-1]
    else:
        px[:, :, :3] = bgr
    return out


def rotation(ry=0.0, rx=0.0, rz=0.0):
    """R = Rz * Rx * Ry (float64 -> 9 float32 values, row-major)."""
    cy, sy, cx, sx, cz, sz = np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx), np.cos(rz), np.sin(rz)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return [float(F(v)) for v in (Rz @ Rx @ Ry).reshape(-1)]


def identity_model(cx=0.0, cy=0.0, f=1000.0):
    return dict(fx=f, fy=f, cx=cx, cy=cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, R=[1, 0, 0, 0, 1, 0, 0, 0, 1],
                new_fx=f, new_fy=f, new_cx=cx, new_cy=cy)


def example_model(ws, hs, W, H):
    """The issue's example: k = (-0.12, 0.05, 7e-4, -4e-4, 0.01), rotations 0.01 / -0.006 / 0.004 rad about y / x / z, f 1734 -> 1700
    (scaled to the source width), principal points at the image centres."""
    s = ws / 1920.0
    return dict(fx=1734.0 * s, fy=1734.5 * s, cx=ws / 2.0 + 3.25, cy=hs / 2.0 - 2.5, k1=-0.12, k2=0.05, p1=7e-4, p2=-4e-4, k3=0.01,
                R=rotation(0.01, -0.006, 0.004), new_fx=1700.0 * s, new_fy=1700.0 * s, new_cx=W / 2.0, new_cy=H / 2.0)


def second_model(ws, hs, W, H):
    """A different camera for the end-to-end pairs."""
    s = ws / 1920.0
    return dict(fx=1650.0 * s, fy=1648.0 * s, cx=ws / 2.0 - 5.5, cy=hs / 2.0 + 4.0, k1=0.08, k2=-0.03, p1=-5e-4, p2=6e-4, k3=0.004,
                R=rotation(-0.008, 0.005, -0.003), new_fx=1640.0 * s, new_fy=1640.0 * s, new_cx=W / 2.0 + 1.5, new_cy=H / 2.0 - 0.5)
