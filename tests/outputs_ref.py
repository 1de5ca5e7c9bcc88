"""The outputs of adc_match_out / adc_reproject_device (include/adcensus_c_api.h: adc_outputs) computed in numpy from a final
disparity map and the left image -- the definition the GPU tests hold the kernels to, bit for bit.  Every operand is np.float32 (an
array or a scalar), so every operation rounds once to binary32; numpy's float32 division is correctly rounded."""
import numpy as np

POINT_DTYPE = np.dtype({"names": ["x", "y", "z", "r", "g", "b", "pad"], "formats": ["<f4", "<f4", "<f4", "u1", "u1", "u1", "u1"],
                        "offsets": [0, 4, 8, 12, 13, 14, 15], "itemsize": 16})
F = np.float32
INF = F(np.inf)


def calib_f32(calib):
    """(focal_px, baseline, cx, cy, doffs) as np.float32 scalars plus fb = focal_px * baseline (one f32 multiply)."""
    f, b, cx, cy, doffs = (F(v) for v in calib)
    return f, b, cx, cy, doffs, F(f * b)


def disp8(disp):
    """uint8 [H][W]: SaveDisparityMap's image (main.cpp:180-206), the formula tests/test_gpu_api.py::test_cpp_facade_cli pins."""
    a = np.abs(np.asarray(disp, F))
    w = a.shape[1]
    valid = a != INF
    mn, mx = F(w), F(-w)
    if valid.any():
        mn, mx = min(mn, a[valid].min()), max(mx, a[valid].max())
    out = np.zeros(a.shape, np.uint8)
    if mx > mn:
        with np.errstate(invalid="ignore"):
            out[valid] = ((a[valid] - F(mn)) / F(mx - mn) * F(255)).astype(np.uint8)  # (in [0, 255]: the cast truncates)
    return out


def depth(disp, calib):
    """(depth float32 [H][W], valid bool [H][W]): s = a + doffs, valid <=> a finite and s > 0, Z = fb / s, +inf where invalid."""
    _, _, _, _, doffs, fb = calib_f32(calib)
    a = np.abs(np.asarray(disp, F))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = a + doffs
        valid = np.isfinite(a) & (s > 0)
        z = np.where(valid, fb / np.where(valid, s, F(1)), INF).astype(F)
    return z, valid


def cloud(disp, left_bgr, calib=None):
    """POINT_DTYPE array: one point per valid pixel in raster order.  Without a calibration the reference's rows (x, y, |d|), valid
    <=> |d| != +inf (SaveDisparityCloud, main.cpp:212-230); with one X = ((x - cx) * Z) / f, Y = ((y - cy) * Z) / f, Z, validity of
    depth().  r, g, b from the left image (stored B,G,R); pad = 0."""
    a = np.abs(np.asarray(disp, F))
    h, w = a.shape
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.astype(F), ys.astype(F)
    if calib is None:
        valid, px, py, pz = a != INF, xs, ys, a
    else:
        f, _, cx, cy, _, _ = calib_f32(calib)
        pz, valid = depth(disp, calib)
        with np.errstate(invalid="ignore", over="ignore"):
            px = ((xs - cx) * pz) / f
            py = ((ys - cy) * pz) / f
    pts = np.zeros(int(valid.sum()), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = px[valid], py[valid], pz[valid]  # (boolean indexing walks the array in C order: raster order)
    img = np.asarray(left_bgr, np.uint8).reshape(h, w, 3)
    pts["r"], pts["g"], pts["b"] = img[..., 2][valid], img[..., 1][valid], img[..., 0][valid]
    return pts


def outputs(disp, left_bgr, calib=None):
    """(depth or None, cloud, disp8) of a final map."""
    return (None if calib is None else depth(disp, calib)[0]), cloud(disp, left_bgr, calib), disp8(disp)
