"""The definition of the stereo-aware TSDF fusion (include/adcensus_c_api.h: adc_tsdf_weights_device, adc_tsdf_fuse_device) in numpy:
what adcensus_amd/csrc/tsdf_fuse.h (tests/emul/emul_tsdf_fuse.cpp) and the kernels (adcensus_amd/csrc/k_tsdf_fuse.hip) are held to bit
for bit.  The conventions are those of tests/tsdf_ref.py, whose helpers are used: every float operand is np.float32, so every
operation rounds once to binary32 in the order the header writes them; what a voxel accumulates is an integer (Python-exact int64 /
object arithmetic where the numerator passes 2^32).

weight params: dict(class_weight (4), min_confidence, flags, depth_power, z_ref); fuse params: dict(flags, interp_gap)."""
import numpy as np

from tests import register_ref as RR
from tests import tsdf_ref as T

F = T.F
Q = T.Q
W_SCALE_CONFIDENCE = 1
FUSE_BILINEAR = 1
FILL_WTA, FILL_VOTING, FILL_INTERPOLATION, FILL_NONE = 0, 1, 2, 3
PROV_FILL_SHIFT = 2
PROV_SPECKLE = 0x10
WEIGHT_FIELDS = ("valid", "nonzero", "below_confidence", "saturated")
FUSE_FIELDS = ("in_frustum", "no_depth", "unweighted", "occluded", "updated", "interpolated")


def weight_params(class_weight=(16, 4, 1, 0), min_confidence=0.0, flags=0, depth_power=4, z_ref=1.0):
    return dict(class_weight=tuple(class_weight), min_confidence=min_confidence, flags=flags, depth_power=depth_power, z_ref=z_ref)


def fuse_params(flags=0, interp_gap=0.0):
    return dict(flags=flags, interp_gap=interp_gap)


def weights(depth_map, fr, wp=None, provenance=None, confidence=None):
    """-> (weight uint8 [H][W], report dict)"""
    wp = weight_params() if wp is None else wp
    m = np.asarray(depth_map, F)
    D, valid = RR.source_z(m, fr["kind"], fr["calib"])
    if provenance is None:
        fill = np.zeros(m.shape, np.int64)
        speckle = np.zeros(m.shape, bool)
    else:
        code = np.asarray(provenance, np.uint8).astype(np.int64)
        fill = (code >> PROV_FILL_SHIFT) & 3
        speckle = (code & PROV_SPECKLE) != 0
    wc = np.asarray(wp["class_weight"], np.int64)[fill]
    wc = np.where(speckle, 0, wc)
    below = np.zeros(m.shape, bool)
    with np.errstate(all="ignore"):
        if confidence is not None:
            conf = np.asarray(confidence, F)
            tested = fill == FILL_WTA
            below = valid & tested & ~(conf >= F(wp["min_confidence"]))
            wc = np.where(tested & ~(conf >= F(wp["min_confidence"])), 0, wc)
            if wp["flags"] & W_SCALE_CONFIDENCE:
                clipped = np.minimum(np.maximum(np.where(np.isnan(conf), F(0), conf), F(0.0)), F(1.0))
                cq = np.floor(clipped * F(256.0) + F(0.5)).astype(np.int64)
                wc = np.where(tested, (wc * cq + 128) >> 8, wc)
        live = valid & (wc != 0) & np.isfinite(D)
        g = F(wp["z_ref"]) / np.where(live, D, F(1.0))
        s = wc.astype(F)
        if wp["depth_power"] == 2:
            s = s * (g * g)
        elif wp["depth_power"] == 4:
            s = s * ((g * g) * (g * g))
        elif wp["depth_power"] != 0:
            raise ValueError("depth_power")
        w = np.floor(np.minimum(np.where(live, s, F(0)), F(255.0)) + F(0.5)).astype(np.int64)
    w = np.where(live, w, 0)
    rep = dict(valid=int(valid.sum()), nonzero=int((w > 0).sum()), below_confidence=int(below.sum()), saturated=int((w == 255).sum()))
    return w.astype(np.uint8), rep


def fuse(volume, p, fr, depth_map, image=None, weight=None, fp=None):
    """One frame -> (new volume, report dict).  The volume given is left unchanged."""
    fp = fuse_params() if fp is None else fp
    tsdf, color = volume
    tsdf = tsdf.copy()
    color = None if color is None else color.copy()
    if image is not None and color is None:
        raise ValueError("an image needs a colour volume")
    m = np.asarray(depth_map, F)
    H, W = m.shape
    focal, _, cx, cy, _ = (F(v) for v in fr["calib"])
    R = [F(v) for v in fr["R"]]
    t = [F(v) for v in fr["t"]]
    trunc, inv_trunc = F(p["trunc"]), F(1.0) / F(p["trunc"])
    xw, yw, zw = T.centres(p)
    xw, yw, zw = xw[None, None, :], yw[None, :, None], zw[:, None, None]
    with np.errstate(all="ignore"):
        Xc = ((R[0] * xw + R[1] * yw) + R[2] * zw) + t[0]
        Yc = ((R[3] * xw + R[4] * yw) + R[5] * zw) + t[1]
        Zc = ((R[6] * xw + R[7] * yw) + R[8] * zw) + t[2]
        ok = np.isfinite(Zc) & (Zc > 0) & (F(p["z_min"]) <= Zc) & (Zc <= F(p["z_max"]))
        rz = F(1.0) / np.where(ok, Zc, F(1.0))
        u = ((Xc * focal) * rz) + cx
        v = ((Yc * focal) * rz) + cy
        ok &= (np.abs(u) < F(32768.0)) & (np.abs(v) < F(32768.0))
        u, v = np.where(ok, u, F(0)), np.where(ok, v, F(0))
        x = np.floor(u + F(0.5)).astype(np.int64)
        y = np.floor(v + F(0.5)).astype(np.int64)
        ok &= (x >= 0) & (x < W) & (y >= 0) & (y < H)
        x, y = np.where(ok, x, 0), np.where(ok, y, 0)
        Z, valid = RR.source_z(m, fr["kind"], fr["calib"])
        D, has = Z[y, x], valid[y, x]
        no_depth = ok & ~has
        wo = np.ones(x.shape, np.int64) if weight is None else np.asarray(weight, np.uint8).astype(np.int64)[y, x]
        unweighted = ok & has & (wo == 0)
        seen = ok & has & (wo != 0)
        interp = np.zeros(x.shape, bool)
        if fp["flags"] & FUSE_BILINEAR:
            x0 = np.floor(u).astype(np.int64)
            y0 = np.floor(v).astype(np.int64)
            inside = seen & (x0 >= 0) & (x0 + 1 < W) & (y0 >= 0) & (y0 + 1 < H)
            x0s, y0s = np.where(inside, x0, 0), np.where(inside, y0, 0)
            x1s, y1s = np.where(inside, x0 + 1, 0), np.where(inside, y0 + 1, 0)
            a, b, c, d = m[y0s, x0s], m[y0s, x1s], m[y1s, x0s], m[y1s, x1s]
            four = inside & valid[y0s, x0s] & valid[y0s, x1s] & valid[y1s, x0s] & valid[y1s, x1s]
            a, b, c, d = (np.where(four, q_, F(1.0)) for q_ in (a, b, c, d))
            hi = np.maximum(np.maximum(a, b), np.maximum(c, d))
            lo = np.minimum(np.minimum(a, b), np.minimum(c, d))
            gated = four & ((hi - lo) <= F(fp["interp_gap"]))
            fx = u - x0.astype(F)
            fy = v - y0.astype(F)
            top = a + fx * (b - a)
            bot = c + fx * (d - c)
            val = top + fy * (bot - top)
            Zv, vv = RR.source_z(np.where(gated, val, F(1.0)), fr["kind"], fr["calib"])
            interp = gated & vv
            D = np.where(interp, Zv, D)
        sdf = np.where(seen, D, F(0)) - Zc
        occluded = seen & ~(sdf >= -trunc)
        upd = seen & (sdf >= -trunc)
        f = np.minimum(np.where(upd, sdf, F(0)) * inv_trunc, F(1.0))
        q = np.floor(f * F(32767.0) + F(0.5)).astype(np.int64)
        band = upd & (np.abs(sdf) <= trunc)
    told, wold = T.word_t(tsdf), T.word_w(tsdf)
    wo = np.where(upd, wo, 1)
    mm = wold + wo
    num = (told + Q) * wold + (q + Q) * wo + mm // 2  # int64: below 2^33
    assert (num[upd] >= 0).all() and (num[upd] < 2 ** 33).all()
    tn = num // mm - Q
    wn = np.minimum(mm, p["max_weight"])
    tsdf = np.where(upd, T.make_words(tn, wn), tsdf).astype(np.uint32)
    if color is not None and image is not None:
        img = np.asarray(image, np.uint8).astype(np.int64)
        cw = (color >> np.uint32(24)).astype(np.int64)
        cm = cw + 1
        new = np.zeros(color.shape, np.int64)
        for shift, ch in ((0, 2), (8, 1), (16, 0)):  # r, g, b of the word <- image stored B,G,R
            c_ = ((color >> np.uint32(shift)) & np.uint32(0xFF)).astype(np.int64)
            new |= ((c_ * cw + img[y, x, ch] + cm // 2) // cm) << shift
        new |= np.minimum(cm, min(p["max_weight"], 255)) << 24
        color = np.where(band, new.astype(np.uint32), color).astype(np.uint32)
    rep = dict(in_frustum=int(ok.sum()), no_depth=int(no_depth.sum()), unweighted=int(unweighted.sum()), occluded=int(occluded.sum()),
               updated=int(upd.sum()), interpolated=int(interp.sum()))
    return (tsdf, color), rep
