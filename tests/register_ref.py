"""The definition of the registration of depth into a second camera (include/adcensus_c_api.h: adc_register_depth_device,
adc_align_color_device) in numpy: every operation on float32 arrays, one rounding each, in the order the header writes them.  The
kernels (adcensus_amd/csrc/k_register.hip) and the serial program built from the shared header (tests/emul/emul_register.cpp) are
held to these functions bit for bit.

A target is anything with the fields of adc_reg_target (adcensus_amd.RegTarget); a calibration is (focal_px, baseline, cx, cy, doffs)."""
import numpy as np

F = np.float32
FROM_DISPARITY, FROM_DEPTH = 0, 1
MAX_SPLAT = 8
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _calib(calib):
    if hasattr(calib, "focal_px"):
        calib = (calib.focal_px, calib.baseline, calib.cx, calib.cy, calib.doffs)
    return tuple(F(v) for v in calib)


def source_z(m, kind, calib):
    """(Z float32 [H][W], valid bool [H][W]) of a map."""
    focal, baseline, _, _, doffs = _calib(calib)
    m = np.asarray(m, F)
    with np.errstate(all="ignore"):
        if kind == FROM_DEPTH:
            return m, np.isfinite(m) & (m > 0)
        a = np.abs(m)
        s = a + doffs
        ok = np.isfinite(a) & (s > 0)
        fb = F(focal * baseline)
        return np.where(ok, fb / np.where(ok, s, F(1)), F(np.inf)).astype(F), ok


def project(calib, T, xs, ys, Z):
    """The source points (xs, ys, Z) in the target image: (u, v, Zt, ok), ok = in front and in range."""
    focal, _, cx, cy, _ = _calib(calib)
    R = [F(v) for v in T.R]
    t = [F(v) for v in T.t]
    k1, k2, p1, p2, k3 = F(T.k1), F(T.k2), F(T.p1), F(T.p2), F(T.k3)
    two = F(2)
    with np.errstate(all="ignore"):
        X = ((xs - cx) * Z) / focal
        Y = ((ys - cy) * Z) / focal
        Xt = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]
        Yt = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
        Zt = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
        front = np.isfinite(Zt) & (Zt > 0)
        x, y = Xt / Zt, Yt / Zt
        x2, y2 = x * x, y * y
        r2, xy = x2 + y2, x * y
        rad = F(1) + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = (x * rad + (two * p1) * xy) + p2 * (r2 + two * x2)
        yd = (y * rad + p1 * (r2 + two * y2)) + (two * p2) * xy
        u = F(T.fx) * xd + F(T.cx)
        v = F(T.fy) * yd + F(T.cy)
        ok = front & (np.abs(u) < F(32768)) & (np.abs(v) < F(32768))
    for a in (X, Xt, Zt, x, rad, xd, u):
        assert a.dtype == F
    return u, v, Zt, ok


def _extent(a, b, c, ok, splat, n):
    with np.errstate(all="ignore"):
        if splat:
            lo = np.where(ok, np.ceil(np.minimum(a, b)), 0).astype(np.int64)
            hi = np.where(ok, np.ceil(np.maximum(a, b)), 0).astype(np.int64) - 1
        else:
            lo = np.where(ok, np.floor(c + F(0.5)), 0).astype(np.int64)
            hi = lo.copy()
    lo = np.maximum(lo, 0)
    hi = np.minimum(hi, n - 1)
    hi = np.minimum(hi, lo + MAX_SPLAT - 1)
    return lo, hi


def footprints(m, kind, calib, T, splat=True):
    """Per source pixel: valid, projected (non-empty footprint), Zc and the inclusive ranges j0, j1, i0, i1."""
    Z, valid = source_z(m, kind, calib)
    H, W = Z.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    half = F(0.5)
    uc, vc, zc, okc = project(calib, T, xs, ys, Z)
    ua, va, _, oka = project(calib, T, xs - half, ys - half, Z)
    ub, vb, _, okb = project(calib, T, xs + half, ys + half, Z)
    ok = valid & okc & oka & okb
    j0, j1 = _extent(ua, ub, uc, ok, splat, int(T.width))
    i0, i1 = _extent(va, vb, vc, ok, splat, int(T.height))
    proj = ok & (j0 <= j1) & (i0 <= i1)
    return dict(valid=valid, projected=proj, zc=zc, j0=j0, j1=j1, i0=i0, i1=i1)


def register(m, kind, calib, T, splat=True):
    """-> depth float32 [Ht][Wt], index int32 [Ht][Wt], report dict (src_valid, src_projected, dst_filled, and -- not part of the ABI --
    candidates: keys sent to the z-buffer, tied: target pixels that received two different keys with the same depth bits)."""
    fp = footprints(m, kind, calib, T, splat)
    H, W = fp["valid"].shape
    Wt, Ht = int(T.width), int(T.height)
    zbuf = np.full(Ht * Wt, EMPTY, np.uint64)
    sel = np.flatnonzero(fp["projected"].ravel())
    key = (fp["zc"].ravel()[sel].view(np.uint32).astype(np.uint64) << np.uint64(32)) | sel.astype(np.uint64)
    j0, j1, i0, i1 = (fp[k].ravel()[sel] for k in ("j0", "j1", "i0", "i1"))
    sent = []
    for di in range(MAX_SPLAT):
        for dj in range(MAX_SPLAT):
            on = (i0 + di <= i1) & (j0 + dj <= j1)
            if not on.any():
                continue
            at = (i0[on] + di) * Wt + (j0[on] + dj)
            np.minimum.at(zbuf, at, key[on])
            sent.append((at, key[on]))
    hit = zbuf != EMPTY
    depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(F), F(np.inf)).astype(F).reshape(Ht, Wt)
    index = np.where(hit, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32).reshape(Ht, Wt)
    candidates, tied = 0, 0
    if sent:
        at = np.concatenate([s[0] for s in sent])
        ky = np.concatenate([s[1] for s in sent])
        candidates = int(at.size)
        lost = ky != zbuf[at]
        tied = int(np.unique(at[lost & ((ky >> np.uint64(32)) == (zbuf[at] >> np.uint64(32)))]).size)
    rep = dict(src_valid=int(fp["valid"].sum()), src_projected=int(fp["projected"].sum()), dst_filled=int(hit.sum()), candidates=candidates, tied=tied)
    return depth, index, rep


def align(m, kind, calib, T, target_bgr):
    """Colour aligned to depth -> (bgr uint8 [H][W][3], valid uint8 [H][W])."""
    Z, valid = source_z(m, kind, calib)
    H, W = Z.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    uc, vc, _, ok = project(calib, T, xs, ys, Z)
    ok = ok & valid
    with np.errstate(all="ignore"):
        j = np.where(ok, np.floor(uc + F(0.5)), -1).astype(np.int64)
        i = np.where(ok, np.floor(vc + F(0.5)), -1).astype(np.int64)
    ok = ok & (j >= 0) & (j < int(T.width)) & (i >= 0) & (i < int(T.height))
    t = np.asarray(target_bgr, np.uint8).reshape(int(T.height), int(T.width), 3)
    out = np.where(ok[..., None], t[np.where(ok, i, 0), np.where(ok, j, 0)], 0).astype(np.uint8)
    return out, ok.astype(np.uint8)


def report_words(rep):
    return [rep["src_valid"], rep["src_projected"], rep["dst_filled"], 0]
