"""The definition of the TSDF volume (include/adcensus_c_api.h: adc_tsdf_integrate_device, adc_tsdf_extract_device) in numpy: what
adcensus_amd/csrc/tsdf_voxel.h (tests/emul/emul_tsdf.cpp) and the kernels (adcensus_amd/csrc/k_tsdf.hip) are held to bit for bit.

Every float operand is np.float32, so every operation rounds once to binary32, in the order the header writes them; everything a
voxel accumulates is an integer (int64 here, below 2^32 by the header's argument).  Validity and Z of a map value are taken from
tests/register_ref.py (source_z).

params: dict(nx, ny, nz, voxel, origin (3), trunc, z_min, z_max, max_weight, flags); frame: dict(kind, calib (focal_px, baseline, cx,
cy, doffs), R (9, row-major), t (3)).  A volume is (tsdf uint32 [nz][ny][nx], color uint32 [nz][ny][nx] or None)."""
import numpy as np

from tests import register_ref as RR

F = np.float32
Q = 32767
COLOR = 1
FROM_DISPARITY, FROM_DEPTH = RR.FROM_DISPARITY, RR.FROM_DEPTH
REPORT_FIELDS = ("in_frustum", "no_depth", "occluded", "updated")
EXTRACT_FIELDS = ("voxels_seen", "points")
POINT_DTYPE = np.dtype([("x", F), ("y", F), ("z", F), ("r", np.uint8), ("g", np.uint8), ("b", np.uint8), ("pad", np.uint8)])
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def params(nx, ny, nz, voxel, origin, trunc, z_min=0.0, z_max=float("inf"), max_weight=64, flags=0):
    return dict(nx=nx, ny=ny, nz=nz, voxel=voxel, origin=tuple(origin), trunc=trunc, z_min=z_min, z_max=z_max, max_weight=max_weight, flags=flags)


def frame(calib, R=IDENTITY, t=(0.0, 0.0, 0.0), kind=FROM_DISPARITY):
    return dict(kind=kind, calib=tuple(calib), R=tuple(R), t=tuple(t))


def empty(p):
    shape = (p["nz"], p["ny"], p["nx"])
    return np.zeros(shape, np.uint32), (np.zeros(shape, np.uint32) if p["flags"] & COLOR else None)


def centres(p):
    """step 1: (xw [nx], yw [ny], zw [nz]) float32"""
    v = F(p["voxel"])
    return tuple(F(p["origin"][a]) + (np.arange(n, dtype=F) + F(0.5)) * v for a, n in enumerate((p["nx"], p["ny"], p["nz"])))


def word_t(words):
    """t of voxel words as int64 (a stored -32768 is read as -32767)"""
    return np.maximum((words & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.int64), -Q)


def word_w(words):
    return (words >> np.uint32(16)).astype(np.int64)


def make_words(t, w):
    return (np.asarray(t, np.int64) & 0xFFFF).astype(np.uint32) | (np.asarray(w, np.int64).astype(np.uint32) << np.uint32(16))


def integrate(volume, p, fr, depth_map, image=None):
    """One frame -> (new volume, report dict).  The volume given is left unchanged."""
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
    xw, yw, zw = centres(p)
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
        x = np.floor(np.where(ok, u, F(0)) + F(0.5)).astype(np.int64)
        y = np.floor(np.where(ok, v, F(0)) + F(0.5)).astype(np.int64)
        ok &= (x >= 0) & (x < W) & (y >= 0) & (y < H)
        x, y = np.where(ok, x, 0), np.where(ok, y, 0)
        Z, valid = RR.source_z(m, fr["kind"], fr["calib"])
        D, has = Z[y, x], valid[y, x]
        no_depth = ok & ~has
        sdf = np.where(ok & has, D, F(0)) - Zc
        seen = ok & has
        occluded = seen & ~(sdf >= -trunc)
        upd = seen & (sdf >= -trunc)
        f = np.minimum(np.where(upd, sdf, F(0)) * inv_trunc, F(1.0))
        q = np.floor(f * F(32767.0) + F(0.5)).astype(np.int64)
        band = upd & (np.abs(sdf) <= trunc)
    told, wold = word_t(tsdf), word_w(tsdf)
    mm = wold + 1
    num = (told + Q) * wold + (q + Q) + mm // 2
    assert (num[upd] >= 0).all() and (num[upd] < 2 ** 32).all()
    tn = num // mm - Q
    wn = np.minimum(mm, p["max_weight"])
    tsdf = np.where(upd, make_words(tn, wn), tsdf).astype(np.uint32)
    if color is not None and image is not None:
        img = np.asarray(image, np.uint8).astype(np.int64)
        cw = (color >> np.uint32(24)).astype(np.int64)
        cm = cw + 1
        new = np.zeros(color.shape, np.int64)
        for shift, ch in ((0, 2), (8, 1), (16, 0)):  # r, g, b of the word <- image stored B,G,R
            c = ((color >> np.uint32(shift)) & np.uint32(0xFF)).astype(np.int64)
            new |= ((c * cw + img[y, x, ch] + cm // 2) // cm) << shift
        new |= np.minimum(cm, min(p["max_weight"], 255)) << 24
        color = np.where(band, new.astype(np.uint32), color).astype(np.uint32)
    rep = dict(in_frustum=int(ok.sum()), no_depth=int(no_depth.sum()), occluded=int(occluded.sum()), updated=int(upd.sum()))
    return (tsdf, color), rep


def extract(volume, p, min_weight=1, capacity=None):
    """-> (points POINT_DTYPE [n] in the definition's order, report dict); capacity None: ALL points, else the first min(points,
    capacity) of them -- the report counts every crossing whatever the capacity"""
    tsdf, color = volume
    nz, ny, nx = tsdf.shape
    t, w = word_t(tsdf), word_w(tsdf)
    seen = w >= min_weight
    neg = t < 0
    cen = centres(p)
    voxel = F(p["voxel"])
    n_of = np.arange(nx * ny * nz, dtype=np.int64).reshape(nz, ny, nx)
    recs = []
    for axis, np_axis in ((0, 2), (1, 1), (2, 0)):  # x is the last numpy axis
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[np_axis], b[np_axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        cross = seen[a] & seen[b] & (neg[a] != neg[b])
        idx = np.nonzero(cross)
        ta, tb = t[a][idx].astype(F), t[b][idx].astype(F)
        with np.errstate(all="ignore"):
            s = ta / (ta - tb)
        k, j, i = idx
        pos = [cen[0][i], cen[1][j], cen[2][k]]
        pos[axis] = pos[axis] + s * voxel
        out = np.zeros(len(s), POINT_DTYPE)
        out["x"], out["y"], out["z"] = pos
        if color is not None:
            c = np.where(s <= F(0.5), color[a][idx], color[b][idx])
            out["r"], out["g"], out["b"] = c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF
        out["pad"] = np.minimum(np.minimum(w[a][idx], w[b][idx]), 255)
        recs.append((n_of[a][idx] * 3 + axis, out))
    key = np.concatenate([r[0] for r in recs])
    pts = np.concatenate([r[1] for r in recs])[np.argsort(key, kind="stable")]
    return (pts if capacity is None else pts[:capacity]), dict(voxels_seen=int(seen.sum()), points=len(pts))


def report_words(rep, fields=REPORT_FIELDS):
    return [rep[k] for k in fields]
