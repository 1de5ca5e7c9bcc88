"""The moving TSDF volume in numpy (include/adcensus_c_api.h holds the definition in words, adcensus_amd/csrc/tsdf_shift.h is the rule
the kernels and the serial program share).  A shift s = (sx, sy, sz) moves the window by +s voxels in the world: new voxel (i, j, k)
takes the words of old voxel (i + sx, j + sy, k + sz) or becomes empty; an old voxel leaves iff (i - sx, j - sy, k - sz) lies outside
the box; the leaving list is the extraction's list of the OLD volume restricted to crossings with a leaving endpoint.  Volumes are
(tsdf uint32 [nz][ny][nx], color the same or None) as in tests/tsdf_ref.py, which stays the definition of a crossing and its record.
"""
import numpy as np

from tests import tsdf_ref as T

F = np.float32
SHIFT_FIELDS = ("moved_nonempty", "left_nonempty", "left_seen", "points")
MAX_OFFSET = 1 << 24
FOLLOW_MAX_SHIFT = 1 << 30


def shift_params(shift, min_weight=1):
    return dict(shift=tuple(int(v) for v in shift), min_weight=int(min_weight))


def follow_params(anchor=(0.0, 0.0, 2.5), margin=8, quantum=4):
    return dict(anchor=tuple(float(v) for v in anchor), margin=int(margin), quantum=int(quantum))


def leaves(shape, shift):
    """bool [nz][ny][nx]: the old voxels that leave"""
    nz, ny, nx = shape
    out = []
    for n, s in ((nx, shift[0]), (ny, shift[1]), (nz, shift[2])):
        c = np.arange(n, dtype=np.int64) - int(s)
        out.append((c < 0) | (c >= n))
    return out[2][:, None, None] | out[1][None, :, None] | out[0][None, None, :]


def move(plane, shift):
    """the new plane of words"""
    nz, ny, nx = plane.shape
    new = np.zeros_like(plane)
    src = []
    for n, s in ((nx, shift[0]), (ny, shift[1]), (nz, shift[2])):
        c = np.arange(n, dtype=np.int64) + int(s)
        ok = (c >= 0) & (c < n)
        src.append((np.nonzero(ok)[0], c[ok]))
    (di, si), (dj, sj), (dk, sk) = src
    if len(di) and len(dj) and len(dk):
        new[np.ix_(dk, dj, di)] = plane[np.ix_(sk, sj, si)]
    return new


def leaving_list(volume, p, shift, min_weight=1):
    """-> (points POINT_DTYPE [n] in the extraction's order, kinds uint8 [n]: 1 only a leaves, 2 only b, 3 both).  tests/tsdf_ref.extract
    with one more condition per pair; the records are its records (the OLD origin)."""
    tsdf, color = volume
    nz, ny, nx = tsdf.shape
    t, w = T.word_t(tsdf), T.word_w(tsdf)
    seen = w >= min_weight
    neg = t < 0
    lv = leaves(tsdf.shape, shift)
    cen = T.centres(p)
    voxel = F(p["voxel"])
    n_of = np.arange(nx * ny * nz, dtype=np.int64).reshape(nz, ny, nx)
    recs = []
    for axis, np_axis in ((0, 2), (1, 1), (2, 0)):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[np_axis], b[np_axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        cross = seen[a] & seen[b] & (neg[a] != neg[b]) & (lv[a] | lv[b])
        idx = np.nonzero(cross)
        ta, tb = t[a][idx].astype(F), t[b][idx].astype(F)
        with np.errstate(all="ignore"):
            s = ta / (ta - tb)
        k, j, i = idx
        pos = [cen[0][i], cen[1][j], cen[2][k]]
        pos[axis] = pos[axis] + s * voxel
        out = np.zeros(len(s), T.POINT_DTYPE)
        out["x"], out["y"], out["z"] = pos
        if color is not None:
            c = np.where(s <= F(0.5), color[a][idx], color[b][idx])
            out["r"], out["g"], out["b"] = c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF
        out["pad"] = np.minimum(np.minimum(w[a][idx], w[b][idx]), 255)
        kind = (lv[a][idx].astype(np.uint8) | (lv[b][idx].astype(np.uint8) << 1))
        recs.append((n_of[a][idx] * 3 + axis, out, kind))
    order = np.argsort(np.concatenate([r[0] for r in recs]), kind="stable")
    return np.concatenate([r[1] for r in recs])[order], np.concatenate([r[2] for r in recs])[order]


def origin_after(origin0, offset, voxel):
    """binary32: one multiply, one add, from the total offset"""
    return tuple(float(F(origin0[a]) + F(np.float32(int(offset[a])) * F(voxel))) for a in range(3))


def offset_refused(offset, shift):
    return any(abs(int(offset[a]) + int(shift[a])) > MAX_OFFSET for a in range(3))


def shift(volume, p, sp, offset=(0, 0, 0), origin0=None, capacity=None):
    """One shift -> (new volume, new params, new offset, points, report dict).  p holds the CURRENT origin; origin0 (default: p's origin
    with a zero offset) is the origin at creation.  The volume given is left unchanged."""
    tsdf, color = volume
    s, mw = sp["shift"], sp["min_weight"]
    origin0 = tuple(p["origin"]) if origin0 is None else tuple(origin0)
    assert not offset_refused(offset, s)
    if s == (0, 0, 0):
        pts = np.zeros(0, T.POINT_DTYPE)
        return (tsdf.copy(), None if color is None else color.copy()), dict(p), tuple(offset), pts, dict.fromkeys(SHIFT_FIELDS, 0)
    pts, _ = leaving_list(volume, p, s, mw)
    lv = leaves(tsdf.shape, s)
    new = (move(tsdf, s), None if color is None else move(color, s))
    rep = dict(moved_nonempty=int((new[0] != 0).sum()), left_nonempty=int(((tsdf != 0) & lv).sum()), left_seen=int(((T.word_w(tsdf) >= mw) & lv).sum()),
               points=len(pts))
    noff = tuple(int(offset[a]) + int(s[a]) for a in range(3))
    q = dict(p)
    q["origin"] = origin_after(origin0, noff, p["voxel"])
    return new, q, noff, (pts if capacity is None else pts[:capacity]), rep


def follow_plan(p, R, t, fp):
    """the follow rule in binary64, in the written order"""
    anchor, margin, quantum = fp["anchor"], fp["margin"], fp["quantum"]
    d = [np.float64(F(anchor[a])) - np.float64(F(t[a])) for a in range(3)]
    R = [np.float64(F(v)) for v in R]
    n = (p["nx"], p["ny"], p["nz"])
    out = []
    for a in range(3):
        A = (R[a] * d[0] + R[3 + a] * d[1]) + R[6 + a] * d[2]
        c = (A - np.float64(F(p["origin"][a]))) / np.float64(F(p["voxel"])) - np.float64(n[a]) / np.float64(2.0)
        v = np.float64(0.0)
        if abs(c) > margin:
            v = np.float64(quantum) * np.trunc(c / np.float64(quantum))
        out.append(int(min(max(v, -FOLLOW_MAX_SHIFT), FOLLOW_MAX_SHIFT)))
    return tuple(out)


def report_words(rep):
    return [rep[k] for k in SHIFT_FIELDS]
