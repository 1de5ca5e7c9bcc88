"""The definition of frame-to-model tracking (include/adcensus_c_api.h: adc_track_device) in numpy: what adcensus_amd/csrc/tsdf_track.h
(tests/emul/emul_tsdf_track.cpp) and the kernels (adcensus_amd/csrc/k_tsdf_track.hip) are held to bit for bit.

The reduce pass: every float operand is np.float32, so every operation rounds once to binary32, in the order the header writes them;
what a pixel contributes is seven integers and every sum is an exact Python / int64 integer.  The solve: Python floats (binary64),
+ - * / only in the header's order, math.sqrt (correctly rounded) for the three numbers of the record no decision reads.

frame: the dict of tests/tsdf_ref.py (kind, calib, R, t: the guess); model: dict(width, height, focal_px, cx, cy, R, t); params: the
dict of `params()` below.  track() returns a dict in the layout of adc_track_result plus the sums of every reduce pass."""
import math

import numpy as np

from tests import register_ref as RR

F = np.float32
Q = F(65536.0)
RANGE = F(4.0)
MAX_PIXELS = 1 << 26
MAX_ITERATIONS_LIMIT = 32
CONVERGED, MAX_ITERATIONS, LOST, DEGENERATE, DIVERGED = range(5)
STATUS_NAMES = ("CONVERGED", "MAX_ITERATIONS", "LOST", "DEGENERATE", "DIVERGED")
COUNT_FIELDS = ("pixels", "no_depth", "outside", "no_model", "too_far", "angle", "out_of_range", "used")
PARAM_FIELDS = ("iterations", "stride", "max_dist", "min_cos", "z_far", "min_pixels", "eps_rot", "eps_trans", "max_rot", "max_trans", "damping", "pivot_ratio")
DEFAULTS = dict(iterations=10, stride=1, max_dist=0.1, min_cos=0.8, z_far=8.0, min_pixels=64, eps_rot=1.0e-5, eps_trans=1.0e-5, max_rot=0.5, max_trans=0.5,
                damping=0.0, pivot_ratio=1.0e-6)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def model(width, height, focal_px, cx, cy, R, t):
    return dict(width=width, height=height, focal_px=focal_px, cx=cx, cy=cy, R=tuple(R), t=tuple(t))


def _rot_t(R, d):
    return [((R[a] * d[0]) + (R[3 + a] * d[1])) + (R[6 + a] * d[2]) for a in range(3)]


def _rot(R, d):
    return [((R[3 * r] * d[0]) + (R[3 * r + 1] * d[1])) + (R[3 * r + 2] * d[2]) for r in range(3)]


def reduce_pass(depth_map, fnormals, fr, mdl, mdepth, mnormals, p, Rk, tk):
    """One reduce pass under the float pose (Rk, tk) -> (sums: 28 Python ints, counts: dict of COUNT_FIELDS, what: the class of every
    participating pixel as an int8 grid, 0 .. 6 in the order of COUNT_FIELDS[1:])."""
    m = np.asarray(depth_map, F)
    H, W = m.shape
    s = int(p["stride"])
    focal, _, cx, cy, _ = (F(v) for v in fr["calib"])
    Rk = [F(v) for v in Rk]
    tk = [F(v) for v in tk]
    Rm = [F(v) for v in mdl["R"]]
    tm = [F(v) for v in mdl["t"]]
    fm, cxm, cym = F(mdl["focal_px"]), F(mdl["cx"]), F(mdl["cy"])
    mw, mh = mdl["width"], mdl["height"]
    md = np.asarray(mdepth, F).reshape(mh, mw)
    mn = np.asarray(mnormals, F).reshape(mh, mw, 4)
    z_far, max_dist = F(p["z_far"]), F(p["max_dist"])
    max_dist2 = max_dist * max_dist
    min_cos = F(p["min_cos"])
    ys, xs = np.meshgrid(np.arange(0, H, s), np.arange(0, W, s), indexing="ij")
    what = np.full(ys.shape, -1, np.int8)
    with np.errstate(all="ignore"):
        Zall, valid = RR.source_z(m, fr["kind"], fr["calib"])
        Z, ok = Zall[ys, xs], valid[ys, xs]
        ok = ok & (Z <= z_far)
        what[~ok] = 0
        Z = np.where(ok, Z, F(1))
        Pc = [((xs.astype(F) - cx) / focal) * Z, ((ys.astype(F) - cy) / focal) * Z, Z]
        d = [Pc[a] - tk[a] for a in range(3)]
        Pw = _rot_t(Rk, d)
        Pm = [v + tm[a] for a, v in enumerate(_rot(Rm, Pw))]
        front = np.isfinite(Pm[2]) & (Pm[2] > 0)
        rz = F(1.0) / np.where(front, Pm[2], F(1))
        pu = ((Pm[0] * fm) * rz) + cxm
        pv = ((Pm[1] * fm) * rz) + cym
        inr = front & (np.abs(pu) < F(32768.0)) & (np.abs(pv) < F(32768.0))
        xm = np.floor(np.where(inr, pu, F(0)) + F(0.5)).astype(np.int64)
        ym = np.floor(np.where(inr, pv, F(0)) + F(0.5)).astype(np.int64)
        inr &= (xm >= 0) & (xm < mw) & (ym >= 0) & (ym < mh)
        what[ok & ~inr] = 1
        ok &= inr
        xm, ym = np.where(ok, xm, 0), np.where(ok, ym, 0)
        Dm = md[ym, xm]
        nm = [mn[ym, xm, a] for a in range(4)]
        has = (Dm > 0) & (nm[3] > 0)
        what[ok & ~has] = 2
        ok &= has
        Qm = [((xm.astype(F) - cxm) / fm) * Dm, ((ym.astype(F) - cym) / fm) * Dm, Dm]
        df = [Pm[a] - Qm[a] for a in range(3)]
        d2 = ((df[0] * df[0]) + (df[1] * df[1])) + (df[2] * df[2])
        near = d2 <= max_dist2
        what[ok & ~near] = 3
        ok &= near
        if fnormals is not None:
            fn = np.asarray(fnormals, F).reshape(H, W, 4)[ys, xs]
            nr = _rot(Rm, _rot_t(Rk, [fn[..., 0], fn[..., 1], fn[..., 2]]))
            dot = ((nr[0] * nm[0]) + (nr[1] * nm[1])) + (nr[2] * nm[2])
            fails = (fn[..., 3] > 0) & ~(dot >= min_cos)
            what[ok & fails] = 4
            ok &= ~fails
        r = ((nm[0] * df[0]) + (nm[1] * df[1])) + (nm[2] * df[2])
        c = [(Pm[1] * nm[2]) - (Pm[2] * nm[1]), (Pm[2] * nm[0]) - (Pm[0] * nm[2]), (Pm[0] * nm[1]) - (Pm[1] * nm[0])]
        sv = [c[0] / z_far, c[1] / z_far, c[2] / z_far, nm[0], nm[1], nm[2], r / max_dist]
        inside = np.ones(ys.shape, bool)
        for v in sv:
            inside &= np.abs(v) < RANGE
        what[ok & ~inside] = 5
        ok &= inside
        what[ok] = 6
        q = [np.rint(np.where(ok, v, F(0)) * Q).astype(np.int64)[ok] for v in sv]
    assert (what >= 0).all()
    sums = []
    for i in range(6):
        for j in range(i, 6):
            sums.append(int((q[i] * q[j]).sum()))
    for i in range(6):
        sums.append(int((q[i] * q[6]).sum()))
    sums.append(int((q[6] * q[6]).sum()))
    assert all(abs(v) < 2 ** 62 for v in sums) and what.size <= MAX_PIXELS
    counts = dict(pixels=int(what.size))
    for i, name in enumerate(COUNT_FIELDS[1:]):
        counts[name] = int((what == i).sum())
    return sums, counts, what


def _mat3(A, B):
    return [((A[3 * i] * B[j]) + (A[3 * i + 1] * B[3 + j])) + (A[3 * i + 2] * B[6 + j]) for i in range(3) for j in range(3)]


def _compose(a, b):
    R = _mat3(a[0], b[0])
    t = [(((a[0][3 * i] * b[1][0]) + (a[0][3 * i + 1] * b[1][1])) + (a[0][3 * i + 2] * b[1][2])) + a[1][i] for i in range(3)]
    return R, t


def _inverse(a):
    R = [a[0][3 * j + i] for i in range(3) for j in range(3)]
    t = [-(((R[3 * i] * a[1][0]) + (R[3 * i + 1] * a[1][1])) + (R[3 * i + 2] * a[1][2])) for i in range(3)]
    return R, t


def _f(v):
    """a double rounded once to float, back as a Python float"""
    with np.errstate(all="ignore"):
        return float(F(v))


def _div(a, b):
    """IEEE division of doubles (Python raises where IEEE gives inf / NaN)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _finite(v):
    return v - v == 0.0


def solve(sums, counts, p, mdl, Rk, tk):
    """One solve -> dict(status or None (go on), R, t (floats as Python floats), H (36), b (6), record (used, rms, rot, trans))"""
    used = counts["used"]
    inv_q = 1.0 / 65536.0
    zs, rs = float(F(p["z_far"])) * inv_q, float(F(p["max_dist"])) * inv_q
    sc = [zs, zs, zs, inv_q, inv_q, inv_q]
    H = [0.0] * 36
    n = 0
    for i in range(6):
        for j in range(i, 6):
            v = (float(sums[n]) * sc[i]) * sc[j]
            n += 1
            H[6 * i + j] = v
            H[6 * j + i] = v
    b = [(float(sums[21 + i]) * sc[i]) * rs for i in range(6)]
    rms = _f(math.sqrt(((float(sums[27]) * rs) * rs) / float(used))) if used else 0.0
    out = dict(status=None, R=[_f(v) for v in Rk], t=[_f(v) for v in tk], H=H, b=b, record=[used, rms, 0.0, 0.0])
    if used < p["min_pixels"]:
        out["status"] = LOST
        return out
    damping, ratio = float(F(p["damping"])), float(F(p["pivot_ratio"]))
    diag = [H[7 * i] + (damping * H[7 * i]) for i in range(6)]
    L = [0.0] * 36
    D = [0.0] * 6
    for j in range(6):
        dj = diag[j]
        for c in range(j):
            dj = dj - ((L[6 * j + c] * L[6 * j + c]) * D[c])
        if not (_finite(dj) and dj > ratio * diag[j]):
            out["status"] = DEGENERATE
            return out
        D[j] = dj
        for i in range(j + 1, 6):
            v = H[6 * i + j]
            for c in range(j):
                v = v - ((L[6 * i + c] * L[6 * j + c]) * D[c])
            L[6 * i + j] = _div(v, dj)
    xi = [0.0] * 6
    for i in range(6):
        v = -b[i]
        for c in range(i):
            v = v - (L[6 * i + c] * xi[c])
        xi[i] = v
    xi = [_div(xi[i], D[i]) for i in range(6)]
    for i in range(5, -1, -1):
        v = xi[i]
        for c in range(i + 1, 6):
            v = v - (L[6 * c + i] * xi[c])
        xi[i] = v
    w2 = ((xi[0] * xi[0]) + (xi[1] * xi[1])) + (xi[2] * xi[2])
    v2 = ((xi[3] * xi[3]) + (xi[4] * xi[4])) + (xi[5] * xi[5])
    out["record"][2] = _f(math.sqrt(w2)) if w2 >= 0 and _finite(w2) else _f(w2 if w2 != w2 else math.inf)
    out["record"][3] = _f(math.sqrt(v2)) if v2 >= 0 and _finite(v2) else _f(v2 if v2 != v2 else math.inf)
    max_rot, max_trans = float(F(p["max_rot"])), float(F(p["max_trans"]))
    if not (w2 <= max_rot * max_rot) or not (v2 <= max_trans * max_trans):
        out["status"] = DIVERGED
        return out
    a = [xi[0] * 0.5, xi[1] * 0.5, xi[2] * 0.5]
    aa = ((a[0] * a[0]) + (a[1] * a[1])) + (a[2] * a[2])
    den, one = 1.0 + aa, 1.0 - aa
    X = [0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0]
    dR = [_div(((one if i == j else 0.0) + (2.0 * (a[i] * a[j]))) + (2.0 * X[3 * i + j]), den) for i in range(3) for j in range(3)]
    dT = (dR, [xi[3], xi[4], xi[5]])
    Tk = ([float(F(v)) for v in Rk], [float(F(v)) for v in tk])
    Tm = ([float(F(v)) for v in mdl["R"]], [float(F(v)) for v in mdl["t"]])
    T3 = _compose(_compose(_compose(Tk, _inverse(Tm)), _inverse(dT)), Tm)
    Rt = [T3[0][3 * j + i] for i in range(3) for j in range(3)]
    G = _mat3(Rt, T3[0])
    B = [((3.0 if i == j else 0.0) - G[3 * i + j]) * 0.5 for i in range(3) for j in range(3)]
    out["R"] = [_f(v) for v in _mat3(T3[0], B)]
    out["t"] = [_f(v) for v in T3[1]]
    eps_rot, eps_trans = float(F(p["eps_rot"])), float(F(p["eps_trans"]))
    if w2 < eps_rot * eps_rot and v2 < eps_trans * eps_trans:
        out["status"] = CONVERGED
    return out


def track(depth_map, fnormals, fr, mdl, mdepth, mnormals, p):
    """The whole loop -> dict(status, solves, R, t, counts (dict), H, b, iteration (list of [used, rms, rot, trans], one per solve),
    sums (list of the 28 sums of every reduce pass))"""
    Rk, tk = [float(F(v)) for v in fr["R"]], [float(F(v)) for v in fr["t"]]
    res = dict(status=MAX_ITERATIONS, solves=0, iteration=[], sums=[])
    for k in range(p["iterations"]):
        sums, counts, _ = reduce_pass(depth_map, fnormals, fr, mdl, mdepth, mnormals, p, Rk, tk)
        s = solve(sums, counts, p, mdl, Rk, tk)
        res["solves"] = k + 1
        res["counts"], res["H"], res["b"] = counts, s["H"], s["b"]
        res["iteration"].append(s["record"])
        res["sums"].append(sums)
        Rk, tk = s["R"], s["t"]
        if s["status"] is not None:
            res["status"] = s["status"]
            break
    res["R"], res["t"] = Rk, tk
    return res


def result_bytes(res):
    """the 960 bytes of the adc_track_result of a reference result"""
    out = np.zeros(960, np.uint8)
    out[0:8].view(np.uint32)[:] = (res["status"], res["solves"])
    out[8:56].view(F)[:] = list(res["R"]) + list(res["t"])
    out[56:88].view(np.uint32)[:] = [res["counts"][k] for k in COUNT_FIELDS]
    out[88:424].view(np.float64)[:] = list(res["H"]) + list(res["b"])
    for i, rec in enumerate(res["iteration"]):
        out[424 + 16 * i:428 + 16 * i].view(np.uint32)[:] = rec[0]
        out[428 + 16 * i:440 + 16 * i].view(F)[:] = rec[1:]
    return out.tobytes()
