"""The definition of the surface normals from a disparity map (include/adcensus_c_api.h: adc_normals_device) in numpy: what
adcensus_amd/csrc/normals_fit.h (tests/emul/emul_normals.cpp) and the kernel (adcensus_amd/csrc/k_normals.hip) are held to bit for bit.

Integers up to the four determinants (int64 arrays: exact), then float32 arrays, one numpy operation per rounding, in the order the
header writes.  An int64 becomes a float through `.astype(np.float32)`: ONE rounding to nearest even (a Python int would go through
double and round twice above 2^53)."""
import numpy as np

F = np.float32
MAX_RADIUS = 7
A_LIMIT = F(32768.0)
SCALE = F(1024.0)
INV_SCALE = F(2.0 ** -10)
DEFAULTS = dict(radius=2, max_diff=1.0, min_points=5)


def gate(max_diff):
    """G = (int32)rintf(max_diff * 1024.0f)"""
    return int(np.rint(F(max_diff) * SCALE))


def quantise(d):
    """-> (usable bool [H][W], q int32 [H][W] with 0 where not usable)"""
    a = np.abs(np.asarray(d, F))
    with np.errstate(invalid="ignore"):
        usable = np.isfinite(a) & (a < A_LIMIT)
    q = np.rint(np.where(usable, a, F(0)) * SCALE).astype(np.int32)
    return usable, q


def sums(d, radius, max_diff):
    """The nine sums over every centre's support as int64 arrays (dict), plus usable and q."""
    usable, q = quantise(d)
    H, W = q.shape
    r, G = int(radius), gate(max_diff)
    qp = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    up = np.zeros((H + 2 * r, W + 2 * r), bool)
    qp[r:r + H, r:r + W] = q
    up[r:r + H, r:r + W] = usable
    s = {k: np.zeros((H, W), np.int64) for k in ("n", "sx", "sy", "sxx", "sxy", "syy", "se", "sxe", "sye")}
    qc = q.astype(np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            e = qp[r + dy:r + dy + H, r + dx:r + dx + W] - qc
            ok = up[r + dy:r + dy + H, r + dx:r + dx + W] & usable & (np.abs(e) <= G)
            e = np.where(ok, e, 0)
            n = ok.astype(np.int64)
            s["n"] += n
            s["sx"] += dx * n
            s["sy"] += dy * n
            s["sxx"] += dx * dx * n
            s["sxy"] += dx * dy * n
            s["syy"] += dy * dy * n
            s["se"] += e
            s["sxe"] += dx * e
            s["sye"] += dy * e
    for k, v in s.items():
        assert np.abs(v).max(initial=0) < 2 ** 31, k  # (every sum fits int32)
    return s, usable, q


def det3(a, b, c, d, e, f, g, h, i):
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)


def normals(d, calib, radius=2, max_diff=1.0, min_points=5):
    """-> (normals float32 [H][W][4], normals8 uint8 [H][W][4], report dict usable / fitted / few_points / degenerate).
    calib: (focal_px, baseline, cx, cy, doffs)."""
    focal, _, cx, cy, doffs = (F(v) for v in calib)
    assert 1 <= radius <= MAX_RADIUS and 0 < max_diff <= 64 and 3 <= min_points <= (2 * radius + 1) ** 2
    s, usable, q = sums(d, radius, max_diff)
    H, W = q.shape
    n, sx, sy, sxx, sxy, syy, se, sxe, sye = (s[k] for k in ("n", "sx", "sy", "sxx", "sxy", "syy", "se", "sxe", "sye"))
    Dt = det3(sxx, sxy, sx, sxy, syy, sy, sx, sy, n)
    Na = det3(sxe, sxy, sx, sye, syy, sy, se, sy, n)
    Nb = det3(sxx, sxe, sx, sxy, sye, sy, sx, se, n)
    Nc = det3(sxx, sxy, sxe, sxy, syy, sye, sx, sy, se)
    assert (Dt >= 0).all() and max(np.abs(Na).max(initial=0), np.abs(Nb).max(initial=0), np.abs(Nc).max(initial=0)) < 2 ** 57
    enough = usable & (n >= min_points)
    solvable = enough & (Dt > 0)
    Df = np.where(solvable, Dt, 1).astype(F)
    y, x = np.meshgrid(np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32), indexing="ij")
    with np.errstate(all="ignore"):
        ga = (Na.astype(F) / Df) * INV_SCALE
        gb = (Nb.astype(F) / Df) * INV_SCALE
        dc = (q.astype(F) * INV_SCALE) + ((Nc.astype(F) / Df) * INV_SCALE)
        sd = dc + doffs
        nx = ga * focal
        ny = gb * focal
        nz = ((ga * (cx - x.astype(F))) + (gb * (cy - y.astype(F)))) + sd
        L = np.sqrt(((nx * nx) + (ny * ny)) + (nz * nz))
        fitted = solvable & (sd > 0) & np.isfinite(L) & (L > 0)
        Ls = np.where(fitted, L, F(1))
        v = np.stack([-nx / Ls, -ny / Ls, -nz / Ls, n.astype(np.int32).astype(F)], axis=-1).astype(F)
    out = np.where(fitted[..., None], v, F(0)).astype(F)
    b = (np.rint(out[..., :3] * F(127.0)).astype(np.int32) + 128).astype(np.uint8)
    out8 = np.concatenate([b, np.full((H, W, 1), 255, np.uint8)], axis=-1)
    out8 = np.where(fitted[..., None], out8, np.uint8(0)).astype(np.uint8)
    rep = dict(usable=int(usable.sum()), fitted=int(fitted.sum()), few_points=int((usable & ~enough).sum()), degenerate=int((enough & ~fitted).sum()))
    assert rep["usable"] == rep["fitted"] + rep["few_points"] + rep["degenerate"]
    return np.ascontiguousarray(out), np.ascontiguousarray(out8), rep


def report_words(rep):
    return [rep["usable"], rep["fitted"], rep["few_points"], rep["degenerate"]]
