"""The definition of the TSDF volume's ray cast (include/adcensus_c_api.h: adc_tsdf_raycast_device) in numpy: what
adcensus_amd/csrc/tsdf_ray.h (tests/emul/emul_tsdf_raycast.cpp) and the kernel (adcensus_amd/csrc/k_tsdf_raycast.hip) are held to bit
for bit.  Vectorised over the rays, sequential in the samples of a ray.

Every float operand is np.float32, so every operation rounds once to binary32, in the order the header writes them.  A volume is
(tsdf uint32 [nz][ny][nx], color uint32 [nz][ny][nx] or None) with the parameters of tests/tsdf_ref.py; a view is a dict(width,
height, focal_px, cx, cy, R (9, row-major), t (3), z_near, z_far, step, skip, min_weight, max_steps)."""
import numpy as np

from tests import tsdf_ref as T

F = np.float32
Q = T.Q
MISS, HIT, NO_SURFACE, BEHIND, EXHAUSTED = range(5)
STATUS_NAMES = ("miss", "hit", "no_surface", "behind", "exhausted")
REPORT_FIELDS = ("rays",) + STATUS_NAMES + ("samples_lo", "samples_hi")
CORNERS = tuple((c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8))


def view(width, height, focal_px, cx, cy, R=T.IDENTITY, t=(0.0, 0.0, 0.0), z_near=0.05, z_far=100.0, step=0.025, skip=None, min_weight=1, max_steps=4096):
    return dict(width=width, height=height, focal_px=focal_px, cx=cx, cy=cy, R=tuple(R), t=tuple(t), z_near=z_near, z_far=z_far, step=step,
                skip=step if skip is None else skip, min_weight=min_weight, max_steps=max_steps)


def _lerp(lo, hi, frac):
    return lo + (frac * (hi - lo))


class _Rays:
    """the rays of a view in grid coordinates and their clipped ranges (all pixels, raster order)"""

    def __init__(self, p, v):
        W, H = v["width"], v["height"]
        x = np.tile(np.arange(W, dtype=F), H)
        y = np.repeat(np.arange(H, dtype=F), W)
        focal, cx, cy = F(v["focal_px"]), F(v["cx"]), F(v["cy"])
        R = [F(a) for a in v["R"]]
        t = [F(a) for a in v["t"]]
        inv_voxel = F(1.0) / F(p["voxel"])
        self.n = (p["nx"], p["ny"], p["nz"])
        dx = (x - cx) / focal
        dy = (y - cy) / focal
        N = W * H
        self.g0, self.gd = [], []
        z_lo, z_hi = np.full(N, F(v["z_near"])), np.full(N, F(v["z_far"]))
        miss = np.zeros(N, bool)
        for a in range(3):
            dw = ((R[a] * dx) + (R[3 + a] * dy)) + R[6 + a]
            cc = -(((R[a] * t[0]) + (R[3 + a] * t[1])) + (R[6 + a] * t[2]))
            g0 = F(((cc - F(p["origin"][a])) * inv_voxel) - F(0.5))
            gd = dw * inv_voxel
            top = F(self.n[a] - 1)
            fin = np.isfinite(g0) & np.isfinite(gd)
            zero = gd == 0
            miss |= ~fin
            miss |= fin & zero & ~((g0 >= 0) & (g0 <= top))
            act = fin & ~zero
            safe = np.where(act, gd, F(1.0))
            t1 = (F(0.0) - g0) / safe
            t2 = (top - g0) / safe
            tf = np.isfinite(t1) & np.isfinite(t2)
            miss |= act & ~tf
            ok = act & tf
            lo, hi = np.where(t1 < t2, t1, t2), np.where(t1 < t2, t2, t1)
            z_lo = np.where(ok & (lo > z_lo), lo, z_lo)
            z_hi = np.where(ok & (hi < z_hi), hi, z_hi)
            self.g0.append(g0)
            self.gd.append(gd)
        miss |= ~(z_lo <= z_hi)
        self.z_lo, self.z_hi, self.miss = z_lo, z_hi, miss

    def cell(self, idx, Z):
        """step 1 for the rays idx at depths Z -> (inside bool [m], cell int64 [m][3], frac float32 [m][3])"""
        inside = np.ones(len(idx), bool)
        cell = np.zeros((len(idx), 3), np.int64)
        frac = np.zeros((len(idx), 3), F)
        for a in range(3):
            g = self.g0[a] + (Z * self.gd[a][idx])
            ok = np.abs(g) < F(32768.0)
            fl = np.floor(np.where(ok, g, F(0.0)))
            cell[:, a] = np.where(ok, fl.astype(np.int64), -1)
            frac[:, a] = np.where(ok, g - fl, F(0.0))
            inside &= ok & (cell[:, a] >= 0) & (cell[:, a] < self.n[a] - 1)
        return inside, cell, frac


def _index(n, i, j, k):
    return (k * n[1] + j) * n[0] + i


def _nearest(n, cell, frac):
    up = (frac >= F(0.5)).astype(np.int64)
    return _index(n, cell[:, 0] + up[:, 0], cell[:, 1] + up[:, 1], cell[:, 2] + up[:, 2])


def _corners(n, words, cell):
    return np.stack([words[_index(n, cell[:, 0] + di, cell[:, 1] + dj, cell[:, 2] + dk)] for di, dj, dk in CORNERS], -1)


def _trilinear(t, frac):
    a, b, c = frac[:, 0], frac[:, 1], frac[:, 2]
    c00, c10 = _lerp(t[:, 0], t[:, 1], a), _lerp(t[:, 2], t[:, 3], a)
    c01, c11 = _lerp(t[:, 4], t[:, 5], a), _lerp(t[:, 6], t[:, 7], a)
    return _lerp(_lerp(c00, c10, b), _lerp(c01, c11, b), c)


def raycast(volume, p, v):
    """-> dict(depth float32 [H][W], normals float32 [H][W][4], bgr uint8 [H][W][3] (None without a colour volume), status uint8 [H][W],
    samples int64 [H][W], report dict)"""
    tsdf, color = volume
    words = np.ascontiguousarray(tsdf, np.uint32).ravel()
    W, H = v["width"], v["height"]
    N = W * H
    mw, max_steps = v["min_weight"], v["max_steps"]
    step, skip = F(v["step"]), F(v["skip"])
    with np.errstate(all="ignore"):
        rays = _Rays(p, v)
        n = rays.n
        status = np.where(rays.miss, MISS, 255).astype(np.int64)
        Z = rays.z_lo.copy()
        Zp, fp, Zh = np.zeros(N, F), np.zeros(N, F), np.zeros(N, F)
        pv = np.zeros(N, bool)
        count = np.zeros(N, np.int64)
        live = np.nonzero(status == 255)[0]
        while live.size:
            gone = ~(Z[live] <= rays.z_hi[live])
            status[live[gone]] = NO_SURFACE
            live = live[~gone]
            spent = count[live] >= max_steps
            status[live[spent]] = EXHAUSTED
            cur = live[~spent]
            count[cur] += 1
            Zc = Z[cur]
            inside, cell, frac = rays.cell(cur, Zc)
            valid = np.zeros(len(cur), bool)
            f = np.zeros(len(cur), F)
            nxt = Zc + step
            ins = np.nonzero(inside)[0]
            near = words[_nearest(n, cell[ins], frac[ins])]
            free = (T.word_w(near) >= mw) & (T.word_t(near) == Q)
            fr = ins[free]
            valid[fr] = True
            f[fr] = F(Q)
            nxt[fr] = Zc[fr] + skip
            rest = ins[~free]
            cw = _corners(n, words, cell[rest])
            seen = (T.word_w(cw) >= mw).all(-1)
            it = rest[seen]
            valid[it] = True
            f[it] = _trilinear(T.word_t(cw[seen]).astype(F), frac[it])
            ends = valid & (f <= 0)
            hit = ends & pv[cur] & (fp[cur] > 0)
            h = cur[hit]
            status[h] = HIT
            Zh[h] = Zp[h] + ((Zc[hit] - Zp[h]) * (fp[h] / (fp[h] - f[hit])))
            status[cur[ends & ~hit]] = BEHIND
            on = valid & ~ends
            pv[cur[~valid]] = False
            pv[cur[on]] = True
            fp[cur[on]] = f[on]
            Zp[cur[on]] = Zc[on]
            Z[cur[~ends]] = nxt[~ends]
            live = cur[~ends]
        # the outputs of the hits
        depth = np.where(status == HIT, Zh, F(0.0)).astype(F)
        normals = np.zeros((N, 4), F)
        bgr = None if color is None else np.zeros((N, 3), np.uint8)
        h = np.nonzero(status == HIT)[0]
        inside, cell, frac = rays.cell(h, Zh[h])
        h, cell, frac = h[inside], cell[inside], frac[inside]
        if color is not None:
            c = np.ascontiguousarray(color, np.uint32).ravel()[_nearest(n, cell, frac)]
            has = (c >> np.uint32(24)) > 0
            for ch, shift in ((0, 16), (1, 8), (2, 0)):
                bgr[h, ch] = np.where(has, (c >> np.uint32(shift)) & np.uint32(0xFF), 0)
        cw = _corners(n, words, cell)
        seen = (T.word_w(cw) >= mw).all(-1)
        h, cw, frac = h[seen], cw[seen], frac[seen]
        t = T.word_t(cw).astype(F)
        a, b, c = frac[:, 0], frac[:, 1], frac[:, 2]
        gx = _lerp(_lerp(t[:, 1] - t[:, 0], t[:, 3] - t[:, 2], b), _lerp(t[:, 5] - t[:, 4], t[:, 7] - t[:, 6], b), c)
        gy = _lerp(_lerp(t[:, 2] - t[:, 0], t[:, 3] - t[:, 1], a), _lerp(t[:, 6] - t[:, 4], t[:, 7] - t[:, 5], a), c)
        gz = _lerp(_lerp(t[:, 4] - t[:, 0], t[:, 5] - t[:, 1], a), _lerp(t[:, 6] - t[:, 2], t[:, 7] - t[:, 3], a), b)
        L = np.sqrt(((gx * gx) + (gy * gy)) + (gz * gz))
        ok = np.isfinite(L) & (L > 0)
        Ls = np.where(ok, L, F(1.0))
        nw = [gx / Ls, gy / Ls, gz / Ls]
        R = [F(x) for x in v["R"]]
        for r in range(3):
            normals[h, r] = np.where(ok, ((R[3 * r] * nw[0]) + (R[3 * r + 1] * nw[1])) + (R[3 * r + 2] * nw[2]), F(0.0))
        normals[h, 3] = np.where(ok, T.word_w(cw).min(-1).astype(F), F(0.0))
    total = int(count.sum())
    rep = dict(rays=N, samples_lo=total & 0xFFFFFFFF, samples_hi=total >> 32)
    for s, name in enumerate(STATUS_NAMES):
        rep[name] = int((status == s).sum())
    return dict(depth=depth.reshape(H, W), normals=normals.reshape(H, W, 4), bgr=None if bgr is None else bgr.reshape(H, W, 3),
                status=status.astype(np.uint8).reshape(H, W), samples=count.reshape(H, W), report=rep)


def report_words(rep):
    return [rep[k] for k in REPORT_FIELDS]
