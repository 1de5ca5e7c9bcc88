"""The voxel-grid filter of the cloud (include/adcensus_c_api.h: adc_set_cloud_voxel_grid) in numpy -- the definition the kernels
(adcensus_amd/csrc/k_voxel.hip) and the serial program built from the shared header (tests/emul/emul_voxel.cpp) are held to bit for bit.
Every float operand is np.float32 (an array or a scalar), so every operation rounds once to binary32.

A grid is a dict: leaf, z_min, z_max, pose (None or (R 3x3, t 3)); a calibration is (focal_px, baseline, cx, cy, doffs)."""
import numpy as np

from tests import outputs_ref as O

F = np.float32
POINT_DTYPE = O.POINT_DTYPE
BIAS = 1 << 20


def grid(leaf, z_min=0.0, z_max=np.inf, pose=None):
    return {"leaf": F(leaf), "z_min": F(z_min), "z_max": F(z_max), "pose": pose}


def axis(w, inv):
    """One axis of float32 world coordinates: (in_range bool, cell int64 = i + 2^20, q int64)."""
    with np.errstate(invalid="ignore", over="ignore"):
        u = (np.asarray(w, F) * F(inv)).astype(F)
        ok = np.abs(u) < F(1048576.0)  # (NaN fails)
        us = np.where(ok, u, F(0))
        i = np.floor(us).astype(F)
        f = (us - i).astype(F)  # (one rounding: exactly 1.0 for a tiny negative u)
        q = np.minimum((f * F(65536.0)).astype(F).astype(np.int64), 65535)
    return ok, i.astype(np.int64) + BIAS, q


def points(disp, calib, g):
    """Per pixel in raster order: (valid bool [P], kept bool [P], key uint64 [P], q int64 [P][3]); key and q mean nothing where not kept."""
    f, _, cx, cy, _, _ = O.calib_f32(calib)
    z, valid = O.depth(disp, calib)
    h, w = z.shape
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(invalid="ignore", over="ignore"):
        x = (((xs.astype(F) - cx) * z) / f).astype(F)
        y = (((ys.astype(F) - cy) * z) / f).astype(F)
        kept = valid & (g["z_min"] <= z) & (z <= g["z_max"])
        if g["pose"] is not None:
            R = np.asarray(g["pose"][0], F).reshape(9)
            t = np.asarray(g["pose"][1], F).reshape(3)
            world = [(((R[3 * r] * x + R[3 * r + 1] * y).astype(F) + R[3 * r + 2] * z).astype(F) + t[r]).astype(F) for r in range(3)]
        else:
            world = [x, y, z]
    inv = F(F(1.0) / g["leaf"])
    key = np.zeros(z.shape, np.uint64)
    qs = []
    for a, wa in enumerate(world):
        ok, cell, q = axis(np.where(kept, wa, F(np.nan)), inv)
        kept = kept & ok
        key |= np.where(ok, cell, 0).astype(np.uint64) << np.uint64(42 - 21 * a)
        qs.append(q)
    return valid.ravel(), kept.ravel(), key.ravel(), np.stack(qs, -1).reshape(-1, 3)


def record_xyz(cell, mq, leaf):
    """((float)i + (float)mq * 2^-16) * leaf for int64 arrays cell (biased) and mq: two roundings."""
    with np.errstate(over="ignore"):
        return (((cell - BIAS).astype(F) + (mq.astype(F) * F(2.0 ** -16)).astype(F)).astype(F) * F(leaf)).astype(F)


def voxel_cloud(disp, left_bgr, calib, g):
    """(POINT_DTYPE array of all voxels in ascending order of leader, report dict)."""
    valid, kept, key, q = points(disp, calib, g)
    img = np.asarray(left_bgr, np.uint8).reshape(-1, 3)
    idx = np.nonzero(kept)[0]
    report = {"points_valid": int(valid.sum()), "points_kept": int(idx.size), "voxels": 0}
    if idx.size == 0:
        return np.zeros(0, POINT_DTYPE), report
    keys, first, inverse = np.unique(key[idx], return_index=True, return_inverse=True)  # (first: the first occurrence = lowest raster index)
    nv = keys.size
    n = np.bincount(inverse, minlength=nv).astype(np.int64)
    sums = np.zeros((nv, 6), np.int64)
    vals = np.concatenate([q[idx], img[idx][:, ::-1].astype(np.int64)], 1)  # q x y z, r g b
    for c in range(6):
        np.add.at(sums[:, c], inverse, vals[:, c])
    mean = (sums + (n // 2)[:, None]) // n[:, None]
    order = np.argsort(idx[first], kind="stable")
    pts = np.zeros(nv, POINT_DTYPE)
    k = keys.astype(np.int64)
    cells = [(k >> 42) & 0x1FFFFF, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF]
    for a, name in enumerate("xyz"):
        pts[name] = record_xyz(cells[a], mean[:, a], g["leaf"])
    pts["r"], pts["g"], pts["b"] = mean[:, 3], mean[:, 4], mean[:, 5]
    pts["pad"] = np.minimum(n, 255)
    report["voxels"] = int(nv)
    return pts[order], report


def voxel_cloud_loop(disp, left_bgr, calib, g):
    """The same, word for word from the definition: one pixel at a time into a dict keyed by the integer triple."""
    valid, kept, key, q = points(disp, calib, g)
    img = np.asarray(left_bgr, np.uint8).reshape(-1, 3)
    vox = {}
    for i in range(kept.size):
        if not kept[i]:
            continue
        k = int(key[i])
        triple = ((k >> 42) - BIAS, ((k >> 21) & 0x1FFFFF) - BIAS, (k & 0x1FFFFF) - BIAS)
        v = vox.setdefault(triple, {"n": 0, "sq": [0, 0, 0], "sc": [0, 0, 0], "leader": i})
        v["n"] += 1
        for a in range(3):
            v["sq"][a] += int(q[i, a])
            v["sc"][a] += int(img[i, 2 - a])
        v["leader"] = min(v["leader"], i)
    out = np.zeros(len(vox), POINT_DTYPE)
    for j, (triple, v) in enumerate(sorted(vox.items(), key=lambda kv: kv[1]["leader"])):
        n = v["n"]
        for a, name in enumerate("xyz"):
            mq = (v["sq"][a] + n // 2) // n
            out[name][j] = F(F(F(triple[a]) + F(F(mq) * F(2.0 ** -16))) * g["leaf"])
        out["r"][j], out["g"][j], out["b"][j] = [(s + n // 2) // n for s in v["sc"]]
        out["pad"][j] = min(n, 255)
    return out, {"points_valid": int(valid.sum()), "points_kept": int(kept.sum()), "voxels": len(vox)}
