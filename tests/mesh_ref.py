"""The definition of the triangle mesh from a disparity map (include/adcensus_c_api.h: adc_mesh_device) in numpy: what
adcensus_amd/csrc/mesh_cell.h (tests/emul/emul_mesh.cpp) and the kernels (adcensus_amd/csrc/k_mesh.hip) are held to bit for bit.

Every operand is np.float32, so every operation rounds once to binary32.  Validity, position and colour of a lattice pixel are taken
from tests/outputs_ref.py (the cloud's)."""
import numpy as np

from tests import outputs_ref as O

F = np.float32
MAX_STEP = 16
DEFAULTS = dict(max_diff=1.0, step=1)
REPORT_FIELDS = ("lattice_valid", "vertices", "triangles", "cells_two", "cells_one")


def lattice(n, step):
    return (n - 1) // step + 1


def lattice_values(disp, calib, step):
    """-> (a float32 [Hl][Wl], valid bool [Hl][Wl]) of the lattice pixels"""
    a = np.abs(np.asarray(disp, F))[::step, ::step]
    if calib is None:
        return a, a != O.INF
    return a, O.depth(a, calib)[1]


def near(p, q, max_diff):
    with np.errstate(invalid="ignore"):
        return np.abs(p - q) <= F(max_diff)  # (inf - inf = NaN: fails; such pixels are not valid anyway)


def cells(a, valid, max_diff):
    """Per cell [Hl-1][Wl-1]: (t0, t1 bool: the candidate is emitted; bc bool: the diagonal is BC)."""
    A, B, C, D = a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]
    vA, vB, vC, vD = valid[:-1, :-1], valid[:-1, 1:], valid[1:, :-1], valid[1:, 1:]

    def joined(p, vp, q, vq):
        return vp & vq & near(p, q, max_diff)

    jab, jac, jbd, jcd = joined(A, vA, B, vB), joined(A, vA, C, vC), joined(B, vB, D, vD), joined(C, vC, D, vD)
    jad, jbc = joined(A, vA, D, vD), joined(B, vB, C, vC)
    nvalid = vA.astype(int) + vB + vC + vD
    with np.errstate(invalid="ignore"):
        ad4 = np.abs(A - D) <= np.abs(B - C)  # (ties: AD; NaN: False = BC)
    four, three = nvalid == 4, nvalid == 3
    # candidates: (emitted, diagonal is BC) per slot
    t0 = np.zeros(A.shape, bool)
    t1 = np.zeros(A.shape, bool)
    bc = np.zeros(A.shape, bool)
    m = four & ad4      # T0 = (A, C, D), T1 = (A, D, B)
    t0 |= m & jac & jcd & jad
    t1 |= m & jad & jbd & jab
    m = four & ~ad4     # T0 = (A, C, B), T1 = (B, C, D)
    bc |= m
    t0 |= m & jac & jbc & jab
    t1 |= m & jbc & jcd & jbd
    m = three & ~vD     # (A, C, B): T0 of BC
    bc |= m
    t0 |= m & jac & jbc & jab
    m = three & ~vA     # (B, C, D): T1 of BC
    bc |= m
    t1 |= m & jbc & jcd & jbd
    m = three & ~vB     # (A, C, D): T0 of AD
    t0 |= m & jac & jcd & jad
    m = three & ~vC     # (A, D, B): T1 of AD
    t1 |= m & jad & jbd & jab
    return t0, t1, bc


def mesh(disp, calib=None, max_diff=1.0, step=1, bgr_left=None):
    """-> (vertices O.POINT_DTYPE [nv], vertex_index int32 [nv], triangles uint32 [nt][3], report dict).  calib: (focal_px, baseline,
    cx, cy, doffs) or None."""
    d = np.asarray(disp, F)
    H, W = d.shape
    assert 1 <= step <= MAX_STEP and max_diff >= 0
    a, valid = lattice_values(d, calib, step)
    Hl, Wl = a.shape
    assert (Hl, Wl) == (lattice(H, step), lattice(W, step))
    t0, t1, bc = cells(a, valid, max_diff) if Hl > 1 and Wl > 1 else (np.zeros((max(Hl - 1, 0), max(Wl - 1, 0)), bool),) * 3
    # lattice indices of the corners
    idx = np.arange(Hl * Wl, dtype=np.int64).reshape(Hl, Wl)
    cA, cB, cC, cD = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    first = np.where(bc[..., None], np.stack([cA, cC, cB], -1), np.stack([cA, cC, cD], -1))   # T0
    second = np.where(bc[..., None], np.stack([cB, cC, cD], -1), np.stack([cA, cD, cB], -1))  # T1
    both = np.stack([first, second], axis=-2)             # [Hl-1][Wl-1][2][3]
    emitted = np.stack([t0, t1], axis=-1)                 # [Hl-1][Wl-1][2]: raster order of the cells, T0 before T1
    tri_lattice = both[emitted]                           # [nt][3] lattice indices
    used = np.zeros(Hl * Wl, bool)
    used[tri_lattice.ravel()] = True
    number = np.cumsum(used) - 1                          # vertex number of a used lattice pixel
    triangles = number[tri_lattice].astype(np.uint32).reshape(-1, 3)
    # vertex records: the cloud's points of the used lattice pixels
    lj, li = np.divmod(np.flatnonzero(used), Wl)
    ys, xs = lj * step, li * step
    vertex_index = (ys * W + xs).astype(np.int32)
    vertices = np.zeros(len(vertex_index), O.POINT_DTYPE)
    av = a[lj, li]
    if calib is None:
        vertices["x"], vertices["y"], vertices["z"] = xs.astype(F), ys.astype(F), av
    else:
        f, _, cx, cy, _, _ = O.calib_f32(calib)
        z = O.depth(av, calib)[0]
        with np.errstate(invalid="ignore", over="ignore"):
            vertices["x"] = ((xs.astype(F) - cx) * z) / f
            vertices["y"] = ((ys.astype(F) - cy) * z) / f
        vertices["z"] = z
    if bgr_left is not None:
        img = np.asarray(bgr_left, np.uint8).reshape(H, W, 3)
        vertices["r"], vertices["g"], vertices["b"] = img[ys, xs, 2], img[ys, xs, 1], img[ys, xs, 0]
    rep = dict(lattice_valid=int(valid.sum()), vertices=len(vertices), triangles=len(triangles), cells_two=int((t0 & t1).sum()), cells_one=int((t0 ^ t1).sum()))
    assert rep["triangles"] == 2 * rep["cells_two"] + rep["cells_one"]
    return vertices, vertex_index, np.ascontiguousarray(triangles), rep


def report_words(rep):
    return [rep[k] for k in REPORT_FIELDS]


def cell_flags(disp, calib=None, max_diff=1.0, step=1):
    """(t0, t1, bc) per cell, for the tests that ask what a case exercises"""
    a, valid = lattice_values(np.asarray(disp, F), calib, step)
    return cells(a, valid, max_diff)
