"""The definition of the TSDF volume's triangle mesh (include/adcensus_c_api.h: adc_tsdf_mesh_device) in numpy: what
adcensus_amd/csrc/tsdf_cell.h (tests/emul/emul_tsdf_mesh.cpp) and the kernels (adcensus_amd/csrc/k_tsdf.hip) are held to bit for bit.

The vertices are the points of tests/tsdf_ref.py: extract, the case table is the one tools/gen_tsdf_mc_table.py derives; a triangle is
three integers chosen by integer comparisons, so nothing here rounds."""
import os
import sys

import numpy as np

from tests import tsdf_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_tsdf_mc_table as GEN  # noqa: E402

REPORT_FIELDS = ("voxels_seen", "vertices", "triangles", "cells_seen", "cells_surface")
M, TABLE = GEN.table()


def vertex_numbers(tsdf, min_weight):
    """-> int64 [3][nz][ny][nx]: the position of the crossing (voxel, axis) in the full point list of tsdf_ref.extract, -1 where the
    pair is no crossing"""
    nz, ny, nx = tsdf.shape
    t, w = T.word_t(tsdf), T.word_w(tsdf)
    seen, neg = w >= min_weight, t < 0
    cross = np.zeros((nz, ny, nx, 3), bool)  # (voxel order first, then x, y, z: the order of the list)
    cross[:, :, :-1, 0] = seen[:, :, :-1] & seen[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
    cross[:, :-1, :, 1] = seen[:, :-1, :] & seen[:, 1:, :] & (neg[:, :-1, :] != neg[:, 1:, :])
    cross[:-1, :, :, 2] = seen[:-1, :, :] & seen[1:, :, :] & (neg[:-1, :, :] != neg[1:, :, :])
    rank = np.cumsum(cross.ravel()).reshape(cross.shape) - 1
    return np.moveaxis(np.where(cross, rank, -1), 3, 0), int(cross.sum())


def cells(tsdf, min_weight):
    """-> (seen bool, case int64) [nz-1][ny-1][nx-1]"""
    nz, ny, nx = tsdf.shape
    t, w = T.word_t(tsdf), T.word_w(tsdf)
    seen = np.ones((nz - 1, ny - 1, nx - 1), bool)
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        di, dj, dk = GEN.corner(c)
        sl = (slice(dk, nz - 1 + dk), slice(dj, ny - 1 + dj), slice(di, nx - 1 + di))
        seen &= w[sl] >= min_weight
        case |= (t[sl] < 0).astype(np.int64) << c
    return seen, case


def mesh(volume, p, min_weight=1, vertex_capacity=None, triangle_capacity=None):
    """-> (vertices POINT_DTYPE [.], triangles uint32 [.][3], report dict).  A capacity of None gives the whole list, else its first
    min(count, capacity) records; the triangles keep their true vertex numbers and the report its counts whatever the capacities."""
    tsdf = volume[0]
    nz, ny, nx = tsdf.shape
    pts, xrep = T.extract(volume, p, min_weight)
    vid, n_cross = vertex_numbers(tsdf, min_weight)
    assert n_cross == len(pts)
    seen, case = cells(tsdf, min_weight)
    counts = np.array([len(r) for r in TABLE], np.int64)
    emit = seen & (counts[case] > 0)
    kk, jj, ii = np.nonzero(emit)
    cc = case[emit]
    nn = (kk * ny + jj) * nx + ii
    keys, recs = [], []
    for c in np.unique(cc):
        sel = cc == c
        k, j, i, n = kk[sel], jj[sel], ii[sel], nn[sel]
        for slot, tri in enumerate(TABLE[c]):
            rec = np.zeros((len(n), 3), np.int64)
            for v, e in enumerate(tri):
                (di, dj, dk), axis = GEN.edge_owner(e)
                rec[:, v] = vid[axis, k + dk, j + dj, i + di]
            assert (rec >= 0).all()  # every sign-changing edge of a seen cell is a crossing of the vertex list
            keys.append(n * 8 + slot)
            recs.append(rec)
    if recs:
        tris = np.concatenate(recs)[np.argsort(np.concatenate(keys), kind="stable")].astype(np.uint32)
    else:
        tris = np.zeros((0, 3), np.uint32)
    rep = dict(voxels_seen=xrep["voxels_seen"], vertices=len(pts), triangles=len(tris), cells_seen=int(seen.sum()), cells_surface=int(emit.sum()))
    return (pts if vertex_capacity is None else pts[:vertex_capacity]), (tris if triangle_capacity is None else tris[:triangle_capacity]), rep


def report_words(rep):
    return [rep[k] for k in REPORT_FIELDS]


def count_limit_refused(nx, ny, nz):
    """the call is refused when M * cells does not fit 32 bits"""
    return M * (nx - 1) * (ny - 1) * (nz - 1) > 2 ** 32 - 1
