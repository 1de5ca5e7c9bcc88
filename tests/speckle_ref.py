"""The speckle filter's definition (include/adcensus_c_api.h: adc_set_speckle_filter) in numpy and plain Python, independent of the
kernels; the GPU tests compare k_speckle.hip with it bit for bit.

  valid      d finite (+inf, -inf and NaN are invalid and never touched)
  joined     4-neighbours p, q, both valid, abs(d[p] - d[q]) <= max_diff in binary32 (one subtraction, one rounding)
  component  class of the transitive closure of joined
  label      raster index of the component's first pixel in raster order; -1 at invalid pixels
  filter     components of size <= max_size (max_size > 0) become +inf; everything else keeps its bits
  stats      (components, removed components, removed pixels)

Formulation: maximal row runs (numpy), then a union-find with min-index roots over the runs that touch vertically (plain Python over
the distinct run pairs).  A 1080p map takes a few seconds."""
import numpy as np


def speckle_ref(disp, max_size, max_diff):
    """-> (filtered float32 [H][W], labels int32 [H][W], (components, removed components, removed pixels))"""
    d = np.ascontiguousarray(disp, dtype=np.float32)
    assert d.ndim == 2
    h, w = d.shape
    md = np.float32(max_diff)
    assert np.isfinite(md) and md >= 0
    valid = np.isfinite(d)
    with np.errstate(invalid="ignore", over="ignore"):
        hj = np.zeros((h, w), bool)  # joined to the left neighbour
        hj[:, 1:] = valid[:, 1:] & valid[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= md)
        vj = np.zeros((h, w), bool)  # joined to the upper neighbour
        vj[1:, :] = valid[1:, :] & valid[:-1, :] & (np.abs(d[1:, :] - d[:-1, :]) <= md)
    start = (valid & ~hj).reshape(-1)
    run = np.cumsum(start, dtype=np.int64) - 1  # run of every valid pixel, runs numbered in raster order
    run[~valid.reshape(-1)] = -1
    nruns = int(start.sum())
    first = np.flatnonzero(start)  # first pixel of every run
    run2 = run.reshape(h, w)
    lo, up = run2[1:, :][vj[1:, :]], run2[:-1, :][vj[1:, :]]
    pairs = np.unique(np.stack([lo, up], 1), axis=0) if lo.size else np.zeros((0, 2), np.int64)
    parent = list(range(nruns))
    for a, b in pairs.tolist():
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b
    for r in range(nruns):  # (parent[r] < r is final by the time r is reached)
        parent[r] = parent[parent[r]]
    root = np.asarray(parent, np.int64).reshape(-1)
    labels = np.full(h * w, -1, np.int32)
    v = valid.reshape(-1)
    comp = root[run[v]] if nruns else np.zeros(0, np.int64)  # root run of every valid pixel
    labels[v] = first[comp].astype(np.int32) if nruns else 0
    sizes = np.bincount(comp, minlength=nruns) if nruns else np.zeros(0, np.int64)
    is_root = root == np.arange(nruns)
    out = d.copy().reshape(-1)
    removed_c = removed_p = 0
    if max_size > 0 and nruns:
        small = is_root & (sizes <= max_size)
        kill = small[comp]
        idx = np.flatnonzero(v)[kill]
        out[idx] = np.float32(np.inf)
        removed_c, removed_p = int(small.sum()), int(kill.sum())
    return out.reshape(h, w), labels.reshape(h, w), (int(is_root.sum()), removed_c, removed_p)


def largest(labels):
    """pixels of the largest component"""
    l = labels[labels >= 0]
    return int(np.bincount(l).max()) if l.size else 0
