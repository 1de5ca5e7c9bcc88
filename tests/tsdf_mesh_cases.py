"""Cases of the TSDF volume's triangle mesh (tests/tsdf_mesh_ref.py), shared by tests/test_tsdf_mesh_api.py (CPU: the table, the
reference's properties, the shared header against it) and tests/test_gpu_tsdf_mesh.py (the kernels against it).  Every case is a
volume of voxel words (and colour words) that adc_tsdf_upload brings in.  The shapes are the smallest at which the kernels can go wrong:
8 x 8 x 8; 12 x 5 x 7 (tiles of 256 voxels and chunks of 64 lanes straddle rows and planes); 68 x 5 x 4 (lane 63's +x neighbour in
mid-row, a chunk that ends at a row end); 260 x 4 x 4 (tile boundaries inside a row); 64 x 64 x 4 (all 256 cases as isolated
2 x 2 x 2 blocks between weight-0 voxels); 16 x 12 x 10 with random signs and weights (unseen corners); a sphere in 32^3.

case(name) -> dict(params, volume (tsdf, color)); reference(name, min_weight) -> (vertices, triangles, report), computed once, read-only."""
import functools

import numpy as np

from tests import tsdf_mesh_ref as MR
from tests import tsdf_ref as T

UPLOAD_CASES = ("base8", "straddle", "lane63", "long_row", "all_cases", "random_unseen", "sphere32")
EMUL_CASES = UPLOAD_CASES + ("closed_3", "sphere24")
SHAPES = dict(base8=(8, 8, 8), straddle=(12, 5, 7), lane63=(68, 5, 4), long_row=(260, 4, 4), random_unseen=(16, 12, 10))
MIN_WEIGHTS = (1, 3)


def _params(nx, ny, nz, colour=True):
    return T.params(nx, ny, nz, 0.05, (-0.3, 0.1, 0.5), 0.15, flags=T.COLOR if colour else 0)


def random_volume(nx, ny, nz, seed, weights=(0, 1, 2, 3, 4, 5, 300)):
    """random signs with a few t = 0, +-32767 and stored -32768; weights drawn from `weights` (0 and below min_weight: unseen)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(-T.Q, T.Q + 1, (nz, ny, nx))
    special = rng.random((nz, ny, nx))
    t = np.where(special < 0.03, 0, np.where(special < 0.06, -32768, np.where(special < 0.09, T.Q, t)))
    w = rng.choice(np.array(weights), (nz, ny, nx), p=_weight_probabilities(len(weights)))
    return T.make_words(t, w), rng.integers(0, 2 ** 32, (nz, ny, nx), dtype=np.uint32)


def _weight_probabilities(n):
    # the first two entries (0 and 1: unseen at min_weight 3, 0 always) are rare enough that seen cells remain
    p = np.full(n, 1.0)
    p[0] = p[1] = 0.25
    return p / p.sum()


def closed_volume(seed, shape=(14, 11, 9)):
    """fully seen, random signs inside, an all-positive outermost layer: a closed surface with ambiguous faces"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    t = rng.integers(1, T.Q + 1, (nz, ny, nx)) * rng.choice([-1, 1], (nz, ny, nx))
    t[0], t[-1], t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1] = 7, 7, 7, 7, 7, 7
    return T.make_words(t, np.full((nz, ny, nx), 2)), None


def sphere_volume(n, radius):
    """t < 0 inside a sphere of `radius` voxels about the centre of an n^3 volume, every voxel seen"""
    c = (n - 1) / 2.0 + 0.13  # (off the lattice: no t = 0)
    k, j, i = np.mgrid[0:n, 0:n, 0:n].astype(np.float64)
    d = np.sqrt((i - c) ** 2 + (j - c) ** 2 + (k - c) ** 2) - radius
    t = np.rint(np.clip(d / 3.0, -1, 1) * T.Q).astype(np.int64)
    assert (t != 0).all()
    return T.make_words(t, np.full((n, n, n), 4)), None


def all_cases_volume():
    """64 x 64 x 4: case c as the 2 x 2 x 2 block at (3 * (c % 21), 3 * (c // 21), 0), every voxel between the blocks of weight 0"""
    t = np.full((4, 64, 64), 9, np.int64)
    w = np.zeros((4, 64, 64), np.int64)
    for c in range(256):
        i0, j0 = 3 * (c % 21), 3 * (c // 21)
        for corner in range(8):
            di, dj, dk = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
            t[dk, j0 + dj, i0 + di] = -(100 + corner) if c >> corner & 1 else 200 + corner
            w[dk, j0 + dj, i0 + di] = 3
    return T.make_words(t, w), np.random.default_rng(9).integers(0, 2 ** 32, (4, 64, 64), dtype=np.uint32)


def _build(name):
    if name in SHAPES:
        nx, ny, nz = SHAPES[name]
        return dict(params=_params(nx, ny, nz), volume=random_volume(nx, ny, nz, 100 + sorted(SHAPES).index(name)))
    if name == "all_cases":
        return dict(params=_params(64, 64, 4), volume=all_cases_volume())
    if name == "sphere32":
        return dict(params=_params(32, 32, 32, False), volume=sphere_volume(32, 9.4))
    if name == "sphere24":
        return dict(params=_params(24, 24, 24, False), volume=sphere_volume(24, 7.2))
    if name.startswith("closed_"):
        return dict(params=_params(16, 11, 9, False), volume=closed_volume(int(name[7:]), (16, 11, 9)))
    raise KeyError(name)


def _freeze(a):
    if a is not None:
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    c = _build(name)
    c["volume"] = tuple(_freeze(a) for a in c["volume"])
    return c


@functools.lru_cache(maxsize=None)
def reference(name, min_weight=1):
    c = case(name)
    v, t, rep = MR.mesh(c["volume"], c["params"], min_weight)
    return _freeze(v), _freeze(t), rep


def capacities(count):
    return sorted({0, 1, max(count - 1, 0), count, count + 7})
