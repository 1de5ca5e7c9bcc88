"""The cases of the moving TSDF volume, shared by the CPU tier (tests/test_tsdf_shift_api.py: the shared header, serially) and the GPU
tier (tests/test_gpu_tsdf_shift.py: the kernels).  The volumes are the smallest that reach the seams of the kernels:

  8 x 6 x 5    N = 240, less than one 256-voxel tile
  12 x 7 x 9   tile seams in mid-row, rows shorter than a wave
  68 x 5 x 4   a row longer than 64 lanes: lane 63's extra +x word, and the ragged last 256-voxel row piece of the shift kernel

Voxel words are uniformly random -- t any int16 including -32768, w in 0..3, random colour words --, so every slab holds crossings of
every kind (the long-row volume has one planted row, see words()).  The geometry is dyadic (voxel = 2^-5, origin a multiple of it): every origin and every voxel centre is exact in binary32.

What a shift can hand out.  A crossing (a, b = a + 1 on an axis) is of kind 1 (only a leaves), 2 (only b leaves) or 3 (both).  On the
axis of the pair, a positive shift makes the LOW voxels leave, so the pair across the slab's face is of kind 1, and a negative shift
gives kind 2; a pair of any other axis inside the slab is of kind 3.  A shift can therefore yield kind 1 only with a positive
component below its axis' size, kind 2 only with such a negative component, and all three only with both.  kinds_possible() says
which; the module asserts at import that the numpy leaving list of every case holds at least one crossing of every possible kind
for min_weight 1 and 3 -- and that the shifts with 0 < |s_a| < n_a on EVERY axis (mixed signs) hold all three.  A case that fails
this is to be replaced, not skipped.
"""
import functools

import numpy as np

from tests import tsdf_ref as T
from tests import tsdf_shift_ref as SR

VOXEL = 2.0 ** -5
VOLUMES = {"v8x6x5": (8, 6, 5), "v12x7x9": (12, 7, 9), "v68x5x4": (68, 5, 4)}
ORIGINS = {"v8x6x5": (-4 * VOXEL, 3 * VOXEL, 17 * VOXEL), "v12x7x9": (-37 * VOXEL, -2 * VOXEL, 64 * VOXEL), "v68x5x4": (100 * VOXEL, -11 * VOXEL, 5 * VOXEL)}
SEEDS = {"v8x6x5": 238, "v12x7x9": 26, "v68x5x4": 1}       # (chosen so that the assertion below holds: see _check_cases)
PLANT_ROW = {"v68x5x4": (2, 1)}                              # (j, k) of a row whose weights are 3 and whose signs alternate
MIN_WEIGHTS = (1, 3)


def params(vol, colour):
    nx, ny, nz = VOLUMES[vol]
    return T.params(nx, ny, nz, VOXEL, ORIGINS[vol], 4 * VOXEL, flags=T.COLOR if colour else 0)


@functools.lru_cache(maxsize=None)
def words(vol):
    """(tsdf, color) uint32 [nz][ny][nx], uniformly random; the colour plane is dropped for a volume without colour"""
    nx, ny, nz = VOLUMES[vol]
    rng = np.random.default_rng(SEEDS[vol])
    t = rng.integers(-32768, 32768, (nz, ny, nx), dtype=np.int64)
    t.ravel()[rng.integers(0, t.size, 3)] = -32768
    w = rng.integers(0, 4, (nz, ny, nx), dtype=np.int64)
    if vol in PLANT_ROW:
        # an x face of this volume has 20 pairs: too few for a crossing with min_weight 3 to be there by chance on every face the
        # shifts cut.  One row is planted: random magnitudes, alternating signs, w = 3 -- a crossing on each of its x pairs.
        j, k = PLANT_ROW[vol]
        mag = rng.integers(1, 32768, nx, dtype=np.int64)
        t[k, j, :] = np.where(np.arange(nx) % 2 == 0, mag, -mag)
        w[k, j, :] = 3
    tsdf = (t & 0xFFFF).astype(np.uint32) | (w.astype(np.uint32) << np.uint32(16))
    color = rng.integers(0, 1 << 32, (nz, ny, nx), dtype=np.uint64).astype(np.uint32)
    tsdf.setflags(write=False)
    color.setflags(write=False)
    return tsdf, color


def volume(vol, colour):
    t, c = words(vol)
    return t, (c if colour else None)


def shifts(vol):
    nx, ny, nz = VOLUMES[vol]
    out = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    out += [(s, 0, 0) for s in (3, -3, 4, -4, 5, -5)]          # both variants of the shift kernel
    out += [(4, 1, -1), (-4, -2, 1)]                           # the 16-byte variant with a row offset
    out += [(3, -2, 1), (-2, 3, -1)]                           # 0 < |s_a| < n_a on every axis
    out += [(nx - 1, 0, 0), (nx, 0, 0), (0, ny - 1, 0), (0, -ny, 0), (0, 0, 1 - nz), (0, 0, nz)]
    out += [(0, -(ny + 3), 0), (nx + 7, 1, 0), (2, 1, 1 << 24), (-(1 << 24), 0, 0)]  # larger than the axis
    out += [(0, 0, 0)]
    return out


def kinds_possible(vol, s):
    n = VOLUMES[vol]
    if any(abs(s[a]) >= n[a] for a in range(3)):
        return {3}                                             # everything leaves
    out = set()
    if any(0 < s[a] for a in range(3)):
        out |= {1, 3}
    if any(s[a] < 0 for a in range(3)):
        out |= {2, 3}
    return out


def all_in_range(vol, s):
    n = VOLUMES[vol]
    return all(0 < abs(s[a]) < n[a] for a in range(3))


@functools.lru_cache(maxsize=None)
def reference(vol, colour, s, min_weight):
    """tests/tsdf_shift_ref.shift of the case from a zero offset -> (new volume, new params, offset, ALL points, report)"""
    new, q, off, pts, rep = SR.shift(volume(vol, colour), params(vol, colour), SR.shift_params(s, min_weight))
    for a in new:
        if a is not None:
            a.setflags(write=False)
    pts.setflags(write=False)
    return new, q, off, pts, rep


def capacities(points):
    """0, one short of the list, ample"""
    return sorted({0, max(points - 1, 0), points + 5})


def _check_cases():
    for vol in VOLUMES:
        seen_all = 0
        for s in shifts(vol):
            if s == (0, 0, 0):
                continue
            for mw in MIN_WEIGHTS:
                _, kinds = SR.leaving_list(volume(vol, True), params(vol, True), s, mw)
                got = set(int(k) for k in np.unique(kinds))
                want = kinds_possible(vol, s)
                assert got == want, ("replace this case: kinds", vol, s, mw, got, want)
                if all_in_range(vol, s):
                    assert got == {1, 2, 3}, ("replace this case: not all three kinds", vol, s, mw, got)
                    seen_all += 1
        assert seen_all >= 2 * len(MIN_WEIGHTS), vol


_check_cases()
