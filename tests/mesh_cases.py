"""Maps, calibrations, parameters and the case list shared by the CPU and GPU tiers of the mesh tests (tests/test_mesh_api.py,
tests/test_gpu_mesh.py).  The reference result of a case is computed once (functools.lru_cache) and never modified.  What a case is
named for is asserted on the reference's own counts at import: otherwise the tests show nothing."""
import functools

import numpy as np

from tests import mesh_ref as M
from tests.normals_cases import calib_for, slanted

F = np.float32
INF, NAN = np.inf, np.nan


def quad(a, b, c, d):
    """A 2 x 2 map: corners A B / C D"""
    return np.array([[a, b], [c, d]], F)


def mixed_map():
    """67 x 35: a slanted plane, a step of 40 px at x = 40, holes of +inf, -inf and NaN (single pixels and blocks), a region of
    negative disparities, a patch of 22 px (behind doffs = -25: s <= 0 with the calibration, valid without)."""
    W, H = 67, 35
    d = slanted(W, H, d0=30.0, gx=0.12, gy=0.05, noise=0.3, seed=7)
    d[:, 40:] += F(40)
    d[0:14, 0:14] = F(22)
    d[20:27, 55:62] = NAN
    d[23, 58] = F(75.5)
    d[28:33, 20:24] = INF
    for k, v in enumerate([INF, NAN, -INF, INF, NAN, -INF, INF, NAN]):
        d[3 + 2 * k, 45 + (5 * k) % 9] = F(v)
    d[16, 0] = d[0, 16] = d[32, 48] = INF
    d[0, 48] = d[18, 33] = F(500)  # (on the lattices of steps 1, 3 and 16 / 1 and 3: spikes no gate reaches, valid but unused)
    d[0:11, 58:66] *= F(-1)
    return np.ascontiguousarray(d)


def tiles_map(step):
    """131 x 70: lattice rows of 131 (step 1) or 66 (step 2) points, so chunks of 64 lattice points wrap rows; holes on and next to the
    lattice columns 63 / 64 / 127 / 128 and on the first and last lattice row and column; spikes that stay unused."""
    W, H = 131, 70
    d = slanted(W, H, d0=30.0, gx=0.11, gy=-0.07, noise=0.2, seed=5)
    d[40:, 70:] += F(6)
    Wl, Hl = M.lattice(W, step), M.lattice(H, step)
    holes = [(5, 63), (6, 64), (9, 62), (9, 65), (0, 0), (0, 30), (Hl - 1, 17), (20, 0), (33, Wl - 1), (Hl - 1, Wl - 1), (Hl // 2, Wl // 2)]
    holes += [(12, 127), (13, 128), (15, 126), (15, 129)] if Wl > 129 else [(12, 1), (13, 2)]
    for j, i in holes:
        d[j * step, i * step] = INF
    d[31 * step:33 * step + 1, 62 * step:66 * step + 1] = NAN
    for j, i in ((25, 63), (26, 64), (27, 0), (28, Wl - 1), (3, 40)):  # spikes no gate reaches: valid lattice pixels that no triangle uses
        d[j * step, i * step] = F(500)
    return np.ascontiguousarray(d)


def image_for(W, H, seed=1):
    return np.random.default_rng(1000 + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


# (name, map builder, doffs of the calibration or None for no calibration, max_diff, step)
CASES = [
    ("none_1x1", lambda: np.full((1, 1), 10, F), None, 1.0, 1),
    ("none_1x40", lambda: slanted(40, 1, 10.0, 0.01, 0.0), 0.0, 1.0, 1),
    ("none_40x1", lambda: slanted(1, 40, 10.0, 0.0, 0.01), None, 1.0, 1),
    ("none_step_above_size", lambda: slanted(9, 7, 10.0, 0.01, 0.01), None, INF, 16),
    # 2 x 2, all valid
    ("quad_ad", lambda: quad(10, 10.5, 10.2, 10.1), 0.0, 1.0, 1),
    ("quad_bc", lambda: quad(10, 10.1, 10.2, 10.8), 0.0, 1.0, 1),
    ("quad_tie", lambda: quad(10, 11, 12, 11), 0.0, 2.0, 1),
    ("quad_nan_b", lambda: quad(10, NAN, 10.2, 10.1), None, 1.0, 1),  # (uncalibrated: NaN is "valid" and joins nothing)
    ("quad_nan_d", lambda: quad(10, 10.1, 10.2, NAN), None, 1.0, 1),
    # 2 x 2, three valid corners
    ("quad_miss_a", lambda: quad(INF, 10.1, 10.2, 10.3), 0.0, 1.0, 1),
    ("quad_miss_b", lambda: quad(10, INF, 10.2, 10.3), 0.0, 1.0, 1),
    ("quad_miss_c", lambda: quad(10, 10.1, -INF, 10.3), None, 1.0, 1),
    ("quad_miss_d", lambda: quad(10, 10.1, 10.2, NAN), 0.0, 1.0, 1),
    ("quad_two_valid", lambda: quad(10, INF, INF, 10.1), 0.0, 1.0, 1),
    # 2 x 2, gated: each of the five relevant edges cut in turn by max_diff = 1 (AD is the diagonal in all five)
    ("gate_cut_ab", lambda: quad(10, 11.2, 10.3, 10.6), 0.0, 1.0, 1),
    ("gate_cut_ac", lambda: quad(10, 10.3, 11.2, 10.6), 0.0, 1.0, 1),
    ("gate_cut_bd", lambda: quad(10.6, 11.2, 10.3, 10), 0.0, 1.0, 1),
    ("gate_cut_cd", lambda: quad(10.6, 10.3, 11.2, 10), 0.0, 1.0, 1),
    ("gate_cut_ad", lambda: quad(10, 10.5, 11.7, 11.1), 0.0, 1.0, 1),
    ("gate_zero_constant", lambda: np.full((4, 5), 12.5, F), 0.0, 0.0, 1),
    ("gate_zero_slanted", lambda: slanted(5, 4, 10.0, 0.25, 0.5), 0.0, 0.0, 1),
    ("gate_inf", lambda: slanted(5, 4, 10.0, 0.1, 0.1, noise=5.0), None, INF, 1),
    # mixed, 67 x 35
    ("mixed_s1", mixed_map, None, 1.0, 1),
    ("mixed_s1_calib", mixed_map, -25.0, 1.0, 1),
    ("mixed_s3", mixed_map, None, 1.0, 3),
    ("mixed_s3_calib", mixed_map, -25.0, 1.0, 3),
    ("mixed_s16", mixed_map, None, 3.0, 16),
    ("mixed_s16_calib", mixed_map, -25.0, 3.0, 16),
    # tiles, 131 x 70
    ("tiles_s1", lambda: tiles_map(1), 0.0, 1.0, 1),
    ("tiles_s2", lambda: tiles_map(2), 0.0, 1.0, 2),
]
CASE_NAMES = [c[0] for c in CASES]
MIXED = [n for n in CASE_NAMES if n.startswith("mixed_")]
CAPACITY_CASE = "tiles_s1"


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(map, image, calib (tuple or None), max_diff, step, size, lattice) of a named case."""
    k = CASE_NAMES.index(name)
    _, build, doffs, max_diff, step = CASES[k]
    m = np.ascontiguousarray(build(), F)
    m.setflags(write=False)
    H, W = m.shape
    img = image_for(W, H, k)
    img.setflags(write=False)
    return dict(map=m, image=img, calib=None if doffs is None else calib_for(W, H, doffs), max_diff=max_diff, step=step, size=(W, H),
                lattice=(M.lattice(W, step), M.lattice(H, step)))


@functools.lru_cache(maxsize=None)
def reference(name, with_image=True):
    """-> (vertices, vertex_index, triangles, report) of tests/mesh_ref.py, read-only"""
    c = case(name)
    out = M.mesh(c["map"], c["calib"], c["max_diff"], c["step"], c["image"] if with_image else None)
    for a in out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def flags(name):
    c = case(name)
    return M.cell_flags(c["map"], c["calib"], c["max_diff"], c["step"])


@functools.lru_cache(maxsize=None)
def capacities(name=CAPACITY_CASE):
    """(vertex capacities, triangle capacities): 0, 1, one below / at / one above the count in front of a chunk boundary (64 lattice
    points per chunk; the third chunk boundary, which lies inside a lattice row), the exact count -- all from the reference's counts."""
    c = case(name)
    Wl, Hl = c["lattice"]
    assert c["step"] == 1
    _, vidx, _, rep = reference(name)
    t0, t1, _ = flags(name)
    per_point = np.zeros((Hl, Wl), np.int64)
    per_point[:-1, :-1] = t0.astype(np.int64) + t1
    boundary = 3 * 64
    nv = int((vidx < boundary).sum())  # (step 1: the raster index is the lattice index)
    nt = int(per_point.ravel()[:boundary].sum())
    assert 1 < nv - 1 and nv + 1 < rep["vertices"] and 1 < nt - 1 and nt + 1 < rep["triangles"]
    return (0, 1, nv - 1, nv, nv + 1, rep["vertices"]), (0, 1, nt - 1, nt, nt + 1, rep["triangles"])


def _named():
    def rep(n):
        return reference(n)[3]

    def tri(n):
        return reference(n)[2].tolist()

    for n in ("none_1x1", "none_1x40", "none_40x1", "none_step_above_size"):
        assert rep(n)["vertices"] == rep(n)["triangles"] == 0 and rep(n)["lattice_valid"] > 0, (n, rep(n))
    assert case("none_step_above_size")["lattice"] == (1, 1)
    # vertex numbers of a full 2 x 2: A = 0, B = 1, C = 2, D = 3
    assert tri("quad_ad") == [[0, 2, 3], [0, 3, 1]] and tri("quad_tie") == [[0, 2, 3], [0, 3, 1]] and tri("quad_bc") == [[0, 2, 1], [1, 2, 3]]
    assert not flags("quad_ad")[2].any() and not flags("quad_tie")[2].any() and flags("quad_bc")[2].all()
    m = case("quad_tie")["map"]
    assert abs(m[0, 0] - m[1, 1]) == abs(m[0, 1] - m[1, 0])
    assert rep("quad_nan_b") == dict(lattice_valid=4, vertices=0, triangles=0, cells_two=0, cells_one=0)
    assert rep("quad_nan_d") == dict(lattice_valid=4, vertices=3, triangles=1, cells_two=0, cells_one=1) and tri("quad_nan_d") == [[0, 2, 1]]
    # three valid corners: the vertex numbers skip the missing corner
    assert tri("quad_miss_a") == [[0, 1, 2]] and tri("quad_miss_b") == [[0, 1, 2]] and tri("quad_miss_c") == [[0, 2, 1]] and tri("quad_miss_d") == [[0, 2, 1]]
    for n in ("quad_miss_a", "quad_miss_b", "quad_miss_c", "quad_miss_d"):
        assert rep(n) == dict(lattice_valid=3, vertices=3, triangles=1, cells_two=0, cells_one=1), (n, rep(n))
    assert rep("quad_two_valid")["lattice_valid"] == 2 and rep("quad_two_valid")["triangles"] == 0
    # the gate: one side cut = the triangle on the other side of the diagonal AD survives; the diagonal cut = nothing
    assert tri("gate_cut_ab") == [[0, 1, 2]] and tri("gate_cut_cd") == [[0, 2, 1]]     # (A, C, D) without B / (A, D, B) without C
    assert tri("gate_cut_ac") == [[0, 2, 1]] and tri("gate_cut_bd") == [[0, 1, 2]]     # (A, D, B) without C / (A, C, D) without B
    assert rep("gate_cut_ad") == dict(lattice_valid=4, vertices=0, triangles=0, cells_two=0, cells_one=0)
    for n in ("gate_cut_ab", "gate_cut_ac", "gate_cut_bd", "gate_cut_cd", "gate_cut_ad"):
        assert not flags(n)[2].any(), n  # (AD is the diagonal)
    assert rep("gate_zero_constant") == dict(lattice_valid=20, vertices=20, triangles=24, cells_two=12, cells_one=0)
    assert rep("gate_zero_slanted")["triangles"] == 0 and rep("gate_inf") == dict(lattice_valid=20, vertices=20, triangles=24, cells_two=12, cells_one=0)
    assert flags("gate_inf")[2].any() and not flags("gate_inf")[2].all()
    m = mixed_map()
    assert np.isposinf(m).any() and np.isneginf(m).any() and np.isnan(m).any() and (m < 0).any()
    for n in MIXED + ["tiles_s1", "tiles_s2"]:
        c, r = case(n), rep(n)
        t0, t1, bc = flags(n)
        emitted = t0 | t1
        assert r["cells_two"] > 0 and r["cells_one"] > 0 and (emitted & bc).any() and (emitted & ~bc).any(), (n, r)   # both diagonals taken
        assert 0 < r["vertices"] < r["lattice_valid"] < c["lattice"][0] * c["lattice"][1], (n, r)                         # vertices dropped as unused
    for n in ("mixed_s1", "mixed_s3", "mixed_s16"):  # s <= 0 behind doffs = -25: fewer valid lattice pixels with the calibration
        assert rep(n + "_calib")["lattice_valid"] < rep(n)["lattice_valid"], n
    assert case("mixed_s3")["lattice"] == (23, 12) and (67 - 1) % 3 == 0 and (35 - 1) % 3 != 0 and case("mixed_s16")["lattice"] == (5, 3)
    assert case("tiles_s1")["lattice"] == (131, 70) and case("tiles_s2")["lattice"] == (66, 35)
    capacities()


_named()
