"""CPU tier of the TSDF volume's triangle mesh: the generated case table (tools/gen_tsdf_mc_table.py against the committed header);
properties of tests/tsdf_mesh_ref.py (the definition the GPU tests hold the kernels to): closedness on random signs, a sphere's Euler
characteristic and signed volume, the vertex list, unseen voxels; the header the kernels include (adcensus_amd/csrc/tsdf_cell.h),
compiled alone under g++ into a serial program (tests/emul/emul_tsdf_mesh.cpp) and held to the reference bit for bit on every case,
once more under ASAN + UBSAN as its own executable; and the new surface of the C ABI, the Python mirror, the facade and the CLI --
declared, exported, every refusal before a HIP call, --tsdf-mesh without --tsdf, the sanitizer build of the CLI on the stub."""
import collections
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import tsdf_cases as TC
from tests import tsdf_mesh_cases as MC
from tests import tsdf_mesh_ref as MR
from tests import tsdf_ref as T
from tests.test_tsdf_api import SAN_ENV, c_params, read_pfm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
GEN = MR.GEN
F = np.float32


# ---------------------------------------------------------------------------------------------- the table
def test_committed_table_equals_the_generator():
    assert open(GEN.HEADER).read() == GEN.header_text()
    M, rows = GEN.table()
    assert M == MR.M == 5 and len(rows) == 256 and GEN.row_bytes(M) == 16
    for text in (open(HEADER).read(), open(os.path.join(ROOT, "DESIGN.md")).read()):
        assert "M = 5" in text


def test_table_rows():
    M, rows = GEN.table()
    assert rows[0] == [] and rows[255] == [] and rows[1] == [(0, 4, 8)]
    for corner in range(8):
        assert len(rows[1 << corner]) == 1 and len(rows[255 ^ (1 << corner)]) == 1
    for case, tris in enumerate(rows):
        changing = {e for e in range(12) if (case >> GEN.edge_corners(e)[0] & 1) != (case >> GEN.edge_corners(e)[1] & 1)}
        assert {e for t in tris for e in t} == changing, case
        assert all(len(set(t)) == 3 for t in tris) and len(tris) <= M
        # an edge of a triangle that joins two cell edges of one face is a face segment, never a fan diagonal: used by ONE triangle
        used = collections.Counter(frozenset(x) for a, b, c in tris for x in ((a, b), (b, c), (c, a)))
        assert all(n == 1 for pair, n in used.items() if GEN.in_one_face(*pair)) and all(n == 2 for pair, n in used.items() if not GEN.in_one_face(*pair)), case
    # the owner offsets of the edges, as the definition lists them
    assert [GEN.edge_owner(e) for e in range(12)] == [((0, 0, 0), 0), ((0, 1, 0), 0), ((0, 0, 1), 0), ((0, 1, 1), 0), ((0, 0, 0), 1), ((1, 0, 0), 1), ((0, 0, 1), 1),
                                                     ((1, 0, 1), 1), ((0, 0, 0), 2), ((1, 0, 0), 2), ((0, 1, 0), 2), ((1, 1, 0), 2)]


def test_table_orientation_on_single_cells():
    """Every case as one cell with t = -+1000 (every vertex on its edge's midpoint).  The triangles and the negative parts of the
    cell's faces bound the negative region, so the triangles' summed area vector is minus that of those face parts; the negative part
    of a face grows with its number of negative corners (1/8, 1/4 or 1/2, 7/8, 1).  So the summed area vector has a positive component
    along (centroid of the positive corners - centroid of the negative corners) whenever the two centroids differ: the normals point
    from the negative corners to the positive side."""
    p = T.params(4, 4, 4, 1.0, (0.0, 0.0, 0.0), 1.0)
    checked = 0
    for case in range(1, 255):
        t = np.full((4, 4, 4), 1000, np.int64)
        w = np.zeros((4, 4, 4), np.int64)
        for c in range(8):
            di, dj, dk = GEN.corner(c)
            t[dk, dj, di] = -1000 if case >> c & 1 else 1000
            w[dk, dj, di] = 1
        v, tri, rep = MR.mesh((T.make_words(t, w), None), p, 1)
        assert rep["cells_seen"] == 1 and len(tri) == len(GEN.table()[1][case])
        P = np.stack([v["x"], v["y"], v["z"]], -1).astype(np.float64)[tri.astype(np.int64)]
        area = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]).sum(0) / 2
        corners = np.array([GEN.corner(c) for c in range(8)], np.float64)
        neg = np.array([bool(case >> c & 1) for c in range(8)])
        diff = corners[~neg].mean(0) - corners[neg].mean(0)
        assert (area * diff >= 0).all(), case
        if np.abs(diff).max() > 0:
            assert area @ diff > 1e-9, case
            checked += 1
    assert checked > 200


# ---------------------------------------------------------------------------------------------- properties of the reference alone
def _directed_edges(tri):
    e = collections.Counter()
    for a, b, c in tri.tolist():
        e[(a, b)] += 1
        e[(b, c)] += 1
        e[(c, a)] += 1
    return e


SEEDS = (0, 1, 2, 3, 4, 5)


def _closed_mesh(seed):
    return MR.mesh(MC.closed_volume(seed), T.params(14, 11, 9, 0.05, (0.0, 0.0, 0.0), 0.15), 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_closed_surface_every_directed_edge_once(seed):
    """A fully seen 14 x 11 x 9 volume, random signs inside, an all-positive outermost layer (ambiguous faces occur): every directed
    edge (a, b) of the triangle list occurs exactly once and (b, a) exactly once.

    This holds because no fan diagonal joins two edges of one cell face (tools/gen_tsdf_mc_table.py chooses the fan's apex so): an edge
    between two vertices of a shared face is then always a face segment, which both cells draw once, in opposite directions.  (With the
    apex always at the loop's lowest edge, seeds 0 and 2 had 12 and 8 directed edges twice: a diagonal inside an ambiguous face, drawn
    by both cells.)"""
    tri = _closed_mesh(seed)[1]
    e = _directed_edges(tri)
    bad = {k: n for k, n in e.items() if n != 1 or e.get((k[1], k[0]), 0) != 1}
    print("seed %d: %d triangles, %d directed edges, %d of them not exactly once: %s" % (seed, len(tri), len(e), len(bad), sorted(bad.items())[:6]))
    assert len(tri) > 2000 and not bad


@pytest.mark.parametrize("seed", SEEDS)
def test_closed_surface_is_balanced(seed):
    """the same volumes: every directed edge occurs as often as its reverse (no boundary, consistent orientation)"""
    v, tri, rep = _closed_mesh(seed)
    e = _directed_edges(tri)
    assert len(tri) > 2000 and all(e.get((b, a), 0) == n for (a, b), n in e.items())
    assert len(np.unique(tri)) == len(v)  # (fully seen, all-positive border: every crossing is used)
    cases = MR.cells(MC.closed_volume(seed)[0], 1)[1]
    ambiguous = sum(1 for c in np.unique(cases) if any(len({(c >> q & 1) for q in quad}) == 2 and (c >> quad[0] & 1) == (c >> quad[3] & 1) != (c >> quad[1] & 1) == (c >> quad[2] & 1)
                                                         for quad in ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (2, 3, 6, 7), (0, 2, 4, 6), (1, 3, 5, 7))))
    assert ambiguous > 20  # (ambiguous faces do occur)


def test_sphere_is_a_sphere():
    """t < 0 inside a sphere of radius 7.2 voxels in 24^3: Euler characteristic 2 over the used vertices, positive signed volume"""
    v, tri, rep = MC.reference("sphere24", 1)
    used = np.unique(tri)
    edges = {tuple(sorted(x)) for a, b, c in tri.tolist() for x in ((a, b), (b, c), (c, a))}
    assert len(used) == len(v) and len(used) - len(edges) + len(tri) == 2
    e = _directed_edges(tri)
    assert all(n == 1 and e.get((b, a), 0) == 1 for (a, b), n in e.items())
    P = np.stack([v["x"], v["y"], v["z"]], -1).astype(np.float64)
    volume = np.linalg.det(P[tri.astype(np.int64)]).sum() / 6
    exact = 4 / 3 * np.pi * (7.2 * 0.05) ** 3
    print("sphere: signed volume %.5f, analytic %.5f" % (volume, exact))
    assert volume > 0 and abs(volume - exact) < 0.05 * exact


@pytest.mark.parametrize("name", MC.EMUL_CASES)
def test_vertices_are_the_extraction_and_the_report_adds_up(name):
    c = MC.case(name)
    for mw in MC.MIN_WEIGHTS:
        v, tri, rep = MC.reference(name, mw)
        pts, xrep = T.extract(c["volume"], c["params"], mw)
        assert v.tobytes() == pts.tobytes() and rep["vertices"] == xrep["points"] and rep["voxels_seen"] == xrep["voxels_seen"]
        assert rep["triangles"] == len(tri) and rep["cells_surface"] <= rep["cells_seen"] and (len(tri) == 0 or tri.max() < len(v))
        for vcap, tcap in ((0, 0), (1, 2), (len(v) + 3, len(tri) + 3)):
            v2, t2, rep2 = MR.mesh(c["volume"], c["params"], mw, vcap, tcap)
            assert v2.tobytes() == v[:vcap].tobytes() and np.array_equal(t2, tri[:tcap]) and rep2 == rep
    if name == "all_cases":
        assert MC.reference(name, 1)[2]["cells_seen"] == 256 and MC.reference(name, 1)[2]["triangles"] == sum(len(r) for r in MR.TABLE)


def _cell_of_triangle(tsdf, min_weight):
    seen, case = MR.cells(tsdf, min_weight)
    counts = np.array([len(r) for r in MR.TABLE])[case] * seen
    nz, ny, nx = tsdf.shape
    n = (np.arange(nz - 1)[:, None, None] * ny + np.arange(ny - 1)[None, :, None]) * nx + np.arange(nx - 1)[None, None, :]
    return np.repeat(n.ravel(), counts.ravel())


def test_unseen_voxels_remove_exactly_the_cells_that_touch_them():
    """random weights below min_weight: the triangles (as triples of positions) are those of the fully seen volume whose cell touches
    no unseen voxel, in the same order"""
    nx, ny, nz = 16, 12, 10
    p = T.params(nx, ny, nz, 0.05, (0.0, 0.0, 0.0), 0.15)
    rng = np.random.default_rng(77)
    t = rng.integers(1, T.Q + 1, (nz, ny, nx)) * rng.choice([-1, 1], (nz, ny, nx))
    full = T.make_words(t, np.full((nz, ny, nx), 3))
    w = np.where(rng.random((nz, ny, nx)) < 0.06, rng.integers(0, 3, (nz, ny, nx)), 3)
    holes = T.make_words(t, w)
    vf, tf, rf = MR.mesh((full, None), p, 3)
    vh, th, rh = MR.mesh((holes, None), p, 3)
    unseen = w < 3
    touched = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        di, dj, dk = GEN.corner(c)
        touched |= unseen[dk:nz - 1 + dk, dj:ny - 1 + dj, di:nx - 1 + di]
    assert 0 < touched.sum() < touched.size and rh["cells_seen"] == int((~touched).sum()) and rf["cells_seen"] == touched.size
    nn = (np.arange(nz - 1)[:, None, None] * ny + np.arange(ny - 1)[None, :, None]) * nx + np.arange(nx - 1)[None, None, :]
    keep = ~np.isin(_cell_of_triangle(full, 3), nn[touched])

    def positions(v, tri):
        return np.stack([v["x"], v["y"], v["z"]], -1)[tri.astype(np.int64)]

    assert len(th) == keep.sum() and np.array_equal(positions(vf, tf)[keep], positions(vh, th))
    assert np.array_equal(_cell_of_triangle(holes, 3), _cell_of_triangle(full, 3)[keep])


# ---------------------------------------------------------------------------------------------- the shared header, serially
def _build_emul(tmp, sanitize):
    exe = os.path.join(tmp, "emul_tsdf_mesh_san" if sanitize else "emul_tsdf_mesh")
    cmd = ["g++", "-std=c++17", "-O1" if sanitize else "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "emul", "emul_tsdf_mesh.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emul_tsdf_mesh(tmp_path_factory):
    return _build_emul(str(tmp_path_factory.mktemp("emul_tsdf_mesh")), False)


def _run_emul(exe, name, mw, tmp):
    c = MC.case(name)
    v, tri, rep = MC.reference(name, mw)
    d = os.path.join(tmp, "%s_%d" % (name, mw))
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "case.bin"), "wb") as f:
        f.write(bytes(c_params(c["params"])) + struct.pack("<i", mw))
    c["volume"][0].tofile(os.path.join(d, "tsdf.bin"))
    if c["volume"][1] is not None:
        c["volume"][1].tofile(os.path.join(d, "color.bin"))
    run = subprocess.run([exe, d, d], env=SAN_ENV, capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr and "LeakSanitizer" not in run.stderr, run.stderr[-3000:]
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert open(os.path.join(d, "vertices.bin"), "rb").read() == v.tobytes(), name
    assert open(os.path.join(d, "triangles.bin"), "rb").read() == tri.tobytes(), name
    assert np.fromfile(os.path.join(d, "report.bin"), np.uint32).tolist() == MR.report_words(rep) + [0, 0, 0], name
    return d


@pytest.mark.parametrize("name", MC.EMUL_CASES)
def test_shared_header_equals_the_reference(emul_tsdf_mesh, name, tmp_path):
    for mw in MC.MIN_WEIGHTS:
        _run_emul(emul_tsdf_mesh, name, mw, str(tmp_path))


def test_shared_header_under_sanitizers(tmp_path):
    """The same program built once with ASAN + UBSAN and run as its own executable: a read outside the volume, the table or the rank
    array, an overflowing integer and a leak are reports, and a report is a failure."""
    exe = _build_emul(str(tmp_path), True)
    for name in MC.EMUL_CASES:
        for mw in MC.MIN_WEIGHTS:
            d = _run_emul(exe, name, mw, str(tmp_path))
    assert subprocess.run([exe], env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe, str(tmp_path / "absent"), str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2
    blob = bytearray(open(os.path.join(d, "case.bin"), "rb").read())
    blob[0:4] = struct.pack("<i", 6)  # nx no multiple of 4
    open(os.path.join(d, "case.bin"), "wb").write(bytes(blob))
    assert subprocess.run([exe, d, str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name in A.TSDF_MESH_ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    for phrase in ("M * (nx - 1)(ny - 1)(nz - 1) > 2^32 - 1", "4 bytes per voxel", "zero-area triangles occur and are kept", "counts only",
                   "whatever the vertex capacity", "not a product of adc_products or the farm"):
        assert phrase in text, phrase
    for lib in (A.LIB_PATH, os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(A.TSDF_MESH_ENTRY_POINTS) <= names, lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu", sizeof(adc_tsdf_mesh_report), offsetof(adc_tsdf_mesh_report, cells_surface), sizeof(adc_tsdf_extract_params)); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(A.TsdfMeshReport), A.TsdfMeshReport.cells_surface.offset, C.sizeof(A.TsdfExtractParams)] == [32, 16, 32]
    assert [f[0] for f in A.TsdfMeshReport._fields_] == list(MR.REPORT_FIELDS) + ["reserved_"]
    assert MR.count_limit_refused(2048, 1024, 512) and not MR.count_limit_refused(1024, 1024, 800) and not MR.count_limit_refused(512, 512, 512)


def test_every_refusal_comes_before_a_hip_call():
    """No device here: each of these returns 1 with a message without touching HIP.  A block of ones stands in for a handle that has a
    volume and a Match pending (every flag nonzero): the last check but one, so everything in front of it is reached on it; a zeroed
    block for an idle handle without a volume that has completed nothing."""
    L = A.lib()
    vp = C.c_void_p
    idle = C.cast(C.create_string_buffer(1 << 20), vp)
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), vp)
    dev = vp(4096)
    rep = A.TsdfMeshReport()

    def refused(rc, *words):
        msg = A.last_error()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    for who, call in (("adc_tsdf_mesh_device", lambda h, p=None, v=dev, vc=10, t=dev, tc=10: L.adc_tsdf_mesh_device(h, None if p is None else C.byref(p), v, vc, t, tc, None)),
                      ("adc_tsdf_mesh", lambda h, p=None, v=dev, vc=10, t=dev, tc=10: L.adc_tsdf_mesh(h, None if p is None else C.byref(p), v, vc, t, tc, C.byref(rep)))):
        refused(call(None), who, "null handle")
        for mw in (0, 65536, 2 ** 32 - 1):
            refused(call(busy, A.TsdfExtractParams(mw)), who, "min_weight")
        for k in range(7):
            p = A.TsdfExtractParams()
            p.reserved_[k] = 1
            refused(call(busy, p), who, "reserved")
        refused(call(busy, None, None, 0, None, 0), who, "neither vertices nor triangles")
        refused(call(busy, None, None, 5, dev, 5), who, "null vertices with a capacity")
        refused(call(busy, None, dev, 5, None, 5), who, "null triangles with a capacity")
        refused(call(idle), who, "no volume")
        for args in ((None, dev, 10, dev, 10), (A.TsdfExtractParams(65535), dev, 0, None, 0), (None, None, 0, dev, 0)):
            refused(call(busy, *args), who, "Match is pending")
    for bad in (4096 + 4, 4096 + 8, 4096 + 1):
        refused(L.adc_tsdf_mesh_device(busy, None, vp(bad), 10, None, 0, None), "adc_tsdf_mesh_device", "d_vertices must be 16-byte aligned")
    for bad in (4097, 4098, 4099):
        refused(L.adc_tsdf_mesh_device(busy, None, None, 0, vp(bad), 10, None), "adc_tsdf_mesh_device", "d_triangles must be 4-byte aligned")
        refused(L.adc_tsdf_mesh_device(busy, None, dev, 10, None, 0, vp(bad)), "adc_tsdf_mesh_device", "d_counts must be 4-byte aligned")
    refused(L.adc_get_tsdf_mesh_report(None, C.byref(rep)), "null")
    refused(L.adc_get_tsdf_mesh_report(idle, None), "null")
    refused(L.adc_get_tsdf_mesh_report(idle, C.byref(rep)), "no mesh call")
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    st.width, st.height = 8, 4
    assert st.tsdf_mesh_device(4096, 4, 4096, 4) is False and st.tsdf_mesh_report() is None
    with pytest.raises(RuntimeError):
        st.tsdf_mesh()
    with pytest.raises(ValueError):
        st.tsdf_mesh(vertices=False, triangles=False)


CALLER = r'''
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
int main() {
    ADCensusStereo s; ADCensusOption o;
    uint8 img[96] = {0};
    float32 d[32] = {0};
    adc_tsdf_extract_params x = {1u, {0u, 0u, 0u, 0u, 0u, 0u, 0u}};
    adc_tsdf_mesh_report rep;
    adc_point vtx[8];
    uint32 tri[24];
    // before Initialize there is no matcher underneath: everything is refused
    bool ok = !s.TsdfMesh(&x, vtx, 8, tri, 8, &rep) && !s.TsdfMesh(nullptr, nullptr, 0, tri, 0, nullptr) && !s.GetTsdfMeshReport(&rep);
    return (ok && !s.Match(img, img, d) && !s.Initialize(0, 0, o)) ? 0 : 1;
}
'''


def test_facade_compiles_and_exports_the_members(tmp_path):
    src = tmp_path / "caller.cpp"
    src.write_text(CALLER)
    libdir = os.path.join(ROOT, "adcensus_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libadcensus.so")):
        pytest.fail("libadcensus.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "caller"),
                    "-L", libdir, "-ladcensus", "-ladcensus_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(libdir, "libadcensus.so")], capture_output=True, text=True, check=True).stdout
    for member in ("TsdfMesh(adc_tsdf_extract_params const*, adc_point*, unsigned long, unsigned int*, unsigned long, adc_tsdf_mesh_report*)",
                   "GetTsdfMeshReport(adc_tsdf_mesh_report*)"):
        assert "ADCensusStereo::" + member in out, member
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def test_cli_rejects_tsdf_mesh_without_tsdf(tmp_path):
    """Checked while the arguments are parsed: the images named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    base = [cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "0", "64", str(tmp_path / "out")]
    calib = ["--calib", "100,0.16,40,20,0"]
    for args in (base + ["--tsdf-mesh"], base + calib + ["--tsdf-mesh"], [base[0], "--tsdf-mesh"] + base[1:] + calib):
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and r.stdout.startswith("--tsdf-mesh refused: it needs --tsdf") and "Image Loading" not in r.stdout, r.stdout
    for args in (base + calib + ["--tsdf", "8,8,8,0.1,0,0,1", "--tsdf-mesh"], [base[0], "--tsdf-mesh", "--tsdf", "8,8,8,0.1,0,0,1"] + base[1:] + calib):
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Image Loading" in r.stdout and "refused" not in r.stdout, r.stdout  # (well-formed: gets as far as the images)


def read_tsdf_mesh_ply(path):
    """-> (vertices as tests/tsdf_ref.py records with pad 0, triangles uint32 [.][3]); the whole file must be accounted for"""
    with open(path, "rb") as f:
        blob = f.read()
    head, body = blob.split(b"end_header\n", 1)
    m = re.fullmatch(rb"ply\nformat binary_little_endian 1.0\nelement vertex (\d+)\nproperty float x\nproperty float y\nproperty float z\n"
                     rb"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face (\d+)\nproperty list uchar int vertex_indices\n", head)
    assert m, head
    nv, nt = int(m.group(1)), int(m.group(2))
    assert len(body) == 15 * nv + 13 * nt
    rec = np.frombuffer(body[:15 * nv], np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    out = np.zeros(nv, T.POINT_DTYPE)
    out["x"], out["y"], out["z"] = rec["xyz"][:, 0], rec["xyz"][:, 1], rec["xyz"][:, 2]
    out["r"], out["g"], out["b"] = rec["rgb"][:, 0], rec["rgb"][:, 1], rec["rgb"][:, 2]
    faces = np.frombuffer(body[15 * nv:], np.dtype([("n", "u1"), ("v", "<u4", 3)]))
    assert (faces["n"] == 3).all()
    return out, faces["v"].copy()


def test_cli_tsdf_mesh_under_sanitizers(tmp_path):
    """<out>-tsdf-mesh.ply in the ASAN / UBSAN build on the stub C ABI, whose mesh is tsdf_cell.h run serially: a well-formed ply that
    equals tests/tsdf_mesh_ref.py on the run's .pfm; -tsdf.ply and every other file of the run are byte-identical to a run without
    the flag."""
    from PIL import Image
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "adcensus_amd", "host"), "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cli = os.path.join(ROOT, "adcensus_amd", "build", "asan", "adcensus_cli_asan")
    rng = np.random.default_rng(12)
    w, h = 83, 57
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "l.png")
    Image.fromarray(rgb[:, ::-1].copy()).save(tmp_path / "r.png")
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    calib = (70.0, 0.16, 41.3, 28.2, 1.25)
    calib_arg = ["--calib", ",".join("%.9g" % v for v in calib)]
    R, t = TC.rot(3.0, -4.0, 2.0), (0.02, -0.01, 0.03)
    (tmp_path / "pose.txt").write_text("\n".join("%.9g" % v for v in R + t))

    def run(pref, *extra):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "-3", "29", str(tmp_path / pref), *extra], env=SAN_ENV,
                           capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, r.stdout
        return r.stdout

    total = 0
    for pref, spec, trunc, mw, pose in (("m1", "32,24,32,0.04,-0.64,-0.48,0.35", 0.04 * 3, 1, False), ("m2", "36,20,28,0.05,-0.9,-0.5,0.3,0.2,1", 0.2, 1, True)):
        tsdf_args = ["--tsdf", spec, *calib_arg, *(["--pose", str(tmp_path / "pose.txt")] if pose else [])]
        run(pref + "_plain", *tsdf_args)
        out = run(pref, "--tsdf-mesh", *tsdf_args)
        names = sorted(f[len(pref + "_plain"):] for f in os.listdir(tmp_path) if f.startswith(pref + "_plain-") or f.startswith(pref + "_plain."))
        assert len(names) >= 5 and "-tsdf.ply" in names and "-tsdf-mesh.ply" not in names
        for suffix in names:
            assert open(str(tmp_path / (pref + "_plain")) + suffix, "rb").read() == open(str(tmp_path / pref) + suffix, "rb").read(), (pref, suffix)
        v = spec.split(",")
        p = T.params(int(v[0]), int(v[1]), int(v[2]), float(v[3]), [float(x) for x in v[4:7]], float(F(3.0) * F(v[3])) if len(v) == 7 else trunc, flags=T.COLOR)
        fr = T.frame(calib, R, t) if pose else T.frame(calib)
        vol, _ = T.integrate(T.empty(p), p, fr, read_pfm(str(tmp_path / pref) + ".pfm"), bgr)
        wv, wt, wrep = MR.mesh(vol, p, mw)
        wv = wv.copy()
        wv["pad"] = 0  # (the file does not carry the weight)
        gv, gt = read_tsdf_mesh_ply(str(tmp_path / pref) + "-tsdf-mesh.ply")
        assert gv.tobytes() == wv.tobytes() and np.array_equal(gt, wt), pref
        assert "TSDF mesh: %u voxels seen, %u vertices, %u triangles, %u cells seen, %u surface cells\n" % tuple(MR.report_words(wrep)) in out, out
        total += len(wt)
    assert total > 300
