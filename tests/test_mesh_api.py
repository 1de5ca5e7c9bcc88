"""CPU tier of the triangle mesh from a disparity map: properties of tests/mesh_ref.py (the definition the GPU tests hold the kernels
to) on the cases of tests/mesh_cases.py; the header the kernels include (adcensus_amd/csrc/mesh_cell.h), compiled alone under g++ into
a serial program (tests/emul/emul_mesh.cpp) and held to the reference bit for bit on every case, once more under ASAN + UBSAN as its
own executable; and the new surface of the C ABI, the Python mirror, the facade and the CLI -- declared, exported, struct layouts,
every refusal before a HIP call, malformed --mesh, the sanitizer build of the CLI on the stub."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import mesh_cases as MC
from tests import mesh_ref as M
from tests import normals_ref as N
from tests import outputs_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
ENTRY_POINTS = ["adc_mesh_device", "adc_mesh", "adc_get_mesh_report"]
F = np.float32
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


# ---------------------------------------------------------------------------------------------- properties of the reference alone
@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_reference_properties(name):
    c = MC.case(name)
    v, vi, t, rep = MC.reference(name)
    W, H = c["size"]
    step = c["step"]
    assert rep["triangles"] == 2 * rep["cells_two"] + rep["cells_one"] == len(t) and rep["vertices"] == len(v) == len(vi)
    assert (t < len(v)).all()                                               # every vertex number is < vertices
    assert np.array_equal(np.unique(t), np.arange(len(v)))                  # every vertex is referenced
    assert (np.diff(vi) > 0).all()                                          # strictly ascending ...
    ys, xs = np.divmod(vi.astype(np.int64), W)
    assert (ys < H).all() and (xs % step == 0).all() and (ys % step == 0).all()  # ... and on the lattice
    a = np.abs(c["map"]).ravel()[vi]
    valid = (a != np.inf) if c["calib"] is None else O.depth(a, c["calib"])[1]
    assert valid.all()
    for p, q in ((0, 1), (1, 2), (2, 0)):                                   # every triangle edge is joined
        with np.errstate(invalid="ignore"):
            assert (np.abs(a[t[:, p]] - a[t[:, q]]) <= F(c["max_diff"])).all()
        assert (np.abs(xs[t[:, p]] - xs[t[:, q]]) <= step).all() and (np.abs(ys[t[:, p]] - ys[t[:, q]]) <= step).all()
    x, y = xs[t], ys[t]
    cross = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    assert (cross == -step * step).all()                                    # one winding sign in pixel coordinates, half a cell each
    # without the image the colours are 0 and nothing else changes
    v0, vi0, t0, rep0 = MC.reference(name, False)
    assert rep0 == rep and np.array_equal(vi0, vi) and np.array_equal(t0, t)
    for k in "xyz":
        assert np.array_equal(v0[k].view(np.uint32), v[k].view(np.uint32))
    assert not (v0["r"].any() or v0["g"].any() or v0["b"].any() or v["pad"].any())
    if len(v):
        img = c["image"].reshape(-1, 3)[vi]
        assert np.array_equal(v["r"], img[:, 2]) and np.array_equal(v["g"], img[:, 1]) and np.array_equal(v["b"], img[:, 0])


def test_normal_of_a_fronto_parallel_patch_points_at_the_camera():
    """Z > 0, constant disparity: (v1 - v0) x (v2 - v0) has a negative z for every triangle, as the normals of adc_normals have."""
    d = np.full((6, 7), 20, F)
    v, _, t, _ = M.mesh(d, MC.calib_for(7, 6, 0.0), 1.0, 1)
    p = np.stack([v["x"], v["y"], v["z"]], -1).astype(np.float64)
    nrm = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    assert len(t) == 60 and (nrm[:, 2] < 0).all() and (v["z"] > 0).all()
    out = N.normals(d, MC.calib_for(7, 6, 0.0), 1, 1.0, 3)[0]
    assert (out[..., 2] == -1).all()


def test_a_fully_valid_map_without_a_gate():
    """Wl * Hl vertices and 2 (Wl - 1)(Hl - 1) triangles; at step 1 the vertex records are the cloud of tests/outputs_ref.py bit for bit."""
    W, H = 23, 17
    rng = np.random.default_rng(4)
    d = rng.uniform(1, 60, (H, W)).astype(F)
    d[3, 4] *= F(-1)
    img = MC.image_for(W, H, 99)
    for calib in (None, MC.calib_for(W, H, 0.0), MC.calib_for(W, H, 1.75)):
        for step in (1, 2, 5, 16):
            Wl, Hl = M.lattice(W, step), M.lattice(H, step)
            v, vi, t, rep = M.mesh(d, calib, np.inf, step, img)
            assert rep == dict(lattice_valid=Wl * Hl, vertices=Wl * Hl, triangles=2 * (Wl - 1) * (Hl - 1), cells_two=(Wl - 1) * (Hl - 1), cells_one=0)
            cloud = O.cloud(d, img, calib)
            assert len(cloud) == W * H and v.tobytes() == cloud[vi].tobytes()
            if step == 1:
                assert v.tobytes() == cloud.tobytes() and np.array_equal(vi, np.arange(W * H))
    for step in (16,):  # a step larger than both sizes: one lattice pixel, an empty mesh
        v, vi, t, rep = M.mesh(d[:9, :12], None, np.inf, step)
        assert (len(v), len(vi), len(t)) == (0, 0, 0) and rep == dict(lattice_valid=1, vertices=0, triangles=0, cells_two=0, cells_one=0)


def test_mixed_cloud_points_are_the_vertices():
    """On the mixed maps too a vertex record is the cloud's point of its pixel (the shared validity and arithmetic)."""
    for name in MC.MIXED:
        c = MC.case(name)
        v, vi, _, _ = MC.reference(name)
        a = np.abs(c["map"])
        valid = (a != np.inf) if c["calib"] is None else O.depth(c["map"], c["calib"])[1]
        rank = np.cumsum(valid.ravel()) - 1
        cloud = O.cloud(c["map"], c["image"], c["calib"])
        assert valid.ravel()[vi].all() and v.tobytes() == cloud[rank[vi]].tobytes(), name


# ---------------------------------------------------------------------------------------------- the shared header, serially
def _build_emul(tmp, sanitize):
    exe = os.path.join(tmp, "emul_mesh_san" if sanitize else "emul_mesh")
    cmd = ["g++", "-std=c++17", "-O1" if sanitize else "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "emul", "emul_mesh.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emul_mesh(tmp_path_factory):
    return _build_emul(str(tmp_path_factory.mktemp("emul_mesh")), False)


def _emul_args(c, with_image, ind, outd):
    W, H = c["size"]
    calib = c["calib"] or (0.0, 0.0, 0.0, 0.0, 0.0)
    return [str(W), str(H), str(int(c["calib"] is not None))] + ["%.9g" % v for v in calib] + ["%.9g" % c["max_diff"], str(c["step"]), str(int(with_image)), ind, outd]


def _run_emul(exe, name, tmp, with_image=True):
    c = MC.case(name)
    ind, outd = os.path.join(tmp, "in"), os.path.join(tmp, "out")
    os.makedirs(ind, exist_ok=True)
    os.makedirs(outd, exist_ok=True)
    c["map"].tofile(os.path.join(ind, "map.bin"))
    c["image"].tofile(os.path.join(ind, "img.bin"))
    r = subprocess.run([exe] + _emul_args(c, with_image, ind, outd), env=SAN_ENV, capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    v, vi, t, rep = MC.reference(name, with_image)
    assert open(os.path.join(outd, "vertices.bin"), "rb").read() == v.tobytes(), name
    assert np.array_equal(np.fromfile(os.path.join(outd, "vindex.bin"), np.int32), vi), name
    assert np.array_equal(np.fromfile(os.path.join(outd, "triangles.bin"), np.uint32).reshape(-1, 3), t), name
    assert np.fromfile(os.path.join(outd, "report.bin"), np.uint32).tolist() == M.report_words(rep) + [0, 0, 0], name


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_shared_header_equals_the_reference(emul_mesh, name, tmp_path):
    _run_emul(emul_mesh, name, str(tmp_path), True)
    _run_emul(emul_mesh, name, str(tmp_path), False)


def test_shared_header_under_sanitizers(tmp_path):
    """The same program built once with ASAN + UBSAN and run as its own executable: reads outside the map or the image, a vertex
    number taken from outside the lattice and a leak are reports, and a report is a failure."""
    exe = _build_emul(str(tmp_path), True)
    for name in MC.CASE_NAMES:
        _run_emul(exe, name, str(tmp_path), name != "tiles_s2")
    c = MC.case("quad_ad")
    assert subprocess.run([exe], env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe] + _emul_args(c, True, str(tmp_path / "absent"), str(tmp_path)), env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe] + _emul_args(dict(c, step=17), True, str(tmp_path / "in"), str(tmp_path)), env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe] + _emul_args(dict(c, max_diff=-1.0), True, str(tmp_path / "in"), str(tmp_path)), env=SAN_ENV, capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    assert re.search(r"#define\s+ADC_MESH_MAX_STEP\s+16\b", text) and A.MESH_MAX_STEP == M.MAX_STEP == 16
    for phrase in ("fabsf(a_p - a_q) <= max_diff", "ties go to AD", "D missing: (A, C, B)", "T0 before T1", "counts only", "not a product of adc_products or the farm"):
        assert phrase in text, phrase
    for lib in (A.LIB_PATH, os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(ENTRY_POINTS) <= names, lib
    # the struct layouts, asked of a C compiler; the existing structs keep theirs
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(adc_mesh_params), offsetof(adc_mesh_params, max_diff),\n'
                   ' offsetof(adc_mesh_params, step), offsetof(adc_mesh_params, flags), offsetof(adc_mesh_params, reserved_),\n'
                   ' sizeof(adc_mesh_report), offsetof(adc_mesh_report, cells_one), offsetof(adc_mesh_report, reserved_), sizeof(adc_point), sizeof(adc_calib),\n'
                   ' sizeof(adc_outputs), sizeof(adc_products), sizeof(adc_normals_params)); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    P, Rp = A.MeshParams, A.MeshReport
    assert got == [C.sizeof(P), P.max_diff.offset, P.step.offset, P.flags.offset, P.reserved_.offset, C.sizeof(Rp), Rp.cells_one.offset, Rp.reserved_.offset,
                   A.POINT_DTYPE.itemsize, C.sizeof(A.Calib), C.sizeof(A.Outputs), C.sizeof(A.Products), C.sizeof(A.NormalsParams)]
    assert got[0] == 32 and got[5] == 32 and got[8:] == [16, 20, 48, 80, 32]
    p = A.MeshParams()
    assert (p.max_diff, p.step, p.flags, list(p.reserved_)) == (1.0, 1, 0, [0, 0, 0, 0, 0])
    p = A.MeshParams(max_diff=float("inf"), step=16)
    assert (p.max_diff, p.step) == (float("inf"), 16)
    assert [f[0] for f in A.MeshReport._fields_] == list(M.REPORT_FIELDS) + ["reserved_"]


def test_every_refusal_comes_before_a_hip_call():
    """No device here: each of these returns 1 with a message without touching HIP.  A block of ones stands in for a handle with a
    Match pending (every flag nonzero): the last check of all, so everything in front of it is reached on it; a zeroed block for an
    idle handle that has completed nothing."""
    L = A.lib()
    vp = C.c_void_p
    assert L.adc_mesh_device.argtypes == [vp, vp, vp, C.POINTER(A.Calib), C.POINTER(A.MeshParams), vp, C.c_uint64, vp, vp, C.c_uint64, vp]
    assert L.adc_mesh.argtypes == [vp, vp, vp, C.POINTER(A.Calib), C.POINTER(A.MeshParams), vp, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(A.MeshReport)]
    idle = C.cast(C.create_string_buffer(1 << 20), vp)
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), vp)
    dev = vp(4096)
    good = A.Calib(100.0, 0.16, 10.0, 5.0, 0.0)
    rep = A.MeshReport()

    def refused(rc, *words):
        msg = A.last_error()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    def device(h, m, c=good, p=None, v=dev, vi=dev, t=dev, n=dev, img=dev):
        return L.adc_mesh_device(h, m, img, None if c is None else C.byref(c), None if p is None else C.byref(p), v, 100, vi, t, 100, n)

    def host(h, m, c=good, p=None, v=dev, vi=dev, t=dev, n=None, img=dev):
        return L.adc_mesh(h, m, img, None if c is None else C.byref(c), None if p is None else C.byref(p), v, 100, vi, t, 100, C.byref(rep))

    for who, call in (("adc_mesh_device", device), ("adc_mesh", host)):
        refused(call(None, dev), who, "null handle")
        refused(call(busy, None), who, "null map")
        for k in range(5):
            for v in (float("nan"), float("inf")):
                vals = [100.0, 0.16, 10.0, 5.0, 0.0]
                vals[k] = v
                refused(call(busy, dev, A.Calib(*vals)), who, "non-finite")
        for f in (0.0, -100.0):
            refused(call(busy, dev, A.Calib(f, 0.16, 10.0, 5.0, 0.0)), who, "focal_px must be positive")
        for md in (-1.0, -1e-30, float("nan"), -float("inf")):
            refused(call(busy, dev, good, A.MeshParams(max_diff=md)), who, "max_diff")
        for step in (0, -1, 17, 2 ** 31 - 1, -2 ** 31):
            refused(call(busy, dev, good, A.MeshParams(step=step)), who, "step")
        for flags in (1, 2, 0x80000000, 0xFFFFFFFF):
            refused(call(busy, dev, good, A.MeshParams(flags=flags)), who, "unknown flag")
        for k in range(5):
            p = A.MeshParams()
            p.reserved_[k] = 1
            refused(call(busy, dev, good, p), who, "reserved")
        refused(call(busy, dev, v=None, vi=None, t=None), who, "neither vertices nor triangles")
        refused(call(busy, dev, v=None, vi=dev, t=dev), who, "vertex_index needs vertices")
        # everything in range passes the argument checks and reaches the handle's state: no calibration, no image, every output set
        for p in (None, A.MeshParams(0.0, 1), A.MeshParams(float("inf"), 16), A.MeshParams(2.5, 3)):
            refused(call(busy, dev, good, p), who, "Match is pending")
            refused(call(busy, dev, None, p, img=None), who, "Match is pending")
        refused(call(busy, dev, v=dev, vi=None, t=None, n=None), who, "Match is pending")
        refused(call(busy, dev, v=None, vi=None, t=dev), who, "Match is pending")
    for bad in (4096 + 4, 4096 + 8, 4096 + 1):
        refused(device(busy, dev, v=vp(bad)), "adc_mesh_device", "16-byte aligned")
    for bad in (4096 + 1, 4096 + 2, 4096 + 3):
        for kw in (dict(vi=vp(bad)), dict(t=vp(bad)), dict(n=vp(bad))):
            refused(device(busy, dev, **kw), "adc_mesh_device", "4-byte aligned")
        refused(device(busy, vp(bad)), "adc_mesh_device", "4-byte aligned")
        refused(device(busy, dev, img=vp(bad)), "Match is pending")  # (bytes: the image may lie anywhere)
    refused(L.adc_get_mesh_report(None, C.byref(rep)), "null")
    refused(L.adc_get_mesh_report(idle, None), "null")
    refused(L.adc_get_mesh_report(idle, C.byref(rep)), "no mesh call")
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    st.width, st.height = 8, 4
    with pytest.raises(RuntimeError):
        st.mesh(np.zeros((4, 8), F))
    with pytest.raises(RuntimeError):
        st.mesh_report()
    assert st.mesh_device(4096, None, d_vertices=4096, vertex_capacity=32) is False


CALLER = r'''
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
int main() {
    ADCensusStereo s; ADCensusOption o;
    uint8 img[96] = {0};
    float32 d[32] = {0};
    adc_calib c = {100.f, 0.16f, 4.f, 2.f, 0.f};
    adc_mesh_params p = {1.0f, 1, 0u, {0u, 0u, 0u, 0u, 0u}};
    adc_mesh_report rep;
    adc_point v[32];
    sint32 vi[32];
    uint32 t[3 * 42];
    // before Initialize there is no matcher underneath: everything is refused
    bool ok = !s.Mesh(d, img, &c, &p, v, 32, vi, t, 42, &rep) && !s.Mesh(d, nullptr, nullptr, nullptr, nullptr, 0, nullptr, t, 42, nullptr) && !s.GetMeshReport(&rep);
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
    assert ("ADCensusStereo::Mesh(float const*, unsigned char const*, adc_calib const*, adc_mesh_params const*, adc_point*, unsigned long, int*, unsigned int*, "
            "unsigned long, adc_mesh_report*)") in out
    assert "ADCensusStereo::GetMeshReport(adc_mesh_report*)" in out
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def test_cli_rejects_malformed_mesh_flags(tmp_path):
    """Checked while the arguments are parsed: the images named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    base = [cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "0", "64", str(tmp_path / "out")]
    for bad in [["--mesh"], ["--mesh", ""], ["--mesh", "-1"], ["--mesh", "nan"], ["--mesh", "1,0"], ["--mesh", "1,17"], ["--mesh", "1,2,3"], ["--mesh", "1x"],
                ["--mesh", ","], ["--mesh", "1,"], ["--mesh", "1,-2"], ["--mesh", "1,2x"], ["--mesh", "one"], ["--mesh", "-inf"], ["--mesh", "1,2.5"]]:
        for front in (False, True):  # (anywhere after the program name)
            argv = [base[0]] + bad + base[1:] if front and len(bad) == 2 else base + bad
            r = subprocess.run(argv, capture_output=True, text=True, timeout=120)
            assert r.returncode != 0 and r.stdout.startswith("--mesh refused") and "Image Loading" not in r.stdout, (bad, r.stdout)
    for good in ("1", "0", "inf", "1.5,2", "0.25,16", "1e-3,1"):
        for extra in ([], ["--calib", "100,0.16,40,20,0"]):  # (it does not need --calib)
            r = subprocess.run([base[0], "--mesh", good] + base[1:] + extra, capture_output=True, text=True, timeout=120)
            assert r.returncode != 0 and "Image Loading" in r.stdout and "--mesh refused" not in r.stdout, good  # (well-formed: gets as far as the images)


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = (int(v) for v in f.readline().split())
        f.readline()
        return np.ascontiguousarray(np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1])


def read_mesh_ply(path):
    """-> (has normals, structured array of the vertices, int32 [m][3] faces); the whole file must be accounted for"""
    with open(path, "rb") as f:
        blob = f.read()
    head, body = blob.split(b"end_header\n", 1)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n")
    n = int(re.search(rb"element vertex (\d+)", head).group(1))
    m = int(re.search(rb"element face (\d+)\nproperty list uchar int vertex_indices\n$", head).group(1))
    with_n = b"property float nx" in head
    props = b"property float x\nproperty float y\nproperty float z\n" + (b"property float nx\nproperty float ny\nproperty float nz\n" if with_n else b"") + \
        b"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face"
    assert props in head
    vdt = np.dtype([("xyz", "<f4", 3)] + ([("n", "<f4", 3)] if with_n else []) + [("rgb", "u1", 3)])
    fdt = np.dtype([("k", "u1"), ("v", "<i4", 3)])
    assert len(body) == n * vdt.itemsize + m * fdt.itemsize
    faces = np.frombuffer(body, fdt, m, n * vdt.itemsize)
    assert (faces["k"] == 3).all()
    return with_n, np.frombuffer(body, vdt, n), np.ascontiguousarray(faces["v"]).reshape(-1, 3)


def check_mesh_ply(pref, left_bgr, calib, max_diff, step, normals, stdout):
    """<pref>-mesh.ply against the reference on <pref>.pfm (normals: the float32 [H][W][4] map whose rows the vertices must carry, or
    None for a file without normals); the line with the five counts in the run's output.  -> the reference's report"""
    disp = read_pfm(pref + ".pfm")
    v, vi, t, rep = M.mesh(disp, calib, max_diff, step, left_bgr)
    with_n, pv, faces = read_mesh_ply(pref + "-mesh.ply")
    assert with_n == (normals is not None) and len(pv) == len(v) and len(faces) == len(t)
    xyz = np.stack([v["x"], v["y"], v["z"]], -1)
    assert np.array_equal(np.ascontiguousarray(pv["xyz"]).view(np.uint32), np.ascontiguousarray(xyz).view(np.uint32))
    assert np.array_equal(pv["rgb"], np.stack([v["r"], v["g"], v["b"]], -1))
    assert np.array_equal(faces, t.astype(np.int32))
    if normals is not None:
        want = np.ascontiguousarray(normals.reshape(-1, 4)[vi][:, :3])
        assert np.array_equal(np.ascontiguousarray(pv["n"]).view(np.uint32), want.view(np.uint32))
    assert "Mesh, step %d: %u valid lattice pixels, %u vertices, %u triangles, %u cells of two, %u cells of one\n" % tuple([step] + M.report_words(rep)) in stdout
    return rep


def test_cli_mesh_under_sanitizers(tmp_path):
    """The flag's parsing and <out>-mesh.ply in the ASAN / UBSAN build on the stub C ABI, whose mesh is mesh_cell.h run serially: the
    file equals tests/mesh_ref.py on the run's .pfm, with and without --normals and --calib; every other file of the run is
    byte-identical to a run without the flag."""
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

    def run(pref, *extra):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "-3", "29", str(tmp_path / pref), *extra], env=SAN_ENV,
                           capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, r.stdout
        return r.stdout

    def same_files(a, b):
        names = sorted(f[len(a):] for f in os.listdir(tmp_path) if f.startswith(a + "-") or f.startswith(a + "."))
        assert len(names) >= 4 and "-mesh.ply" not in names
        for suffix in names:
            assert open(str(tmp_path / a) + suffix, "rb").read() == open(str(tmp_path / b) + suffix, "rb").read(), (a, b, suffix)
        assert sorted(f[len(b):] for f in os.listdir(tmp_path) if f.startswith(b + "-") or f.startswith(b + ".")) == sorted(names + ["-mesh.ply"])

    run("bare")
    run("plain", *calib_arg)
    run("nrm", *calib_arg, "--normals", "2")
    triangles = 0
    for pref, twin, arg, params, cal, extra in (("m1", "bare", "1", (1.0, 1), None, []), ("m2", "plain", "1.5,2", (1.5, 2), calib, calib_arg),
                                                ("m3", "bare", "inf,16", (np.inf, 16), None, []), ("m4", "plain", "0,3", (0.0, 3), calib, calib_arg),
                                                ("m5", "nrm", "2.5,1", (2.5, 1), calib, calib_arg + ["--normals", "2"])):
        out = run(pref, "--mesh", arg, *extra)
        same_files(twin, pref)
        normals = N.normals(read_pfm(str(tmp_path / pref) + ".pfm"), calib, 2, 1.0, 5)[0] if twin == "nrm" else None
        triangles += check_mesh_ply(str(tmp_path / pref), bgr, cal, params[0], params[1], normals, out)["triangles"]
    assert triangles > 100
    # --voxel does not touch the mesh: it comes from the map
    run("vox", *calib_arg, "--voxel", "0.05")
    run("voxm", *calib_arg, "--voxel", "0.05", "--mesh", "1.5,2")
    same_files("vox", "voxm")
    assert open(str(tmp_path / "voxm") + "-mesh.ply", "rb").read() == open(str(tmp_path / "m2") + "-mesh.ply", "rb").read()
