"""CPU tier of the TSDF volume: properties of tests/tsdf_ref.py (the definition the GPU tests hold the kernels to) on the cases of
tests/tsdf_cases.py; the header the kernels include (adcensus_amd/csrc/tsdf_voxel.h), compiled alone under g++ into a serial program
(tests/emul/emul_tsdf.cpp) and held to the reference bit for bit on every case, once more under ASAN + UBSAN as its own executable;
the accuracy of the definition against analytic surfaces; and the new surface of the C ABI, the Python mirror, the facade and the CLI
-- declared, exported, struct layouts, every refusal before a HIP call, malformed --tsdf, the sanitizer build of the CLI on the stub."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import tsdf_cases as TC
from tests import tsdf_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
F = np.float32
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def c_params(p):
    return A.TsdfParams(p["nx"], p["ny"], p["nz"], p["voxel"], p["origin"], p["trunc"], p["z_min"], p["z_max"], p["max_weight"], p["flags"])


def c_frame(fr):
    return A.TsdfFrame(fr["calib"], fr["R"], fr["t"], fr["kind"])


# ---------------------------------------------------------------------------------------------- properties of the reference alone
@pytest.mark.parametrize("name", TC.INTEGRATE_CASES)
def test_reference_properties(name):
    c, r = TC.case(name), TC.reference(name)
    p = c["params"]
    vol = c["init"] if c["init"] is not None else T.empty(p)
    for (fr, m, img), after, rep in zip(c["frames"], r["volumes"], r["reports"]):
        assert rep["in_frustum"] == rep["no_depth"] + rep["occluded"] + rep["updated"], name
        changed = after[0] != vol[0]
        assert changed.sum() <= rep["updated"], name                     # an untouched voxel keeps its bits (an update may leave them, too)
        if c["init"] is None:
            dw = T.word_w(after[0]) - T.word_w(vol[0])
            assert ((dw == 0) | (dw == 1)).all() and (dw == 1).sum() <= rep["updated"] and T.word_w(after[0]).max() <= p["max_weight"], name
            assert (np.abs(T.word_t(after[0])) <= T.Q).all(), name
        if after[1] is not None:
            cchanged = after[1] != vol[1]
            assert not (cchanged & ~changed & (T.word_w(vol[0]) < p["max_weight"])).any(), name   # colour only where the voxel was updated
            if img is None:
                assert not cchanged.any(), name
        vol = after
    if name == "wholly_outside":
        assert all(v == 0 for rep in r["reports"] for v in rep.values())
        assert np.array_equal(r["final"][0], c["init"][0]) and np.array_equal(r["final"][1], c["init"][1])
    else:
        assert r["reports"][0]["updated"] > 0 and r["xreport"]["points"] > 0, name


def test_reference_holes_and_special_values():
    """The spoiled maps: +inf, NaN and -inf pixels count as no_depth; negative disparities give the depth of their absolute value; an
    overflowing fb / s is free space (t = +32767); a voxel behind the camera or outside z_min..z_max keeps its bits."""
    r = TC.reference("tilted_holes_two_poses")
    assert all(rep["no_depth"] > 100 for rep in r["reports"])
    c = TC.case("tilted_holes_two_poses")
    fr, m, img = c["frames"][0]
    flipped = T.integrate(T.empty(c["params"]), c["params"], fr, np.abs(m), img)
    assert np.array_equal(flipped[0][0], r["volumes"][0][0]) and flipped[1] == r["reports"][0]
    c, r = TC.case("behind_and_overflow"), TC.reference("behind_and_overflow")
    t, w = T.word_t(r["final"][0]), T.word_w(r["final"][0])
    zw = T.centres(c["params"])[2] + F(-0.8)
    assert (w[zw <= 0] == 0).all() and (w[zw > 0].max() == 1) and ((t == T.Q) & (w == 1)).any()
    c, r = TC.case("depth_kind_cropped"), TC.reference("depth_kind_cropped")
    zw = T.centres(c["params"])[2]
    out = (zw < F(0.7)) | (zw > F(0.95))
    assert out.any() and (r["final"][0][out] == 0).all() and r["reports"][0]["no_depth"] > 0


def test_reference_plane_saturates_and_does_not_move():
    """A fronto-parallel plane integrated n times: w = min(n, max_weight) wherever it was seen, and t does not depend on n."""
    c, r = TC.case("plane5_saturates"), TC.reference("plane5_saturates")
    first = r["volumes"][0][0]
    seen = T.word_w(first) == 1
    assert seen.sum() == r["reports"][0]["updated"] > 20000
    for n, (tsdf, color) in enumerate(r["volumes"], 1):
        assert (T.word_w(tsdf)[seen] == min(n, 3)).all() and (T.word_w(tsdf)[~seen] == 0).all()
        assert np.array_equal(T.word_t(tsdf), T.word_t(first))
        assert ((color >> np.uint32(24))[color != 0] == min(n, 3)).all()
    assert r["xreport"]["points"] == len(r["points"]) > 2000 and (r["points"]["pad"] == 3).all()


def test_reference_extraction_of_a_hand_made_volume():
    """t = 0, +-32767, a stored -32768, weights below min_weight, crossings on the last voxel of each axis: the points and their order by hand."""
    c, r = TC.case("uploaded_edges"), TC.reference("uploaded_edges")
    p, (tsdf, color) = c["params"], c["init"]
    t, w = T.word_t(tsdf), T.word_w(tsdf)
    assert t.min() == -T.Q and (tsdf & 0xFFFF == 0x8000).any()
    want = []
    for k in range(4):
        for j in range(4):
            for i in range(8):
                for axis, (di, dj, dk) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
                    i2, j2, k2 = i + di, j + dj, k + dk
                    if i2 >= 8 or j2 >= 4 or k2 >= 4 or w[k, j, i] < 3 or w[k2, j2, i2] < 3 or (t[k, j, i] < 0) == (t[k2, j2, i2] < 0):
                        continue
                    s = F(t[k, j, i]) / (F(t[k, j, i]) - F(t[k2, j2, i2]))
                    pos = [F(1.0) + (F(i) + F(0.5)) * F(0.5), F(2.0) + (F(j) + F(0.5)) * F(0.5), F(3.0) + (F(k) + F(0.5)) * F(0.5)]
                    pos[axis] = pos[axis] + s * F(0.5)
                    col = int(color[k, j, i] if s <= F(0.5) else color[k2, j2, i2])
                    want.append((pos[0], pos[1], pos[2], col & 255, (col >> 8) & 255, (col >> 16) & 255, min(w[k, j, i], w[k2, j2, i2], 255)))
    want = np.array(want, T.POINT_DTYPE)
    assert r["points"].tobytes() == want.tobytes() and r["xreport"] == dict(voxels_seen=int((w >= 3).sum()), points=len(want))
    pts = r["points"]
    assert (pts["x"] == F(1.0) + F(6.5) * F(0.5) + F(0.5) * F(0.5)).sum() >= 8          # last voxel of x: s = 0.5 exactly
    assert (pts["y"] > F(2.0) + F(2.5) * F(0.5)).any() and (pts["z"] > F(3.0) + F(2.5) * F(0.5)).any()  # ... of y and of z
    assert 255 in pts["pad"] and 5 in pts["pad"]
    # t = 0 is non-negative: voxel (1, 1, 1) crosses towards its -5 neighbour with s = 0: the point is its centre
    centre = (F(1.0) + F(1.5) * F(0.5), F(2.0) + F(1.5) * F(0.5), F(3.0) + F(1.5) * F(0.5))
    assert ((pts["x"] == centre[0]) & (pts["y"] == centre[1]) & (pts["z"] == centre[2])).sum() == 1
    # the count does not depend on a capacity: a smaller buffer receives the first records of the full list, the report stays
    for cap in (0, 1, len(want) - 1, len(want), len(want) + 5):
        got, rep = T.extract(c["init"], p, 3, cap)
        assert got.tobytes() == want[:cap].tobytes() and rep == r["xreport"], cap
    assert T.extract(c["init"], p, 1)[1]["points"] > len(want)   # (weights below 3 join in)


# ---------------------------------------------------------------------------------------------- the shared header, serially
def _build_emul(tmp, sanitize):
    exe = os.path.join(tmp, "emul_tsdf_san" if sanitize else "emul_tsdf")
    cmd = ["g++", "-std=c++17", "-O1" if sanitize else "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "emul", "emul_tsdf.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emul_tsdf(tmp_path_factory):
    return _build_emul(str(tmp_path_factory.mktemp("emul_tsdf")), False)


def write_emul_case(c, ind):
    W, H = c["size"]
    os.makedirs(ind, exist_ok=True)
    frames = c["frames"]
    with open(os.path.join(ind, "case.bin"), "wb") as f:
        f.write(bytes(c_params(c["params"])))
        f.write(struct.pack("<5i", W, H, len(frames), c["min_weight"], int(c["init"] is not None)))
        for fr, _, _ in frames:
            f.write(bytes(c_frame(fr)))
        f.write(struct.pack("<%di" % len(frames), *[int(img is not None) for _, _, img in frames]))
    np.stack([m for _, m, _ in frames] if frames else [np.zeros((0, H, W), F)]).astype(F).tofile(os.path.join(ind, "maps.bin"))
    np.stack([img if img is not None else np.zeros((H, W, 3), np.uint8) for _, _, img in frames] if frames else [np.zeros((0, H, W, 3), np.uint8)]).tofile(os.path.join(ind, "img.bin"))
    if c["init"] is not None:
        c["init"][0].tofile(os.path.join(ind, "init_tsdf.bin"))
        if c["init"][1] is not None:
            c["init"][1].tofile(os.path.join(ind, "init_color.bin"))


def _run_emul(exe, name, tmp):
    c, r = TC.case(name), TC.reference(name)
    ind, outd = os.path.join(tmp, "in_" + name), os.path.join(tmp, "out_" + name)
    write_emul_case(c, ind)
    os.makedirs(outd, exist_ok=True)
    run = subprocess.run([exe, ind, outd], env=SAN_ENV, capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr and "LeakSanitizer" not in run.stderr, run.stderr[-3000:]
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert open(os.path.join(outd, "tsdf.bin"), "rb").read() == r["final"][0].tobytes(), name
    if r["final"][1] is not None:
        assert open(os.path.join(outd, "color.bin"), "rb").read() == r["final"][1].tobytes(), name
    assert np.fromfile(os.path.join(outd, "reports.bin"), np.uint32).tolist() == [v for rep in r["reports"] for v in T.report_words(rep) + [0, 0, 0, 0]], name
    assert open(os.path.join(outd, "points.bin"), "rb").read() == r["points"].tobytes(), name
    assert np.fromfile(os.path.join(outd, "xreport.bin"), np.uint32).tolist() == T.report_words(r["xreport"], T.EXTRACT_FIELDS) + [0] * 6, name
    return ind


@pytest.mark.parametrize("name", TC.CASE_NAMES)
def test_shared_header_equals_the_reference(emul_tsdf, name, tmp_path):
    _run_emul(emul_tsdf, name, str(tmp_path))


def test_shared_header_under_sanitizers(tmp_path):
    """The same program built once with ASAN + UBSAN and run as its own executable: a read outside the map, the image or the volume,
    an overflowing integer and a leak are reports, and a report is a failure."""
    exe = _build_emul(str(tmp_path), True)
    for name in TC.CASE_NAMES:
        if name != "big_scan":
            ind = _run_emul(exe, name, str(tmp_path))
    assert subprocess.run([exe], env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe, str(tmp_path / "absent"), str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2
    blob = bytearray(open(os.path.join(ind, "case.bin"), "rb").read())
    blob[0:4] = struct.pack("<i", 6)  # nx no multiple of 4
    open(os.path.join(ind, "case.bin"), "wb").write(bytes(blob))
    assert subprocess.run([exe, ind, str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------- accuracy of the definition
def test_fronto_parallel_plane_within_the_derived_bound():
    """The plane of `plane5_saturates` lies at D = RN(fb / d), identity pose, so Zc = zw exactly and only z carries an error.
    In units of u = trunc / 32767 the stored t of a voxel differs from its true sdf / u by at most e = 0.5 + 2^-7: half a unit of
    quantisation, plus four binary32 roundings (the difference, the two products, the sum with 0.5) of at most 2^-24 relative each on
    values below 2^15.  One frame leaves t = q, further frames of the same plane leave it there.  For a crossing a -> b with A, B the
    true distances in units and V = A - B = voxel / u: s * V - A = (V * ea - A * (ea - eb)) / (V + ea - eb) with |ea|, |eb| <= e and
    |A| <= V + e, so |z - D| <= e * u * (3 V + 2) / (V - 2 e); the roundings of s, s * voxel, the centre and the sum, and those of the
    two centres that make V, add at most 16 * 2^-24 * |z|."""
    c, r = TC.case("plane5_saturates"), TC.reference("plane5_saturates")
    p = c["params"]
    D = float(T.RR.source_z(c["frames"][0][1], T.FROM_DISPARITY, c["frames"][0][0]["calib"])[0][0, 0])
    u = p["trunc"] / T.Q
    V, e = p["voxel"] / u, 0.5 + 2.0 ** -7
    bound = e * u * (3 * V + 2) / (V - 2 * e) + 16 * 2.0 ** -24 * float(np.abs(r["points"]["z"]).max())
    err = np.abs(r["points"]["z"].astype(np.float64) - D)
    print("plane: largest |z - D| = %.3e, bound %.3e (%.2e voxel)" % (err.max(), bound, bound / p["voxel"]))
    assert bound < 1e-3 * p["voxel"] and err.max() <= bound


def accuracy_cases():
    """name -> (params, frames [(frame, depth map)], distance (points float64 [n][3]) -> float64 [n] in voxels)"""
    p = T.params(72, 40, 24, 0.02, TC.ORIGIN_72, 0.06)
    n, d = np.array([0.25, -0.15, 1.0]), 0.86
    sc, sr = np.array([0.0, 0.0, 0.9]), 0.17
    poses = [(T.IDENTITY, (0.0, 0.0, 0.0)), TC.POSE_A, TC.POSE_B]
    plane, sphere = TC.plane_surface(n, d), TC.sphere_surface(sc, sr)

    def frames(surface, which):
        return [(T.frame(TC.CALIB_80, R, t, kind=T.FROM_DEPTH), TC.raycast_depth(80, 60, TC.CALIB_80, R, t, surface)) for R, t in which]

    def plane_distance(x):
        return np.abs(x @ n - d) / np.linalg.norm(n) / p["voxel"]

    def sphere_distance(x):
        return np.abs(np.linalg.norm(x - sc, axis=1) - sr) / p["voxel"]

    return dict(tilted_one=(p, frames(plane, poses[:1]), plane_distance), tilted_poses=(p, frames(plane, poses), plane_distance),
                sphere_one=(p, frames(sphere, poses[:1]), sphere_distance), sphere_poses=(p, frames(sphere, poses), sphere_distance))


def measure_accuracy(name):
    p, frames, distance = accuracy_cases()[name]
    vol = T.empty(p)
    for fr, m in frames:
        vol, _ = T.integrate(vol, p, fr, m)
    pts, _ = T.extract(vol, p, 1)
    d = distance(np.stack([pts["x"], pts["y"], pts["z"]], -1).astype(np.float64))
    return len(pts), float(d.max()), float(np.median(d))


# largest distance to the analytic surface in voxels, as recorded in profiles/tsdf_accuracy.md
RECORDED_LARGEST = dict(tilted_one=0.1510, tilted_poses=0.1602, sphere_one=0.2919, sphere_poses=0.3681)


@pytest.mark.parametrize("name", sorted(RECORDED_LARGEST))
def test_accuracy_against_analytic_surfaces(name):
    """A tilted plane and a sphere, one frame and three poses: the distance of the extracted points to the analytic surface.  The
    bound is 1.25 times the value recorded in profiles/tsdf_accuracy.md: it only stops a later edit of the definition from degrading it
    unnoticed."""
    n, largest, median = measure_accuracy(name)
    print("%s: %d points, largest %.4f voxel, median %.4f voxel" % (name, n, largest, median))
    assert n > 300 and largest <= 1.25 * RECORDED_LARGEST[name]
    text = open(os.path.join(ROOT, "profiles", "tsdf_accuracy.md")).read()
    assert re.search(r"\| %s \| %d \| %.4f \| %.4f \|" % (name, n, RECORDED_LARGEST[name], median), text), name


# ---------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name in A.TSDF_ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    assert re.search(r"#define\s+ADC_TSDF_COLOR\s+1u", text) and A.TSDF_COLOR == T.COLOR == 1
    for phrase in ("t' = (t*w + q + 32767*m + m/2) / m - 32767", "can yield two coincident points", "counts only", "refused, not ignored",
                   "not a product of adc_products or the farm", "No float reaches an"):
        assert phrase in text, phrase
    for lib in (A.LIB_PATH, os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(A.TSDF_ENTRY_POINTS) <= names, lib
    # the struct layouts, asked of a C compiler; the existing structs keep theirs
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(adc_tsdf_params), offsetof(adc_tsdf_params, voxel),\n'
                   ' offsetof(adc_tsdf_params, origin), offsetof(adc_tsdf_params, z_max), offsetof(adc_tsdf_params, flags), offsetof(adc_tsdf_params, reserved_),\n'
                   ' sizeof(adc_tsdf_frame), offsetof(adc_tsdf_frame, calib), offsetof(adc_tsdf_frame, R), offsetof(adc_tsdf_frame, t), offsetof(adc_tsdf_frame, flags),\n'
                   ' sizeof(adc_tsdf_report), sizeof(adc_tsdf_extract_params), sizeof(adc_tsdf_extract_report), sizeof(adc_point), sizeof(adc_mesh_params)); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    P, Fr = A.TsdfParams, A.TsdfFrame
    assert got == [C.sizeof(P), P.voxel.offset, P.origin.offset, P.z_max.offset, P.flags.offset, P.reserved_.offset, C.sizeof(Fr), Fr.calib.offset, Fr.R.offset,
                   Fr.t.offset, Fr.flags.offset, C.sizeof(A.TsdfReport), C.sizeof(A.TsdfExtractParams), C.sizeof(A.TsdfExtractReport), A.POINT_DTYPE.itemsize,
                   C.sizeof(A.MeshParams)]
    assert got[0] == 64 and got[6] == 96 and got[11:] == [32, 32, 32, 16, 32]
    assert T.POINT_DTYPE.itemsize == 16 and [T.POINT_DTYPE.fields[k][1] for k in T.POINT_DTYPE.names] == [A.POINT_DTYPE.fields[k][1] for k in A.POINT_DTYPE.names]
    assert [f[0] for f in A.TsdfReport._fields_] == list(T.REPORT_FIELDS) + ["reserved_"]
    assert [f[0] for f in A.TsdfExtractReport._fields_] == list(T.EXTRACT_FIELDS) + ["reserved_"]
    fr = A.TsdfFrame()
    assert (fr.kind, list(fr.R), list(fr.t), fr.flags) == (0, [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0], 0) and A.TsdfExtractParams().min_weight == 1


GOOD_PARAMS = dict(nx=8, ny=8, nz=8, voxel=0.05, origin=(0.0, 0.0, 0.5), trunc=0.1)


def test_every_refusal_comes_before_a_hip_call():
    """No device here: each of these returns 1 with a message without touching HIP.  A block of ones stands in for a handle that has a
    volume (with colour) and a Match pending (every flag nonzero): the last check of all, so everything in front of it is reached on
    it; a zeroed block for an idle handle without a volume that has completed nothing."""
    L = A.lib()
    vp = C.c_void_p
    idle = C.cast(C.create_string_buffer(1 << 20), vp)
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), vp)
    dev = vp(4096)
    calib = (100.0, 0.16, 10.0, 5.0, 0.0)
    good = A.TsdfFrame(calib)
    rep, xrep = A.TsdfReport(), A.TsdfExtractReport()
    inf, nan = float("inf"), float("nan")

    def refused(rc, *words):
        msg = A.last_error()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    # adc_tsdf_create
    refused(L.adc_tsdf_create(None, C.byref(A.TsdfParams(**GOOD_PARAMS))), "adc_tsdf_create", "null handle")
    refused(L.adc_tsdf_create(busy, None), "adc_tsdf_create", "null params")
    for kw, why in ([(dict(nx=v), "[4, 2048]") for v in (0, -4, 2052, 2 ** 31 - 1)] + [(dict(ny=v), "[4, 2048]") for v in (3, 2049)] +
                    [(dict(nz=v), "[4, 2048]") for v in (3, 2049, -1)] + [(dict(nx=v), "multiple of 4") for v in (5, 6, 7, 2047)] +
                    [(dict(nx=2048, ny=1024, nz=516), "2^30")] + [(dict(voxel=v), "voxel") for v in (0.0, -1.0, inf, nan)] +
                    [(dict(origin=o), "origin") for o in ((nan, 0, 0), (0, inf, 0), (0, 0, -inf))] + [(dict(trunc=v), "trunc") for v in (0.0, -0.1, inf, nan)] +
                    [(dict(z_min=a, z_max=b), "z_min") for a, b in ((-0.1, 1.0), (nan, 1.0), (0.0, nan), (2.0, 1.0), (inf, 1.0))] +
                    [(dict(max_weight=v), "max_weight") for v in (0, 65536, 2 ** 32 - 1)] + [(dict(flags=v), "unknown flag") for v in (2, 3, 0x80000000)]):
        refused(L.adc_tsdf_create(busy, C.byref(A.TsdfParams(**dict(GOOD_PARAMS, **kw)))), "adc_tsdf_create", why)
    for k in range(4):
        p = A.TsdfParams(**GOOD_PARAMS)
        p.reserved_[k] = 1
        refused(L.adc_tsdf_create(busy, C.byref(p)), "adc_tsdf_create", "reserved")
    for kw in (dict(), dict(nx=2048, ny=1024, nz=512), dict(z_min=0.0, z_max=0.0), dict(z_max=inf), dict(max_weight=65535, flags=1), dict(nx=4, ny=4, nz=4)):
        refused(L.adc_tsdf_create(busy, C.byref(A.TsdfParams(**dict(GOOD_PARAMS, **kw)))), "adc_tsdf_create", "Match is pending")
    # reset / destroy / volume / download / upload
    for name, call in (("adc_tsdf_reset", L.adc_tsdf_reset), ("adc_tsdf_destroy", L.adc_tsdf_destroy)):
        refused(call(None), name, "null handle")
        refused(call(busy), name, "Match is pending")
    refused(L.adc_tsdf_reset(idle), "adc_tsdf_reset", "no volume")
    assert L.adc_tsdf_destroy(idle) == 0   # (nothing to give back)
    t, c, p = vp(), vp(), A.TsdfParams()
    refused(L.adc_tsdf_get_volume_device(None, C.byref(t), C.byref(c), C.byref(p)), "adc_tsdf_get_volume_device", "null handle")
    refused(L.adc_tsdf_get_volume_device(idle, C.byref(t), C.byref(c), C.byref(p)), "adc_tsdf_get_volume_device", "no volume")
    for name, call in (("adc_tsdf_download", L.adc_tsdf_download), ("adc_tsdf_upload", L.adc_tsdf_upload)):
        refused(call(None, dev, None), name, "null handle")
        refused(call(busy, None, dev), name, "null tsdf")
        refused(call(idle, dev, None), name, "no volume")
        refused(call(busy, dev, dev), name, "Match is pending")
    # integrate
    for who, call in (("adc_tsdf_integrate_device", lambda h, m, fr, img=None: L.adc_tsdf_integrate_device(h, m, img, None if fr is None else C.byref(fr))),
                      ("adc_tsdf_integrate", lambda h, m, fr, img=None: L.adc_tsdf_integrate(h, m, img, None if fr is None else C.byref(fr), C.byref(rep)))):
        refused(call(None, dev, good), who, "null handle")
        refused(call(busy, None, good), who, "null map")
        refused(call(busy, dev, None), who, "null frame")
        for kind in (-1, 2, 7):
            refused(call(busy, dev, A.TsdfFrame(calib, kind=kind)), who, "kind")
        for k in range(5):
            for v in (nan, inf):
                vals = list(calib)
                vals[k] = v
                refused(call(busy, dev, A.TsdfFrame(vals)), who, "non-finite")
        for f in (0.0, -100.0):
            refused(call(busy, dev, A.TsdfFrame((f,) + calib[1:])), who, "focal_px must be positive")
        for k in range(9):
            R = list(T.IDENTITY)
            R[k] = nan if k % 2 else inf
            refused(call(busy, dev, A.TsdfFrame(calib, R)), who, "R has a non-finite")
        for k in range(3):
            tt = [0.0, 0.0, 0.0]
            tt[k] = -inf if k else nan
            refused(call(busy, dev, A.TsdfFrame(calib, None, tt)), who, "t has a non-finite")
        refused(call(busy, dev, A.TsdfFrame(calib, flags=1)), who, "unknown flag")
        for k in range(5):
            fr = A.TsdfFrame(calib)
            fr.reserved_[k] = 1
            refused(call(busy, dev, fr), who, "reserved")
        refused(call(idle, dev, good), who, "no volume")
        for fr in (good, A.TsdfFrame(calib, TC.POSE_A[0], TC.POSE_A[1], 1)):
            refused(call(busy, dev, fr), who, "Match is pending")
            refused(call(busy, dev, fr, dev), who, "Match is pending")
    for bad in (4097, 4098, 4099):
        refused(L.adc_tsdf_integrate_device(busy, vp(bad), None, C.byref(good)), "adc_tsdf_integrate_device", "4-byte aligned")
        refused(L.adc_tsdf_integrate_device(busy, dev, vp(bad), C.byref(good)), "Match is pending")  # (bytes: the image may lie anywhere)
    # extract
    for who, call in (("adc_tsdf_extract_device", lambda h, p=None, pts=dev, cap=10: L.adc_tsdf_extract_device(h, None if p is None else C.byref(p), pts, cap, None)),
                      ("adc_tsdf_extract", lambda h, p=None, pts=dev, cap=10: L.adc_tsdf_extract(h, None if p is None else C.byref(p), pts, cap, C.byref(xrep)))):
        refused(call(None), who, "null handle")
        for mw in (0, 65536, 2 ** 32 - 1):
            refused(call(busy, A.TsdfExtractParams(mw)), who, "min_weight")
        for k in range(7):
            p = A.TsdfExtractParams()
            p.reserved_[k] = 1
            refused(call(busy, p), who, "reserved")
        refused(call(busy, None, None, 5), who, "null points with a capacity")
        refused(call(idle), who, "no volume")
        for p, pts, cap in ((None, dev, 10), (A.TsdfExtractParams(65535), dev, 0), (A.TsdfExtractParams(1), None, 0)):
            refused(call(busy, p, pts, cap), who, "Match is pending")
    for bad in (4096 + 4, 4096 + 8, 4096 + 1):
        refused(L.adc_tsdf_extract_device(busy, None, vp(bad), 10, None), "adc_tsdf_extract_device", "16-byte aligned")
    for bad in (4097, 4098, 4099):
        refused(L.adc_tsdf_extract_device(busy, None, dev, 10, vp(bad)), "adc_tsdf_extract_device", "4-byte aligned")
    # reports
    refused(L.adc_get_tsdf_report(None, C.byref(rep), None), "null")
    refused(L.adc_get_tsdf_report(idle, None, None), "null")
    refused(L.adc_get_tsdf_report(idle, C.byref(rep), None), "no integrate call")
    refused(L.adc_get_tsdf_report(idle, None, C.byref(xrep)), "no extract call")
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    st.width, st.height = 8, 4
    assert st.tsdf_create(A.TsdfParams(**GOOD_PARAMS)) is False and st.tsdf_reset() is False and st.tsdf_destroy() is False
    assert st.tsdf_integrate_device(4096, good) is False and st.tsdf_extract_device(4096, 4) is False and st.tsdf_report() == (None, None)
    for call in (lambda: st.tsdf_integrate(np.zeros((4, 8), F), good), st.tsdf_extract, st.tsdf_volume_device, st.tsdf_download):
        with pytest.raises(RuntimeError):
            call()


CALLER = r'''
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
int main() {
    ADCensusStereo s; ADCensusOption o;
    uint8 img[96] = {0};
    float32 d[32] = {0};
    adc_tsdf_params p = {8, 8, 8, 0.05f, {0.f, 0.f, 0.5f}, 0.1f, 0.f, 10.f, 64u, ADC_TSDF_COLOR, {0u, 0u, 0u, 0u}};
    adc_tsdf_frame f = {ADC_REG_FROM_DISPARITY, {100.f, 0.16f, 4.f, 2.f, 0.f}, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}, 0u, {0u, 0u, 0u, 0u, 0u}};
    adc_tsdf_extract_params x = {1u, {0u, 0u, 0u, 0u, 0u, 0u, 0u}};
    adc_tsdf_report rep;
    adc_tsdf_extract_report xrep;
    adc_point pts[8];
    // before Initialize there is no matcher underneath: everything is refused
    bool ok = !s.TsdfCreate(&p) && !s.TsdfReset() && !s.TsdfIntegrate(d, img, &f, &rep) && !s.TsdfExtract(&x, pts, 8, &xrep) && !s.TsdfExtract(nullptr, nullptr, 0, nullptr) &&
              !s.GetTsdfReport(&rep, &xrep);
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
    for member in ("TsdfCreate(adc_tsdf_params const*)", "TsdfReset()", "TsdfIntegrate(float const*, unsigned char const*, adc_tsdf_frame const*, adc_tsdf_report*)",
                   "TsdfExtract(adc_tsdf_extract_params const*, adc_point*, unsigned long, adc_tsdf_extract_report*)",
                   "GetTsdfReport(adc_tsdf_report*, adc_tsdf_extract_report*)"):
        assert "ADCensusStereo::" + member in out, member
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def test_cli_rejects_malformed_tsdf_flags(tmp_path):
    """Checked while the arguments are parsed: the images named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    base = [cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "0", "64", str(tmp_path / "out")]
    calib = ["--calib", "100,0.16,40,20,0"]
    good = "8,8,8,0.1,0,0,1"
    for bad in ("", "8,8,8", "8,8,8,0.1,0,0", "6,8,8,0.1,0,0,1", "8,3,8,0.1,0,0,1", "8,8,2052,0.1,0,0,1", "2048,2048,512,0.1,0,0,1", "8,8,8,0,0,0,1", "8,8,8,-1,0,0,1",
                "8,8,8,nan,0,0,1", "8,8,8,0.1,inf,0,1", "8,8,8,0.1,0,0,1,0", "8,8,8,0.1,0,0,1,-2", "8,8,8,0.1,0,0,1,0.3,0", "8,8,8,0.1,0,0,1,0.3,65536", "8,8,8,0.1,0,0,1,0.3,2,9",
                "8,8,8,0.1,0,0,1x", "8,8,8,0.1,0,0,1,0.3x", "8,8,8,0.1,0,0,1,0.3,2x", "8.5,8,8,0.1,0,0,1", "one"):
        r = subprocess.run(base + calib + ["--tsdf", bad], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and r.stdout.startswith("--tsdf refused") and "Image Loading" not in r.stdout, (bad, r.stdout)
    r = subprocess.run(base + ["--tsdf", good], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.stdout.startswith("--tsdf refused: it needs --calib")
    (tmp_path / "short.txt").write_text("1 0 0 0 1 0 0 0 1 0 0\n")
    (tmp_path / "long.txt").write_text("1 0 0 0 1 0 0 0 1 0 0 0 7\n")
    (tmp_path / "nan.txt").write_text("1 0 0 0 nan 0 0 0 1 0 0 0\n")
    (tmp_path / "good.txt").write_text("1 0 0\n0 1 0\n0 0 1\n0.5 0 -1e-3\n")
    for name in ("short.txt", "long.txt", "nan.txt", "absent.txt"):
        r = subprocess.run(base + calib + ["--tsdf", good, "--pose", str(tmp_path / name)], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and r.stdout.startswith("--pose refused") and "Image Loading" not in r.stdout, (name, r.stdout)
    r = subprocess.run(base + calib + ["--pose", str(tmp_path / "good.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.stdout.startswith("--pose refused: it needs --tsdf")
    for spec in (good, good + ",0.3", good + ",0.3,5", "2048,1024,512,1e-3,-1,-1,0.5"):
        for extra in ([], ["--pose", str(tmp_path / "good.txt")]):
            r = subprocess.run([base[0], "--tsdf", spec] + base[1:] + calib + extra, capture_output=True, text=True, timeout=120)
            assert r.returncode != 0 and "Image Loading" in r.stdout and "refused" not in r.stdout, (spec, r.stdout)  # (well-formed: gets as far as the images)


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = (int(v) for v in f.readline().split())
        f.readline()
        return np.ascontiguousarray(np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1])


def read_tsdf_ply(path):
    """-> the points as tests/tsdf_ref.py records (pad 0: the file does not carry the weight); the whole file must be accounted for"""
    with open(path, "rb") as f:
        blob = f.read()
    head, body = blob.split(b"end_header\n", 1)
    m = re.fullmatch(rb"ply\nformat binary_little_endian 1.0\nelement vertex (\d+)\nproperty float x\nproperty float y\nproperty float z\n"
                     rb"property uchar red\nproperty uchar green\nproperty uchar blue\n", head)
    assert m, head
    n = int(m.group(1))
    rec = np.frombuffer(body, np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    assert len(body) == 15 * n and len(rec) == n
    out = np.zeros(n, T.POINT_DTYPE)
    out["x"], out["y"], out["z"] = rec["xyz"][:, 0], rec["xyz"][:, 1], rec["xyz"][:, 2]
    out["r"], out["g"], out["b"] = rec["rgb"][:, 0], rec["rgb"][:, 1], rec["rgb"][:, 2]
    return out


def test_cli_tsdf_under_sanitizers(tmp_path):
    """The flags' parsing and <out>-tsdf.ply in the ASAN / UBSAN build on the stub C ABI, whose volume is tsdf_voxel.h run serially: a
    well-formed ply that equals tests/tsdf_ref.py on the run's .pfm, with and without --pose, TRUNC and MINW; every other file of the run
    is byte-identical to a run without the flag."""
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

    run("plain", *calib_arg)
    names = sorted(f[len("plain"):] for f in os.listdir(tmp_path) if f.startswith("plain-") or f.startswith("plain."))
    assert len(names) >= 4 and "-tsdf.ply" not in names
    total = 0
    for pref, spec, trunc, mw, pose in (("t1", "32,24,32,0.04,-0.64,-0.48,0.35", 0.04 * 3, 1, False), ("t2", "32,24,32,0.04,-0.64,-0.48,0.35,0.08", 0.08, 1, True),
                                        ("t3", "36,20,28,0.05,-0.9,-0.5,0.3,0.2,1", 0.2, 1, True), ("t4", "32,24,32,0.04,-0.64,-0.48,0.35,0.08,2", 0.08, 2, False)):
        out = run(pref, "--tsdf", spec, *calib_arg, *(["--pose", str(tmp_path / "pose.txt")] if pose else []))
        for suffix in names:
            assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / pref) + suffix, "rb").read(), (pref, suffix)
        v = spec.split(",")
        p = T.params(int(v[0]), int(v[1]), int(v[2]), float(v[3]), [float(x) for x in v[4:7]], float(F(3.0) * F(v[3])) if len(v) == 7 else trunc, flags=T.COLOR)
        fr = T.frame(calib, R, t) if pose else T.frame(calib)
        vol, rep = T.integrate(T.empty(p), p, fr, read_pfm(str(tmp_path / pref) + ".pfm"), bgr)
        pts, xrep = T.extract(vol, p, mw)
        pts = pts.copy()
        pts["pad"] = 0
        assert read_tsdf_ply(str(tmp_path / pref) + "-tsdf.ply").tobytes() == pts.tobytes(), pref
        assert "TSDF: %u voxels in the frustum, %u without depth, %u occluded, %u updated; %u voxels seen, %u surface points\n" % tuple(
            T.report_words(rep) + T.report_words(xrep, T.EXTRACT_FIELDS)) in out, out
        assert rep["updated"] > 1000 and (len(pts) > 0) == (mw == 1), (pref, rep, xrep)
        total += len(pts)
    assert total > 300
