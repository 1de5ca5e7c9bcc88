"""CPU tier of frame-to-model tracking: the header the kernels include (adcensus_amd/csrc/tsdf_track.h), compiled alone under g++ into a
serial program (tests/emul/emul_tsdf_track.cpp) and held to tests/tsdf_track_ref.py bit for bit on every case of
tests/tsdf_track_cases.py -- the sums of every reduce pass, the counts, every iteration record and the final pose as raw words --,
once more under ASAN + UBSAN as its own executable; properties of the cases (each reaches the count or status it is there for); the
accuracy checks of tests/tsdf_track_checks.py on the reference and the serial program; and the new surface of the C ABI, the Python
mirror and the facade -- declared, exported, laid out alike, every refusal before a HIP call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import tsdf_track_cases as KC
from tests import tsdf_track_checks as K
from tests import tsdf_track_ref as TR
from tests.test_tsdf_api import SAN_ENV, c_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
F = np.float32


def c_track_params(p):
    return A.TrackParams(*[p[k] for k in TR.PARAM_FIELDS])


def c_model(m):
    """the model view as the adc_tsdf_raycast_params the maps were cast with: the tracker reads the view's size, intrinsics and pose"""
    return A.TsdfRaycastParams(m["width"], m["height"], m["focal_px"], m["cx"], m["cy"], m["R"], m["t"], 0.05, 10.0, 0.025, 0.05, 1, 4096)


# ---------------------------------------------------------------------------------------------- the cases and the reference alone
@pytest.mark.parametrize("name", KC.CASE_NAMES)
def test_cases_reach_their_counts_and_statuses(name):
    c, r = KC.case(name), KC.reference(name)
    cnt, p = r["counts"], c["params"]
    s = p["stride"]
    assert cnt["pixels"] == -(-c["W"] // s) * -(-c["H"] // s) == sum(cnt[k] for k in TR.COUNT_FIELDS[1:])
    assert 1 <= r["solves"] <= p["iterations"] and len(r["iteration"]) == r["solves"] == len(r["sums"])
    for what in KC.REACHES[name]:
        if what in TR.STATUS_NAMES:
            assert TR.STATUS_NAMES[r["status"]] == what, (name, TR.STATUS_NAMES[r["status"]])
        else:
            assert cnt[what] > 0, (name, what, cnt)
    guess = np.array(list(c["frame"]["R"]) + list(c["frame"]["t"]), F)
    final = np.array(list(r["R"]) + list(r["t"]), F)
    if name in ("lost", "degenerate", "diverged"):  # ended in the first solve: the pose is the guess, bit for bit
        assert r["solves"] == 1 and final.tobytes() == guess.tobytes()
    if name == "lost":
        assert cnt["used"] == 0 < p["min_pixels"] and r["iteration"][0] == [0, 0.0, 0.0, 0.0]
    if name == "degenerate":  # the columns of omega_z, v_x, v_y are exactly zero
        H = np.array(r["H"]).reshape(6, 6)
        assert (H[2] == 0).all() and (H[3] == 0).all() and (H[4] == 0).all() and H[0, 0] > 0 and H[5, 5] > 0
    if name == "max_iterations":
        assert r["solves"] == p["iterations"] == 2
    if name == "bad_values":  # the planted values and the pixels behind z_far
        assert cnt["no_depth"] >= 6 + 12
    if "CONVERGED" in KC.REACHES[name]:
        rec = r["iteration"][-1]
        assert rec[2] < p["eps_rot"] and rec[3] < p["eps_trans"] and final.tobytes() != guess.tobytes()
    Rm = np.array(r["R"], np.float64).reshape(3, 3)
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-6  # (a rotation to float accuracy after every update)


# ---------------------------------------------------------------------------------------------- the shared header, serially
def _build_emul(tmp, sanitize):
    exe = os.path.join(tmp, "emul_tsdf_track_san" if sanitize else "emul_tsdf_track")
    cmd = ["g++", "-std=c++17", "-O1" if sanitize else "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "emul", "emul_tsdf_track.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emul_tsdf_track(tmp_path_factory):
    return _build_emul(str(tmp_path_factory.mktemp("emul_tsdf_track")), False)


def write_case(c, d, W=None, H=None):
    os.makedirs(d, exist_ok=True)
    head = np.array([c["W"] if W is None else W, c["H"] if H is None else H, 0 if c["fnormals"] is None else 1, 0], np.int32)
    with open(os.path.join(d, "case.bin"), "wb") as f:
        f.write(head.tobytes() + bytes(c_frame(c["frame"])) + bytes(c_model(c["model"])) + bytes(c_track_params(c["params"])))
    for name, key in (("map", "map"), ("fnormals", "fnormals"), ("mdepth", "mdepth"), ("mnormals", "mnormals")):
        if c[key] is not None:
            np.ascontiguousarray(c[key], F).tofile(os.path.join(d, name + ".bin"))


def run_emul(exe, c, d):
    """the serial program on a case in directory d -> (the bytes of its adc_track_result, its sums as a list of lists of ints)"""
    write_case(c, d)
    run = subprocess.run([exe, d, d], env=SAN_ENV, capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr and "LeakSanitizer" not in run.stderr, run.stderr[-3000:]
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    sums = np.fromfile(os.path.join(d, "sums.bin"), np.int64).reshape(-1, 28)
    return open(os.path.join(d, "result.bin"), "rb").read(), [[int(v) for v in row] for row in sums]


def serial_track(exe, tmp):
    """the serial program behind the interface of tsdf_track_ref.track (status, solves, R, t, counts, iteration)"""
    count = [0]

    def track(depth_map, fnormals, fr, mdl, mdepth, mnormals, p):
        count[0] += 1
        H, W = np.asarray(depth_map).shape
        c = dict(W=W, H=H, map=depth_map, fnormals=fnormals, frame=fr, model=mdl, mdepth=mdepth, mnormals=mnormals, params=p)
        raw, _ = run_emul(exe, c, os.path.join(tmp, "check%d" % count[0]))
        return result_dict(A.TrackResult.from_buffer_copy(raw))
    return track


def result_dict(res):
    """a TrackResult in the layout of tsdf_track_ref.track"""
    return dict(status=res.status, solves=res.solves, R=list(res.R), t=list(res.t), counts={k: getattr(res, k) for k in TR.COUNT_FIELDS}, H=list(res.H), b=list(res.b),
                iteration=[[it.used, it.rms, it.rot, it.trans] for it in list(res.iteration)[:res.solves]])


def _emul_case(exe, name, tmp):
    want = KC.reference(name)
    raw, sums = run_emul(exe, KC.case(name), os.path.join(tmp, name))
    assert sums == want["sums"], (name, "sums")
    if raw != TR.result_bytes(want):
        got = result_dict(A.TrackResult.from_buffer_copy(raw))
        for k in ("status", "solves", "counts", "iteration", "H", "b", "R", "t"):
            assert got[k] == want[k], (name, k, got[k], want[k])
    assert raw == TR.result_bytes(want), name
    return os.path.join(tmp, name)


@pytest.mark.parametrize("name", KC.CASE_NAMES)
def test_shared_header_equals_the_reference(emul_tsdf_track, name, tmp_path):
    _emul_case(emul_tsdf_track, name, str(tmp_path))


def test_shared_header_under_sanitizers(tmp_path):
    """The same program built once with ASAN + UBSAN and run as its own executable: a read outside a map, an overflowing integer, a
    float that does not fit its integer and a leak are reports, and a report is a failure.  Bad arguments, a bad parameter and more
    than 2^26 participating pixels (refused before any file of that size is looked for) end it with 2."""
    exe = _build_emul(str(tmp_path), True)
    for name in KC.CASE_NAMES:
        d = _emul_case(exe, name, str(tmp_path))
    assert subprocess.run([exe], env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe, str(tmp_path / "absent"), str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2
    c = KC.case("converged_64x48")
    write_case(c, d, W=16384, H=8192)  # 2^27 pixels at stride 1
    assert subprocess.run([exe, d, str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2
    write_case(dict(c, params=dict(c["params"], stride=0)), d)
    assert subprocess.run([exe, d, str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2
    write_case(c, d)
    assert subprocess.run([exe, d, d], env=SAN_ENV, capture_output=True).returncode == 0


# ---------------------------------------------------------------------------------------------- checks that do not rest on the code
@pytest.mark.parametrize("motion", K.MOTIONS)
@pytest.mark.parametrize("stride", (1, 2))
def test_analytic_scene_recovers_the_pose(emul_tsdf_track, tmp_path, motion, stride):
    """tests/tsdf_track_checks.py (a): analytic model maps, the frame rendered analytically from a known second pose.  The largest
    displacement of a visible scene point between the recovered and the true pose stays below four times what was measured on the numpy
    reference (profiles/tsdf_track_accuracy.md; K.MEASURED_Q, in units of q = max_dist / 65536) and below 1/100 of the initial one."""
    for track in (TR.track, serial_track(emul_tsdf_track, str(tmp_path))):
        m = K.check_analytic(track, motion, stride)
        print("analytic %s stride %d: %s" % (motion, stride, m))
        assert m["final_q"] <= 4.0 * K.MEASURED_Q[(motion, stride)] and m["final"] < m["initial"] / 100.0, m


def test_whole_chain_recovers_the_pose(emul_tsdf_track, tmp_path):
    """tests/tsdf_track_checks.py (b): the analytic depth integrated three times at pose A by the reference integrator, ray cast from A
    by the reference ray caster, the frame rendered analytically at pose B and tracked from the guess A: the displacement is at most
    one voxel edge and at most 1/10 of the initial one."""
    for track in (TR.track, serial_track(emul_tsdf_track, str(tmp_path))):
        m = K.check_chain(track)
        print("chain: %s" % m)
        assert m["final"] <= m["voxel"] and m["final"] <= m["initial"] / 10.0, m


# ---------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name in A.TRACK_ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    for phrase in ("every sum stays at or below\n * 2^62", "NOT measured optima", "the Cayley map", "No float reaches an address before that integer test",
                   "every refusal stands before the first HIP call", "Not a product of adc_products or the farm"):
        assert phrase in text, phrase
    shared = open(os.path.join(ROOT, "adcensus_amd", "csrc", "tsdf_track.h")).read()
    assert "2^26 * 2^36 = 2^62" in shared and "#include <hip" not in shared and "hip_runtime" not in shared  # (the derivation; no HIP header)
    for lib in (A.LIB_PATH, os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(A.TRACK_ENTRY_POINTS) <= names, lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d", sizeof(adc_track_params), offsetof(adc_track_params, min_pixels),\n'
                   'offsetof(adc_track_params, pivot_ratio), offsetof(adc_track_params, reserved_), sizeof(adc_track_iteration), sizeof(adc_track_result),\n'
                   'offsetof(adc_track_result, pixels), offsetof(adc_track_result, H), offsetof(adc_track_result, iteration), offsetof(adc_track_result, reserved_),\n'
                   'ADC_TRACK_CONVERGED, ADC_TRACK_MAX_ITERATIONS, ADC_TRACK_LOST, ADC_TRACK_DEGENERATE, ADC_TRACK_DIVERGED, ADC_TRACK_MAX_ITERATIONS_LIMIT); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    P, R = A.TrackParams, A.TrackResult
    assert got == [C.sizeof(P), P.min_pixels.offset, P.pivot_ratio.offset, P.reserved_.offset, C.sizeof(A.TrackIteration), C.sizeof(R), R.pixels.offset, R.H.offset,
                   R.iteration.offset, R.reserved_.offset, A.TRACK_CONVERGED, A.TRACK_MAX_ITERATIONS, A.TRACK_LOST, A.TRACK_DEGENERATE, A.TRACK_DIVERGED,
                   A.TRACK_MAX_ITERATIONS_LIMIT] == [64, 20, 44, 52, 16, 960, 56, 88, 424, 936, 0, 1, 2, 3, 4, 32]
    assert [f[0] for f in P._fields_][:12] == list(TR.PARAM_FIELDS) and [f[0] for f in R._fields_][4:12] == list(TR.COUNT_FIELDS)
    assert (TR.CONVERGED, TR.MAX_ITERATIONS, TR.LOST, TR.DEGENERATE, TR.DIVERGED) == (0, 1, 2, 3, 4)
    d = A.TrackParams()  # the defaults of the mirror are those of a NULL pointer (TRACK_DEFAULT) and of the reference
    assert bytes(d) == bytes(c_track_params(TR.DEFAULTS))
    m = re.search(r"TRACK_DEFAULT = \{([^;]*)\};", shared).group(1)
    vals = [v.strip(" {}uf") for v in m.split(",")]
    assert bytes(A.TrackParams(*[float(v) if "." in v else int(v) for v in vals[:12]])) == bytes(d) and all(int(v) == 0 for v in vals[12:])


def _frame():
    return A.TsdfFrame((100.0, 0.16, 40.0, 20.0, 0.0))


def _view():
    return A.TsdfRaycastParams(37, 23, 30.0, 18.0, 11.0, None, None, 0.05, 10.0, 0.025, 0.05, 1, 4096)


def test_every_refusal_comes_before_a_hip_call():
    """No device here: each of these returns 1 with a message without touching HIP.  A block of ones stands in for a handle that has a
    volume and a Match pending (every flag nonzero): the last check but one, so everything in front of it is reached on it; a zeroed
    block for an idle handle without a volume that has completed nothing, and of 0 x 0 pixels: the check behind it, the frame's size,
    refuses that one.  (Its other refusal, more than 2^26 participating pixels, needs a handle of that many pixels, which no test
    can afford: the serial program shows it on the same function, test_shared_header_under_sanitizers.)"""
    L = A.lib()
    vp = C.c_void_p
    idle = C.cast(C.create_string_buffer(1 << 20), vp)
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), vp)
    dev = vp(4096)
    res = A.TrackResult()
    nan, inf = float("nan"), float("inf")

    def refused(rc, *words):
        msg = A.last_error()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    def device(h, m=dev, fn=dev, fr=None, mv=None, md=dev, mn=dev, p=None, r=None, null=()):
        fr = _frame() if fr is None else fr
        mv = _view() if mv is None else mv
        return L.adc_track_device(h, m, fn, None if "frame" in null else C.byref(fr), None if "view" in null else C.byref(mv), md, mn, None if p is None else C.byref(p), r)

    def host(h, m=dev, fr=None, p=None, null=()):
        fr = _frame() if fr is None else fr
        return L.adc_tsdf_track(h, m, None if "frame" in null else C.byref(fr), None if p is None else C.byref(p), C.byref(res))

    who = "adc_track_device"
    refused(device(None), who, "null handle")
    refused(device(busy, m=None), who, "null map")
    refused(device(busy, null=("frame",)), who, "null frame")
    refused(device(busy, null=("view",)), who, "null model view")
    refused(device(busy, md=None), who, "null model depth")
    refused(device(busy, mn=None), who, "null model normals")
    for field, values, word in (("width", (0, -1, 8193), "width, height"), ("height", (0, 8193), "width, height"), ("focal_px", (0.0, -1.0, nan, inf), "focal_px"),
                                ("cx", (nan, inf), "cx, cy"), ("cy", (-inf,), "cx, cy")):
        for value in values:
            v = _view()
            setattr(v, field, value)
            refused(device(busy, mv=v), who, "the model view", word)
    for k in range(9):
        v = _view()
        v.R[k] = nan
        refused(device(busy, mv=v), who, "the model view's R")
    v = _view()
    v.t[2] = inf
    refused(device(busy, mv=v), who, "the model view's t")
    v = _view()  # (fields of the view the tracker does not read are not judged)
    v.max_steps, v.step = 0, nan
    refused(device(busy, mv=v), who, "Match is pending")
    for bad, word in ((4097, "d_map must be 4-byte"), (4098, "d_map must be 4-byte")):
        refused(device(busy, m=vp(bad)), who, word)
    for bad in (4096 + 4, 4096 + 8, 4097):
        refused(device(busy, fn=vp(bad)), who, "d_frame_normals must be 16-byte")
        refused(device(busy, mn=vp(bad)), who, "d_model_normals must be 16-byte")
    refused(device(busy, md=vp(4098)), who, "d_model_depth must be 4-byte")
    for bad in (4097, 4100):
        refused(device(busy, r=vp(bad)), who, "d_result must be 8-byte")
    for fn, r in ((None, None), (dev, dev), (None, dev)):
        refused(device(busy, fn=fn, r=r), who, "Match is pending")
    for who, call in (("adc_track_device", device), ("adc_tsdf_track", host)):
        for field, values, word in (("iterations", (0, 33, 2 ** 32 - 1), "iterations"), ("stride", (0, 17), "stride"), ("max_dist", (0.0, -1.0, nan, inf), "max_dist"),
                                    ("min_cos", (-1.5, 1.5, nan), "min_cos"), ("z_far", (0.0, -2.0, nan, inf), "z_far"), ("min_pixels", (0, 5), "min_pixels"),
                                    ("eps_rot", (-1.0e-3, nan), "eps_rot"), ("eps_trans", (-1.0, nan), "eps_rot, eps_trans"), ("max_rot", (0.0, nan, inf), "max_rot"),
                                    ("max_trans", (0.0, -1.0, inf), "max_rot, max_trans"), ("damping", (-0.1, nan, inf), "damping"),
                                    ("pivot_ratio", (-0.1, 1.0, nan), "pivot_ratio"), ("flags", (1, 2 ** 31), "flag")):
            for value in values:
                p = A.TrackParams()
                setattr(p, field, value)
                refused(call(busy, p=p), who, word)
        for k in range(3):
            p = A.TrackParams()
            p.reserved_[k] = 1
            refused(call(busy, p=p), who, "reserved")
        for k in range(9):
            fr = _frame()
            fr.R[k] = nan
            refused(call(busy, fr=fr), who, "R has a non-finite")
        for k in range(3):
            fr = _frame()
            fr.t[k] = -inf
            refused(call(busy, fr=fr), who, "t has a non-finite")
        fr = _frame()
        fr.kind = 7
        refused(call(busy, fr=fr), who, "kind")
        fr = A.TsdfFrame((0.0, 0.16, 40.0, 20.0, 0.0))
        refused(call(busy, fr=fr), who, "focal_px")
        fr = _frame()
        fr.reserved_[4] = 1
        refused(call(busy, fr=fr), who, "reserved")
        refused(call(busy, p=A.TrackParams()), who, "Match is pending")
    refused(host(None), "adc_tsdf_track", "null handle")
    refused(host(busy, m=None), "adc_tsdf_track", "null map")
    refused(host(busy, null=("frame",)), "adc_tsdf_track", "null frame")
    refused(host(idle), "adc_tsdf_track", "no volume")
    refused(device(idle), "adc_track_device", "the frame is empty")  # (the size check, the last one: a zeroed block is a handle of 0 x 0 pixels)
    refused(L.adc_get_track_result(None, C.byref(res)), "null")
    refused(L.adc_get_track_result(idle, None), "null")
    refused(L.adc_get_track_result(idle, C.byref(res)), "no track")
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    assert st.track_device(4096, _frame(), _view(), 4096, 4096) is False and st.track_result() is None


CALLER = r'''
#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
int main() {
    ADCensusStereo s; ADCensusOption o;
    uint8 img[96] = {0};
    float32 d[32] = {0};
    adc_tsdf_frame fr = {};
    fr.kind = ADC_REG_FROM_DEPTH; fr.calib.focal_px = 4.0f; fr.R[0] = fr.R[4] = fr.R[8] = 1.0f;
    TsdfRaycastParams v = {};
    v.width = 4; v.height = 2; v.focal_px = 4.0f; v.R[0] = v.R[4] = v.R[8] = 1.0f;
    TrackParams p = {};
    p.iterations = 2; p.stride = 1; p.max_dist = 0.1f; p.z_far = 4.0f; p.min_pixels = 6; p.max_rot = p.max_trans = 0.5f;
    TrackResult res;
    // before Initialize there is no matcher underneath: everything is refused
    bool ok = !s.Track(d, nullptr, &fr, &v, d, d, &p, nullptr) && !s.TsdfTrack(d, &fr, nullptr, &res) && !s.GetTrackResult(&res);
    return (ok && sizeof(TrackParams) == sizeof(adc_track_params) && sizeof(TrackResult) == 960 && !s.Match(img, img, d) && !s.Initialize(0, 0, o)) ? 0 : 1;
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
    for member in ("Track(void const*, void const*, adc_tsdf_frame const*, adc_tsdf_raycast_params const*, void const*, void const*, adc_track_params const*, void*)",
                   "TsdfTrack(float const*, adc_tsdf_frame const*, adc_track_params const*, adc_track_result*)", "GetTrackResult(adc_track_result*)"):
        assert "ADCensusStereo::" + member in out, member
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def cli_track_reference(disp, bgr, calib, volume, fused, guess):
    """What adcensus_cli --tsdf SPEC --tsdf-track MAP,GUESS has to deliver, by the references: the map `disp` of the pair fused at the pose
    `fused` (R, t; None = the identity) into the volume (nx, ny, nz, voxel, origin, trunc), the volume cast from the guess by the
    frame's own camera with step = voxel / 2 and skip = max(trunc / 2, step), the same map tracked from the guess with the API's defaults
    but z_far, which the CLI sets to the distance from the guess camera to the volume's farthest corner (binary64, rounded once).
    -> (the reference's result, the text of <out>-track.txt, the report line)"""
    from tests import tsdf_raycast_ref as RR
    from tests import tsdf_ref as T
    h, w = disp.shape
    nx, ny, nz, voxel, origin, trunc = volume
    p = T.params(nx, ny, nz, voxel, origin, trunc, flags=T.COLOR)
    vol, _ = T.integrate(T.empty(p), p, T.frame(calib) if fused is None else T.frame(calib, *fused), disp, bgr)
    gR, gt = [float(F(v)) for v in guess[0]], [float(F(v)) for v in guess[1]]
    centre = [-(((gR[a] * gt[0]) + (gR[3 + a] * gt[1])) + (gR[6 + a] * gt[2])) for a in range(3)]
    far2 = 0.0
    for corner in range(8):
        d2 = 0.0
        for a, n in enumerate((nx, ny, nz)):
            d = (float(F(origin[a])) + (float(n if (corner >> a) & 1 else 0) * float(F(voxel)))) - centre[a]
            d2 = d2 + (d * d)
        far2 = max(far2, d2)
    z_far = float(F(np.sqrt(far2)))
    step, half = float(F(voxel) * F(0.5)), float(F(trunc) * F(0.5))
    v = RR.view(w, h, calib[0], calib[2], calib[3], *guess, z_near=float(F(voxel)), z_far=3.0e38, step=step, skip=max(half, step), max_steps=16384)
    cast = RR.raycast(vol, p, v)
    want = TR.track(disp, None, T.frame(calib, *guess), TR.model(w, h, calib[0], calib[2], calib[3], *guess), cast["depth"], cast["normals"], TR.params(z_far=z_far))
    text = "".join("%.9g\n" % x for x in list(want["R"]) + list(want["t"]))
    last = want["iteration"][-1]
    line = "TSDF track: %s after %u solves, %u of %u pixels used, rms %.9g, last step %.9g rad %.9g\n" % (
        ("converged", "max iterations", "lost", "degenerate", "diverged")[want["status"]], want["solves"], want["counts"]["used"], want["counts"]["pixels"], last[1], last[2], last[3])
    return want, text, line


def test_cli_defaults_are_the_api_defaults():
    """adcensus_cli passes the API's defaults with a z_far of its own, so it spells the twelve values out: they are TRACK_DEFAULT's."""
    shared = open(os.path.join(ROOT, "adcensus_amd", "csrc", "tsdf_track.h")).read()
    cli = open(os.path.join(ROOT, "examples", "adcensus_cli.cpp")).read()
    want = re.search(r"TRACK_DEFAULT = (\{[^;]*\});", shared).group(1)
    got = re.findall(r"adc_track_params tp = (\{[^;]*\});", cli)
    assert got == [want], (got, want)


def test_cli_tsdf_track_under_sanitizers(tmp_path):
    """<out>-track.txt and the report line in the ASAN / UBSAN build on the stub C ABI, whose adc_tsdf_track is tsdf_ray.h and
    tsdf_track.h run serially on the stub's host volume: both equal the reference pipeline on the run's own .pfm, with the default
    guess (the pose of --pose) and with a guess file; every other file of the run is byte-identical to a run without the flag.  The
    second frame is the run's own map, so the volume holds exactly its surface: from the pose it was fused at the track has pixels to
    use and must not be LOST."""
    from PIL import Image
    from tests import tsdf_cases as TC
    from tests.test_tsdf_api import read_pfm
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
    volume = (32, 24, 32, 0.04, (-0.64, -0.48, 0.35), float(F(3.0) * F(0.04)))
    fused = (TC.rot(3.0, -4.0, 2.0), (0.02, -0.01, 0.03))
    (tmp_path / "pose.txt").write_text("\n".join("%.9g" % v for v in fused[0] + fused[1]))
    guess = KC.pose(TC.rot(3.4, -3.7, 2.2), (0.03, -0.015, 0.02))
    (tmp_path / "guess.txt").write_text("\n".join("%.9g" % v for v in guess[0] + guess[1]))
    args = ["--calib", ",".join("%.9g" % v for v in calib), "--tsdf", "32,24,32,0.04,-0.64,-0.48,0.35", "--pose", str(tmp_path / "pose.txt")]

    def run(pref, *extra):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "-3", "29", str(tmp_path / pref), *args, *extra], env=SAN_ENV,
                           capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, r.stdout
        return r.stdout

    run("plain")
    names = sorted(f[len("plain"):] for f in os.listdir(tmp_path) if f.startswith("plain-") or f.startswith("plain."))
    assert len(names) >= 5 and "-tsdf.ply" in names and "-track.txt" not in names
    disp = read_pfm(str(tmp_path / "plain.pfm"))
    for pref, spec, g in (("own", str(tmp_path / "plain.pfm"), fused), ("guess", str(tmp_path / "plain.pfm") + "," + str(tmp_path / "guess.txt"), guess)):
        out = run(pref, "--tsdf-track", spec)
        for suffix in names:
            assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / pref) + suffix, "rb").read(), (pref, suffix)
        want, text, line = cli_track_reference(disp, bgr, calib, volume, fused, g)
        assert (tmp_path / (pref + "-track.txt")).read_text() == text, pref
        assert line in out, (line, out[-600:])
        print(pref, TR.STATUS_NAMES[want["status"]], want["solves"], want["counts"])
        if pref == "own":  # (from another guess the stub's synthetic map may well be LOST: then that is what the CLI has to report)
            assert want["status"] != TR.LOST and want["counts"]["used"] >= TR.DEFAULTS["min_pixels"], (want["status"], want["counts"])


def test_cli_rejects_tsdf_track_without_tsdf_and_bad_guesses(tmp_path):
    """Checked while the arguments are parsed: the images named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    base = [cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "0", "64", str(tmp_path / "out")]
    calib = ["--calib", "100,0.16,40,20,0"]
    tsdf = ["--tsdf", "8,8,8,0.1,0,0,1"]
    spec = ["--tsdf-track", str(tmp_path / "second.pfm")]
    for args in (base + spec, base + calib + spec, [base[0]] + spec + base[1:] + calib):
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and r.stdout.startswith("--tsdf-track refused: it needs --tsdf") and "Image Loading" not in r.stdout, r.stdout
    (tmp_path / "short.txt").write_text("1 0 0 0 1 0 0 0 1 0 0")
    (tmp_path / "nan.txt").write_text("1 0 0 0 1 0 0 0 1 0 0 nan")
    for bad in (",", str(tmp_path / "second.pfm") + "," + str(tmp_path / "absent.txt"), str(tmp_path / "second.pfm") + "," + str(tmp_path / "short.txt"),
                str(tmp_path / "second.pfm") + "," + str(tmp_path / "nan.txt")):
        r = subprocess.run(base + calib + tsdf + ["--tsdf-track", bad], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--tsdf-track refused" in r.stdout and "Image Loading" not in r.stdout, (bad, r.stdout)
    (tmp_path / "guess.txt").write_text("1 0 0 0 1 0 0 0 1 0.01 0 0")
    for args in (base + calib + tsdf + spec, base + calib + tsdf + ["--tsdf-track", str(tmp_path / "second.pfm") + "," + str(tmp_path / "guess.txt")]):
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Image Loading" in r.stdout and "refused" not in r.stdout, r.stdout  # (well-formed: gets as far as the images)
