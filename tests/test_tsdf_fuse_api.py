"""CPU tier of the stereo-aware TSDF fusion: properties of the numpy definition (tests/tsdf_fuse_ref.py) on the cases of
tests/tsdf_fuse_cases.py, among them a per-pixel restatement of the weight rule in scalar arithmetic; the header the kernels include
(adcensus_amd/csrc/tsdf_fuse.h), compiled alone under g++ into a serial program (tests/emul/emul_tsdf_fuse.cpp) and held to the
definition bit for bit on every case, once more under ASAN + UBSAN as its own executable; the accuracy checks of
tests/tsdf_fuse_checks.py on the definition; the surface: header, exported symbols, struct layouts, the ctypes mirror, every refusal."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import register_ref as RR
from tests import tsdf_fuse_cases as FC
from tests import tsdf_fuse_checks as FK
from tests import tsdf_fuse_ref as FR
from tests import tsdf_ref as T
from tests.test_tsdf_api import SAN_ENV, c_frame, c_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
F = np.float32


def c_weight_params(w):
    return None if w is None else A.TsdfWeightParams(w["class_weight"], w["min_confidence"], w["flags"], w["depth_power"], w["z_ref"])


def c_fuse_params(fp):
    return None if fp is None else A.TsdfFuseParams(fp["flags"], fp["interp_gap"])


def fuse_words(rep):
    return [rep[k] for k in FR.FUSE_FIELDS] + [0, 0]


def weight_words(rep):
    return [rep[k] for k in FR.WEIGHT_FIELDS] + [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- properties of the definition alone
@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_reference_properties(name):
    c, r = FC.case(name), FC.reference(name)
    p = c["params"]
    vol = c["init"] if c["init"] is not None else T.empty(p)
    for f, after, rep in zip(c["frames"], r["volumes"], r["reports"]):
        assert rep["in_frustum"] == rep["no_depth"] + rep["unweighted"] + rep["occluded"] + rep["updated"], name
        assert rep["interpolated"] <= rep["occluded"] + rep["updated"] and rep["updated"] > 0, name
        assert (after[0] != vol[0]).sum() <= rep["updated"] and T.word_w(after[0]).max() <= p["max_weight"], name  # an untouched voxel keeps its bits
        assert (np.abs(T.word_t(after[0])) <= T.Q).all(), name
        if f["fp"] is None or not f["fp"]["flags"]:
            assert rep["interpolated"] == 0, name
        vol = after


@pytest.mark.parametrize("name", FC.IDENTITY_CASES)
def test_reference_without_weights_is_the_integrate(name):
    """no weight map (or one of all ones) and no flag: the volume and the four common counts of tests/tsdf_ref.integrate"""
    c, r = FC.case(name), FC.reference(name)
    vol = T.empty(c["params"])
    for f, after, rep in zip(c["frames"], r["volumes"], r["reports"]):
        vol, want = T.integrate(vol, c["params"], f["frame"], f["map"], f["image"])
        assert np.array_equal(after[0], vol[0]) and np.array_equal(after[1], vol[1]), name
        assert rep == dict(want, unweighted=0, interpolated=0), name


def test_reference_cases_reach_what_they_are_there_for():
    # 0 / 1 / 255 mixed: every kind of pixel is met, the cap of 300 is reached and not passed
    c, r = FC.case("mixed_weights"), FC.reference("mixed_weights")
    assert all(rep["unweighted"] > 50 for rep in r["reports"]) and T.word_w(r["final"][0]).max() == 300
    assert {1, 2, 255, 256, 300} <= set(T.word_w(r["final"][0]).ravel().tolist())
    # the largest numerator of step 9': w = 65535, t = 32767, q = 32767, wo = 255 -- and the result stays at the cap
    c, r = FC.case("numerator_64bit"), FC.reference("numerator_64bit")
    t0, w0 = T.word_t(c["init"][0]), T.word_w(c["init"][0])
    top = (t0 == T.Q) & (w0 == 65535) & (T.word_t(r["volumes"][0][0]) == T.Q) & (r["volumes"][0][0] != c["init"][0]).any()
    assert top.sum() > 50 and 65534 * 65535 + 65534 * 255 + 32895 > 2 ** 32
    wn = T.word_w(r["final"][0])
    assert wn.max() == 65535 and (wn >= w0).all() and set(wn[w0 == 0].tolist()) == {0, 510} and (T.word_t(r["final"][0]) < T.Q).any()
    # the gap: a spread equal to interp_gap interpolates, one ulp above it does not; fx == 0 / fy == 0 on the axis
    c, r = FC.case("gap_edges"), FC.reference("gap_edges")
    assert r["reports"][0]["interpolated"] > 400 and r["reports"][1]["interpolated"] == 0
    assert not np.array_equal(r["volumes"][0][0], FR.fuse(T.empty(c["params"]), c["params"], c["frames"][1]["frame"], c["frames"][1]["map"], None, None, c["frames"][1]["fp"])[0][0])
    xw, yw, _ = T.centres(c["params"])
    assert xw[7] == 0 and yw[2] == 0 and FC.CALIB_37[2] == int(FC.CALIB_37[2])  # u = cx, v = cy exactly there
    # a plane comes back: on the ramp (depth affine in x) the interpolated distance differs from the analytic one by rounding only
    fr, m = c["frames"][0]["frame"], c["frames"][0]["map"]
    t = T.word_t(r["volumes"][0][0]).astype(np.float64) / T.Q * c["params"]["trunc"]
    zc = T.centres(c["params"])[2].astype(np.float64)[:, None, None]
    u = xw.astype(np.float64)[None, None, :] * FC.CALIB_37[0] / zc + FC.CALIB_37[2]
    inside = (T.word_w(r["volumes"][0][0]) > 0) & (u >= 0) & (u <= 36) & (np.abs(t) < 0.14)
    assert inside.sum() > 200 and np.abs(t - ((0.6875 + u / 128.0) - zc))[inside].max() < 2 * c["params"]["trunc"] / T.Q
    # disparity specials: pixels without depth, and fewer interpolated voxels than with a clean map
    r = FC.reference("disparity_specials")
    assert all(rep["no_depth"] > 50 and 0 < rep["interpolated"] < rep["occluded"] + rep["updated"] for rep in r["reports"])
    # wider than the view: voxels at x0 = W - 1 / y0 = H - 1 use the nearest pixel
    r = FC.reference("corner_wide")
    assert all(0 < rep["interpolated"] < rep["occluded"] + rep["updated"] for rep in r["reports"])
    r = FC.reference("long_row")
    assert r["reports"][0]["unweighted"] > 1000 and r["wreports"][0]["below_confidence"] > 100


def _scalar_weight(v, code, conf, kind, calib, wp):
    """the weight rule of include/adcensus_c_api.h for one pixel, in np.float32 scalars"""
    focal, baseline, _, _, doffs = (F(x) for x in calib)
    v = F(v)
    with np.errstate(all="ignore"):
        if kind == T.FROM_DEPTH:
            if not (np.isfinite(v) and v > 0):
                return -1, False
            D = v
        else:
            a = np.abs(v)
            s = a + doffs
            if not (np.isfinite(a) and s > 0):
                return -1, False
            D = F(focal * baseline) / s
        fill = FR.FILL_WTA if code is None else (int(code) >> 2) & 3
        wc = int(wp["class_weight"][fill])
        if code is not None and int(code) & 0x10:
            wc = 0
        below = False
        if conf is not None and fill == FR.FILL_WTA:
            if not (F(conf) >= F(wp["min_confidence"])):
                wc, below = 0, True
            elif wp["flags"] & FR.W_SCALE_CONFIDENCE:
                cq = int(np.floor(min(max(F(conf), F(0)), F(1)) * F(256) + F(0.5)))
                wc = (wc * cq + 128) >> 8
        if wc == 0 or not np.isfinite(D):
            return 0, below
        g = F(wp["z_ref"]) / D
        s = F(wc)
        if wp["depth_power"] == 2:
            s = s * (g * g)
        elif wp["depth_power"] == 4:
            s = s * ((g * g) * (g * g))
        return int(np.floor(np.minimum(s, F(255)) + F(0.5))), below


@pytest.mark.parametrize("name", FC.WEIGHT_CASE_NAMES)
def test_reference_weights_equal_the_rule_pixel_by_pixel(name):
    c = FC.weight_case(name)
    w, rep = FC.weight_reference(name)
    wp = c["wparams"] or FR.weight_params()
    H, W = c["map"].shape
    want = np.zeros((H, W), np.int64)
    counts = dict(valid=0, nonzero=0, below_confidence=0, saturated=0)
    for y in range(H):
        for x in range(W):
            v, below = _scalar_weight(c["map"][y, x], None if c["prov"] is None else c["prov"][y, x], None if c["conf"] is None else c["conf"][y, x],
                                      c["frame"]["kind"], c["frame"]["calib"], wp)
            want[y, x] = max(v, 0)
            counts["valid"] += v >= 0
            counts["nonzero"] += v > 0
            counts["below_confidence"] += below
            counts["saturated"] += v == 255
    assert np.array_equal(w, want) and rep == counts, name
    assert rep["valid"] == int(RR.source_z(c["map"], c["frame"]["kind"], c["frame"]["calib"])[1].sum()) < W * H and 0 < rep["nonzero"] < rep["valid"]


def test_reference_weight_cases_reach_what_they_are_there_for():
    c, (w, rep) = FC.weight_case("fills_and_speckle"), FC.weight_reference("fills_and_speckle")
    assert set(w.ravel().tolist()) == {0, 7, 30, 90, 200}  # every fill class, the speckle bit, depth_power 0
    D, valid = RR.source_z(c["map"], 0, c["frame"]["calib"])
    assert (w[valid & ((c["prov"] & 0x10) != 0)] == 0).all() and (w[valid & np.isfinite(D) & ((c["prov"] & 0x10) == 0)] > 0).all()
    c, (w, rep) = FC.weight_case("confidence_threshold"), FC.weight_reference("confidence_threshold")
    conf = c["conf"]
    at = valid & (conf == F(0.375)) & np.isfinite(D)
    assert at.any() and (w[at] > 0).all()                                                    # exactly min_confidence passes
    assert (w[np.isnan(conf) | (conf < F(0.375))] == 0).all() and rep["saturated"] > 0       # NaN and everything below fail
    assert (w[valid & (conf > 1) & np.isfinite(D)] > 0).all() and (conf < 0).any() and (conf > 1).any()
    assert (w[valid & np.isinf(D)] == 0).all() and (valid & np.isinf(D)).sum() == 10            # an overflowing fb / s
    _, rep = FC.weight_reference("confidence_scaled")
    assert rep["below_confidence"] > 0
    for a, b in (("defaults_map_only", "fills_and_speckle"),):
        assert FC.weight_case(a)["wparams"] is None and FC.weight_case(b)["wparams"]["depth_power"] == 0
    assert {FC.weight_case(n)["wparams"]["depth_power"] for n in FC.WEIGHT_CASE_NAMES[1:]} == {0, 2, 4}


# ---------------------------------------------------------------------------------------------- the shared header, serially
def _build_emul(tmp, sanitize):
    exe = os.path.join(tmp, "emul_tsdf_fuse_san" if sanitize else "emul_tsdf_fuse")
    cmd = ["g++", "-std=c++17", "-O1" if sanitize else "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "emul", "emul_tsdf_fuse.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emul_fuse(tmp_path_factory):
    return _build_emul(str(tmp_path_factory.mktemp("emul_tsdf_fuse")), False)


def write_emul_case(c, ind):
    W, H = c["size"]
    os.makedirs(ind, exist_ok=True)
    frames = c["frames"]
    with open(os.path.join(ind, "case.bin"), "wb") as f:
        f.write(bytes(c_params(c["params"])))
        f.write(struct.pack("<4i", W, H, len(frames), int(c["init"] is not None)))
        for fr in frames:
            mode = 1 if fr["weight"] is not None else (2 if fr["wparams"] is not None else 0)
            f.write(bytes(c_frame(fr["frame"])) + bytes(c_fuse_params(fr["fp"]) or A.TsdfFuseParams()) + bytes(c_weight_params(fr["wparams"]) or A.TsdfWeightParams()))
            f.write(struct.pack("<4i", int(fr["image"] is not None), mode, int(fr["prov"] is not None), int(fr["conf"] is not None)))

    def plane(key, shape, dtype):
        return np.stack([np.zeros(shape, dtype) if fr[key] is None else np.asarray(fr[key], dtype) for fr in frames])

    plane("map", (H, W), F).tofile(os.path.join(ind, "maps.bin"))
    plane("image", (H, W, 3), np.uint8).tofile(os.path.join(ind, "img.bin"))
    plane("weight", (H, W), np.uint8).tofile(os.path.join(ind, "weights.bin"))
    plane("prov", (H, W), np.uint8).tofile(os.path.join(ind, "prov.bin"))
    plane("conf", (H, W), F).tofile(os.path.join(ind, "conf.bin"))
    if c["init"] is not None:
        c["init"][0].tofile(os.path.join(ind, "init_tsdf.bin"))
        if c["init"][1] is not None:
            c["init"][1].tofile(os.path.join(ind, "init_color.bin"))


def _run_emul(exe, name, tmp):
    c, r = FC.case(name), FC.reference(name)
    W, H = c["size"]
    ind, outd = os.path.join(tmp, "in_" + name), os.path.join(tmp, "out_" + name)
    write_emul_case(c, ind)
    os.makedirs(outd, exist_ok=True)
    run = subprocess.run([exe, ind, outd], env=SAN_ENV, capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr and "LeakSanitizer" not in run.stderr, run.stderr[-3000:]
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert open(os.path.join(outd, "tsdf.bin"), "rb").read() == r["final"][0].tobytes(), name
    if r["final"][1] is not None:
        assert open(os.path.join(outd, "color.bin"), "rb").read() == r["final"][1].tobytes(), name
    assert np.fromfile(os.path.join(outd, "reports.bin"), np.uint32).tolist() == [v for rep in r["reports"] for v in fuse_words(rep)], name
    wmaps = np.fromfile(os.path.join(outd, "wmaps.bin"), np.uint8).reshape(len(c["frames"]), H, W)
    wreps = np.fromfile(os.path.join(outd, "wreports.bin"), np.uint32).reshape(len(c["frames"]), 8)
    for i, (w, wrep) in enumerate(zip(r["wmaps"], r["wreports"])):
        assert np.array_equal(wmaps[i], np.ones((H, W), np.uint8) if w is None else w), (name, i)
        assert wreps[i].tolist() == ([0] * 8 if wrep is None else weight_words(wrep)), (name, i)
    return ind


@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_shared_header_equals_the_reference(emul_fuse, name, tmp_path):
    _run_emul(emul_fuse, name, str(tmp_path))


@pytest.mark.parametrize("name", FC.WEIGHT_CASE_NAMES)
def test_shared_header_weights_equal_the_reference(emul_fuse, name, tmp_path):
    """the weight cases through the serial program: one frame with computed weights into a token volume"""
    wc = FC.weight_case(name)
    c = dict(params=T.params(8, 4, 4, 0.1, (-0.4, -0.2, 0.5), 0.2), size=wc["size"], init=None,
             frames=[dict(frame=wc["frame"], map=wc["map"], image=None, weight=None, wparams=wc["wparams"] or FR.weight_params(), prov=wc["prov"], conf=wc["conf"], fp=None)])
    ind, outd = str(tmp_path / "in"), str(tmp_path / "out")
    write_emul_case(c, ind)
    os.makedirs(outd)
    assert subprocess.run([emul_fuse, ind, outd], capture_output=True, timeout=300).returncode == 0
    w, rep = FC.weight_reference(name)
    assert open(os.path.join(outd, "wmaps.bin"), "rb").read() == w.tobytes(), name
    assert np.fromfile(os.path.join(outd, "wreports.bin"), np.uint32).tolist() == weight_words(rep), name


def test_shared_header_under_sanitizers(tmp_path):
    """The same program built once with ASAN + UBSAN and run as its own executable: a read outside the map, the weight map, the four
    taps or the volume, an overflowing integer and a leak are reports, and a report is a failure."""
    exe = _build_emul(str(tmp_path), True)
    for name in FC.CASE_NAMES:
        ind = _run_emul(exe, name, str(tmp_path))
    assert subprocess.run([exe], env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe, str(tmp_path / "absent"), str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2
    blob = bytearray(open(os.path.join(ind, "case.bin"), "rb").read())
    blob[0:4] = struct.pack("<i", 6)  # nx no multiple of 4
    open(os.path.join(ind, "case.bin"), "wb").write(bytes(blob))
    assert subprocess.run([exe, ind, str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------- accuracy of the definition
def test_staircase_chain_fails_with_nearest_and_holds_with_bilinear_sampling():
    """profiles/tsdf_fuse_accuracy.md (a).  The premise is pinned: with nearest sampling the chain's own criterion fails."""
    near = FK.check_staircase(FR.fuse, False)
    print("nearest :", near)
    assert near["final"] > 0.1 * near["initial"] and not FK.chain_criterion(near)
    bil = FK.check_staircase(FR.fuse, True)
    print("bilinear:", bil)
    assert bil["final"] <= bil["voxel"] and bil["final"] <= 0.1 * bil["initial"] and FK.chain_criterion(bil)
    text = open(os.path.join(ROOT, "profiles", "tsdf_fuse_accuracy.md")).read()
    assert "| nearest | %.4f | %.4f |" % (near["final"], near["ratio"]) in text and "| bilinear | %.4f | %.4f |" % (bil["final"], bil["ratio"]) in text


def test_noise_scene_z4_weights_and_bilinear_against_uniform_nearest():
    """profiles/tsdf_fuse_accuracy.md (b): the ratio of the rms depth errors is at most 1.5 times the one measured on this definition."""
    m = FK.check_noise(FR.fuse, FR.weights)
    print(m)
    assert FK.NOISE_BOUND < 0.75 and m["ratio"] <= FK.NOISE_BOUND and min(m["pixels"]) > 15000
    assert abs(m["ratio"] - FK.NOISE_MEASURED_RATIO) < 5e-4  # (the recorded figure is this definition's)
    text = open(os.path.join(ROOT, "profiles", "tsdf_fuse_accuracy.md")).read()
    assert "| z4 | bilinear | %.4f |" % m["z4_bilinear"] in text and "| uniform | nearest | %.4f |" % m["uniform_nearest"] in text


# ---------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name in A.TSDF_FUSE_ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    assert re.search(r"#define\s+ADC_TSDF_FUSE_BILINEAR\s+1u", text) and re.search(r"#define\s+ADC_TSDF_W_SCALE_CONFIDENCE\s+1u", text)
    assert A.TSDF_FUSE_BILINEAR == FR.FUSE_BILINEAR == 1 and A.TSDF_W_SCALE_CONFIDENCE == FR.W_SCALE_CONFIDENCE == 1
    for phrase in ("t' = ((t + 32767) * w + (q + 32767) * wo + m / 2) / m - 32767", "With wo == 1 this is step 9 bit for bit",
                   "in_frustum = no_depth + unweighted + occluded + updated", "wc = (wc * cq + 128) >> 8", "a plane comes back exactly up to rounding"):
        assert phrase in text, phrase
    for lib in (A.LIB_PATH, os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(A.TSDF_FUSE_ENTRY_POINTS) <= names, lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(adc_tsdf_weight_params), offsetof(adc_tsdf_weight_params, min_confidence),\n'
                   ' offsetof(adc_tsdf_weight_params, flags), offsetof(adc_tsdf_weight_params, depth_power), offsetof(adc_tsdf_weight_params, z_ref),\n'
                   ' offsetof(adc_tsdf_weight_params, reserved_), sizeof(adc_tsdf_fuse_params), offsetof(adc_tsdf_fuse_params, interp_gap),\n'
                   ' offsetof(adc_tsdf_fuse_params, reserved_), sizeof(adc_tsdf_weight_report), sizeof(adc_tsdf_fuse_report), offsetof(adc_tsdf_fuse_report, interpolated));\n'
                   ' return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    Wp, Fp = A.TsdfWeightParams, A.TsdfFuseParams
    assert got == [C.sizeof(Wp), Wp.min_confidence.offset, Wp.flags.offset, Wp.depth_power.offset, Wp.z_ref.offset, Wp.reserved_.offset, C.sizeof(Fp),
                   Fp.interp_gap.offset, Fp.reserved_.offset, C.sizeof(A.TsdfWeightReport), C.sizeof(A.TsdfFuseReport), A.TsdfFuseReport.interpolated.offset]
    assert got[0] == 64 and got[6] == 32 and got[9:] == [32, 32, 20]
    assert [f[0] for f in A.TsdfFuseReport._fields_] == list(FR.FUSE_FIELDS) + ["reserved_"]
    assert [f[0] for f in A.TsdfWeightReport._fields_] == list(FR.WEIGHT_FIELDS) + ["reserved_"]
    d = A.TsdfWeightParams()
    assert (list(d.class_weight), d.min_confidence, d.flags, d.depth_power, d.z_ref) == ([16, 4, 1, 0], 0.0, 0, 4, 1.0) and FR.weight_params() == dict(
        class_weight=(16, 4, 1, 0), min_confidence=0.0, flags=0, depth_power=4, z_ref=1.0)
    assert (A.TsdfFuseParams().flags, A.TsdfFuseParams().interp_gap) == (0, 0.0)


def test_every_refusal_comes_before_a_hip_call():
    """No device here: each of these returns 1 with a message without touching HIP.  A block of ones stands in for a handle that has a
    volume (with colour) and a Match pending, the last check of all; a zeroed block for an idle handle without a volume."""
    L = A.lib()
    vp = C.c_void_p
    idle = C.cast(C.create_string_buffer(1 << 20), vp)
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), vp)
    dev = vp(4096)
    calib = (100.0, 0.16, 10.0, 5.0, 0.0)
    good = A.TsdfFrame(calib)
    inf, nan = float("inf"), float("nan")
    frep, wrep = A.TsdfFuseReport(), A.TsdfWeightReport()

    def refused(rc, *words):
        msg = A.last_error()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    def ref(x):
        return None if x is None else C.byref(x)

    bad_frames = [(A.TsdfFrame(calib, kind=2), "kind"), (A.TsdfFrame((nan,) + calib[1:]), "non-finite"), (A.TsdfFrame((0.0,) + calib[1:]), "focal_px must be positive"),
                  (A.TsdfFrame(calib, [inf] * 9), "R has a non-finite"), (A.TsdfFrame(calib, None, [nan, 0, 0]), "t has a non-finite"), (A.TsdfFrame(calib, flags=1), "unknown flag")]
    reserved = A.TsdfFrame(calib)
    reserved.reserved_[4] = 1
    bad_frames.append((reserved, "reserved"))
    # weights
    for who, call in (("adc_tsdf_weights_device", lambda h, m, fr, wp, w, prov=None, conf=None: L.adc_tsdf_weights_device(h, m, prov, conf, ref(fr), ref(wp), w)),
                      ("adc_tsdf_weights", lambda h, m, fr, wp, w, prov=None, conf=None: L.adc_tsdf_weights(h, m, prov, conf, ref(fr), ref(wp), w, C.byref(wrep)))):
        refused(call(None, dev, good, None, dev), who, "null handle")
        refused(call(busy, None, good, None, dev), who, "null map")
        refused(call(busy, dev, good, None, None), who, "null weight")
        refused(call(busy, dev, None, None, dev), who, "null frame")
        for fr, why in bad_frames:
            refused(call(busy, dev, fr, None, dev), who, why)
        for kw, why in ([(dict(min_confidence=v), "min_confidence") for v in (-0.1, 1.5, nan, inf)] + [(dict(flags=v), "unknown flag") for v in (2, 3, 0x80000000)] +
                        [(dict(depth_power=v), "depth_power") for v in (1, 3, 5, 8)] + [(dict(z_ref=v), "z_ref") for v in (0.0, -1.0, nan, inf)]):
            refused(call(busy, dev, good, A.TsdfWeightParams(**kw), dev), who, why)
        for k in range(11):
            wp = A.TsdfWeightParams()
            wp.reserved_[k] = 1
            refused(call(busy, dev, good, wp, dev), who, "reserved")
        for wp in (None, A.TsdfWeightParams(), A.TsdfWeightParams((255, 255, 255, 255), 1.0, 1, 0, 1e30), A.TsdfWeightParams(depth_power=2)):
            refused(call(busy, dev, good, wp, dev), who, "Match is pending")   # (needs no volume: the pending Match is all that is left)
            refused(call(busy, dev, good, wp, dev, dev, dev), who, "Match is pending")
    for bad in (4097, 4098, 4099):
        refused(L.adc_tsdf_weights_device(busy, vp(bad), None, None, C.byref(good), None, dev), "adc_tsdf_weights_device", "d_map must be 4-byte aligned")
        refused(L.adc_tsdf_weights_device(busy, dev, None, vp(bad), C.byref(good), None, dev), "adc_tsdf_weights_device", "d_confidence must be 4-byte aligned")
        refused(L.adc_tsdf_weights_device(busy, dev, vp(bad), None, C.byref(good), None, vp(bad)), "Match is pending")  # (bytes may lie anywhere)
    # fuse
    for who, call in (("adc_tsdf_fuse_device", lambda h, m, fr, fp=None, w=None, img=None: L.adc_tsdf_fuse_device(h, m, img, w, ref(fr), ref(fp))),
                      ("adc_tsdf_fuse", lambda h, m, fr, fp=None, w=None, img=None: L.adc_tsdf_fuse(h, m, img, w, ref(fr), ref(fp), C.byref(frep)))):
        refused(call(None, dev, good), who, "null handle")
        refused(call(busy, None, good), who, "null map")
        refused(call(busy, dev, None), who, "null frame")
        for fr, why in bad_frames:
            refused(call(busy, dev, fr), who, why)
        for kw, why in ([(dict(flags=v), "unknown flag") for v in (2, 3, 0x80000000)] + [(dict(interp_gap=v), "interp_gap") for v in (-0.1, nan, inf, -inf)]):
            refused(call(busy, dev, good, A.TsdfFuseParams(**kw)), who, why)
        for k in range(6):
            fp = A.TsdfFuseParams(1, 0.5)
            fp.reserved_[k] = 1
            refused(call(busy, dev, good, fp), who, "reserved")
        refused(call(idle, dev, good), who, "no volume")
        refused(call(idle, dev, good, A.TsdfFuseParams(1, 0.2), dev), who, "no volume")
        for fp in (None, A.TsdfFuseParams(), A.TsdfFuseParams(1, 0.0), A.TsdfFuseParams(1, 3e38)):
            refused(call(busy, dev, good, fp), who, "Match is pending")
            refused(call(busy, dev, good, fp, dev, dev), who, "Match is pending")
    for bad in (4097, 4098, 4099):
        refused(L.adc_tsdf_fuse_device(busy, vp(bad), None, None, C.byref(good), None), "adc_tsdf_fuse_device", "4-byte aligned")
        refused(L.adc_tsdf_fuse_device(busy, dev, vp(bad), vp(bad), C.byref(good), None), "Match is pending")  # (bytes: image and weights may lie anywhere)
    # an image without a colour volume: refused, not ignored (a block whose flags word is 0 but whose volume is set cannot be faked
    # here; tests/test_gpu_tsdf_fuse.py holds it)
    # the report
    refused(L.adc_get_tsdf_fuse_report(None, C.byref(frep), None), "adc_get_tsdf_fuse_report", "null argument")
    refused(L.adc_get_tsdf_fuse_report(idle, None, None), "adc_get_tsdf_fuse_report", "null argument")
    refused(L.adc_get_tsdf_fuse_report(idle, C.byref(frep), None), "adc_get_tsdf_fuse_report", "no fuse call has completed")
    refused(L.adc_get_tsdf_fuse_report(idle, None, C.byref(wrep)), "adc_get_tsdf_fuse_report", "no weights call has completed")


# ---------------------------------------------------------------------------------------------- the CLI on the stub, under sanitizers
def test_cli_tsdf_fuse_under_sanitizers(tmp_path):
    """--tsdf-fuse in the ASAN / UBSAN build of the CLI on the stub C ABI, whose fusion is tsdf_fuse.h run serially: the flag's parsing,
    the report lines and <out>-tsdf.ply equal tests/tsdf_fuse_ref.py on the run's own .pfm and the provenance and confidence maps of the
    same Match (the files of a run with --extras: the CLI keeps --calib and --extras apart, and the stub's maps are a function of the
    pixel and its disparity alone); every other file of the run is
    byte-identical to a run without the flag."""
    from PIL import Image
    from tests.test_tsdf_api import read_pfm, read_tsdf_ply
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
    spec = "32,24,32,0.04,-0.64,-0.48,0.35,0.08"
    p = T.params(32, 24, 32, 0.04, (-0.64, -0.48, 0.35), 0.08, flags=T.COLOR)

    def run(pref, *extra, rc=0):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "-3", "29", str(tmp_path / pref), *extra], env=SAN_ENV,
                           capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == rc, r.stdout
        return r.stdout

    for bad in ("", "16,4,1,0,0.1,4", "16,4,1,0,0.1,3,1.5", "16,4,1,256,0.1,4,1.5", "16,4,1,0,1.5,4,1.5", "16,4,1,0,0.1,4,0", "16,4,1,0,0.1,4,1.5,-1", "16,4,1,0,0.1,4,1.5,0.5,7",
                "16,4,1,0,0.1,4,1.5x"):
        assert "--tsdf-fuse refused" in run("bad", "--tsdf", spec, *calib_arg, "--tsdf-fuse", bad, rc=255), bad
    assert "--tsdf-fuse refused: it needs --tsdf" in run("bad", *calib_arg, "--tsdf-fuse", "16,4,1,0,0.1,4,1.5", rc=255)
    run("plain", "--tsdf", spec, *calib_arg)
    names = sorted(f[len("plain"):] for f in os.listdir(tmp_path) if (f.startswith("plain-") or f.startswith("plain.")) and not f.endswith("-tsdf.ply"))
    assert len(names) >= 4
    run("maps", "--extras")
    prov = np.array(Image.open(tmp_path / "maps-prov.png"))
    conf = read_pfm(str(tmp_path / "maps-conf.pfm"))
    assert prov.shape == (h, w) and len(set(prov.ravel().tolist())) > 4 and conf.max() > 0.9
    for pref, arg, wp, fp in (("f1", "16,4,1,0,0.25,0,1", FR.weight_params((16, 4, 1, 0), 0.25, 0, 0, 1.0), FR.fuse_params()),
                              ("f2", "200,90,30,7,0,2,0.9,1.5", FR.weight_params((200, 90, 30, 7), 0.0, 0, 2, 0.9), FR.fuse_params(FR.FUSE_BILINEAR, 1.5)),
                              ("f3", "16,4,1,0,0.5,4,1.25,0", FR.weight_params((16, 4, 1, 0), 0.5, 0, 4, 1.25), FR.fuse_params(FR.FUSE_BILINEAR, 0.0))):
        out = run(pref, "--tsdf", spec, *calib_arg, "--tsdf-fuse", arg)
        for suffix in names:
            assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / pref) + suffix, "rb").read(), (pref, suffix)
        m = read_pfm(str(tmp_path / pref) + ".pfm")
        fr = T.frame(calib)
        wmap, wrep = FR.weights(m, fr, wp, prov, conf)
        vol, rep = FR.fuse(T.empty(p), p, fr, m, bgr, wmap, fp)
        pts, xrep = T.extract(vol, p, 1)
        pts = pts.copy()
        pts["pad"] = 0
        assert read_tsdf_ply(str(tmp_path / pref) + "-tsdf.ply").tobytes() == pts.tobytes(), pref
        assert "TSDF: %u voxels in the frustum, %u without depth, %u occluded, %u updated; %u voxels seen, %u surface points\n" % (
            rep["in_frustum"], rep["no_depth"], rep["occluded"], rep["updated"], xrep["voxels_seen"], xrep["points"]) in out, out
        assert "TSDF fuse: %u pixels with depth, %u weighted, %u below the confidence, %u saturated; %u voxels unweighted, %u interpolated\n" % (
            wrep["valid"], wrep["nonzero"], wrep["below_confidence"], wrep["saturated"], rep["unweighted"], rep["interpolated"]) in out, out
        assert rep["updated"] > 500 and rep["unweighted"] > 0 and len(pts) > 0, (pref, rep)
        assert (rep["interpolated"] > 0) == (pref == "f2"), (pref, rep)
