"""CPU tier of the moving TSDF volume: the numpy definition's own properties; the rule the kernels include
(adcensus_amd/csrc/tsdf_shift.h), compiled alone under g++ into a serial program (tests/emul/emul_tsdf_shift.cpp) and held to the numpy
definition on every case of tests/tsdf_shift_cases.py, once more as a stand-alone ASAN + UBSAN build; the follow rule against numpy on
drawn poses, with its two properties; the surface (symbols, struct layouts) and every refusal, none of which reaches a HIP call."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import tsdf_ref as T
from tests import tsdf_shift_cases as SC
from tests import tsdf_shift_ref as SR
from tests.test_tsdf_api import HEADER, ROOT, SAN_ENV, c_params

F = np.float32
VOLS = tuple(SC.VOLUMES)


def c_shift_params(sp):
    return A.TsdfShiftParams(sp["shift"], sp["min_weight"])


def c_follow_params(fp):
    return A.TsdfFollowParams(fp["anchor"], fp["margin"], fp["quantum"])


# ---------------------------------------------------------------------------------------------- properties of the reference alone
@pytest.mark.parametrize("vol", VOLS)
def test_reference_properties(vol):
    nx, ny, nz = SC.VOLUMES[vol]
    old = SC.volume(vol, True)
    p = SC.params(vol, True)
    full, xrep = T.extract(old, p, 1)
    for s in SC.shifts(vol):
        new, q, off, pts, rep = SC.reference(vol, True, s, 1)
        lv = SR.leaves(old[0].shape, s)
        if s == (0, 0, 0):
            assert rep == dict.fromkeys(SR.SHIFT_FIELDS, 0) and len(pts) == 0 and q == p and np.array_equal(new[0], old[0])
            continue
        # every word either moved or left, and what re-enters is empty
        assert rep["moved_nonempty"] + rep["left_nonempty"] == int((old[0] != 0).sum()), s
        assert int(lv.sum()) == old[0].size - int(np.prod([max(n - abs(v), 0) for n, v in zip((nx, ny, nz), s)])), s
        assert off == s and q["origin"] == tuple(float(F(p["origin"][a]) + F(s[a]) * F(SC.VOXEL)) for a in range(3)), s
        if any(abs(s[a]) >= n for a, n in enumerate((nx, ny, nz))):
            assert not new[0].any() and not new[1].any() and pts.tobytes() == full.tobytes() and rep["left_seen"] == xrep["voxels_seen"], s
        else:
            # exactly once: what left plus what the shifted volume still holds is the untouched volume's list (dyadic geometry: the
            # records of a crossing are the same bits from either origin)
            rest, _ = T.extract(new, q, 1)
            both = np.concatenate([pts, rest])
            assert sorted(both.view("V16").tolist()) == sorted(full.view("V16").tolist()), s


def test_reference_two_shifts_against_one():
    """two successive shifts lose what left in between; a single shift by their sum does not"""
    vol = "v12x7x9"
    old, p = SC.volume(vol, True), SC.params(vol, True)
    a, b = (3, 0, -2), (-3, 1, 2)
    v1, p1, o1, _, _ = SR.shift(old, p, SR.shift_params(a))
    v2, p2, o2, _, _ = SR.shift(v1, p1, SR.shift_params(b), o1, p["origin"])
    one, q, off, _, _ = SR.shift(old, p, SR.shift_params((0, 1, 0)))
    assert o2 == off == (0, 1, 0) and p2 == q
    differ = v2[0] != one[0]
    assert differ.any() and not v2[0][differ].any()  # (where they differ, the two-step volume is empty)
    lost = SR.move(SR.move(np.ones_like(old[0]), a), b) == 0
    assert np.array_equal(differ, lost & (one[0] != 0))


def test_cases_hold_every_kind_of_crossing():
    """tests/tsdf_shift_cases.py asserts it at import; here the figures, and that both variants of the shift kernel are reached"""
    for vol in VOLS:
        mod4 = {s[0] % 4 == 0 for s in SC.shifts(vol) if s != (0, 0, 0) and all(abs(s[a]) < SC.VOLUMES[vol][a] for a in range(3))}
        assert mod4 == {True, False}, vol
        for s in SC.shifts(vol):
            if SC.all_in_range(vol, s):
                for mw in SC.MIN_WEIGHTS:
                    _, kinds = SR.leaving_list(SC.volume(vol, True), SC.params(vol, True), s, mw)
                    assert set(np.unique(kinds).tolist()) == {1, 2, 3}, (vol, s, mw)


# ---------------------------------------------------------------------------------------------- the shared header, serially
def _build_emul(tmp, sanitize):
    exe = os.path.join(tmp, "emul_tsdf_shift_san" if sanitize else "emul_tsdf_shift")
    cmd = ["g++", "-std=c++17", "-O1" if sanitize else "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "emul", "emul_tsdf_shift.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emul_shift(tmp_path_factory):
    return _build_emul(str(tmp_path_factory.mktemp("emul_tsdf_shift")), False)


def follow_record(p, R, t, fp):
    return bytes(c_params(p)) + struct.pack("<12f", *R, *t) + bytes(c_follow_params(fp))


def write_emul_case(ind, p, volume, shift_list, follows=()):
    os.makedirs(ind, exist_ok=True)
    with open(os.path.join(ind, "case.bin"), "wb") as f:
        f.write(bytes(c_params(p)) + struct.pack("<2i", len(shift_list), len(follows)))
        for sp in shift_list:
            f.write(bytes(c_shift_params(sp)))
        for rec in follows:
            f.write(follow_record(*rec))
    volume[0].tofile(os.path.join(ind, "init_tsdf.bin"))
    if volume[1] is not None:
        volume[1].tofile(os.path.join(ind, "init_color.bin"))


def run_emul(exe, ind, outd, rc=0):
    os.makedirs(outd, exist_ok=True)
    run = subprocess.run([exe, ind, outd], env=SAN_ENV, capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr and "LeakSanitizer" not in run.stderr, run.stderr[-3000:]
    assert run.returncode == rc, (run.returncode, run.stderr[-2000:])


def _emul_against_numpy(exe, vol, colour, tmp):
    """every shift of the volume as a one-shift run, then the whole list as one sequence"""
    p, old = SC.params(vol, colour), SC.volume(vol, colour)

    def check(outd, i, new, q, off, pts, rep, what):
        assert open(os.path.join(outd, "tsdf_%d.bin" % i), "rb").read() == new[0].tobytes(), what
        if colour:
            assert open(os.path.join(outd, "color_%d.bin" % i), "rb").read() == new[1].tobytes(), what
        assert open(os.path.join(outd, "points_%d.bin" % i), "rb").read() == pts.tobytes(), what
        reps = np.fromfile(os.path.join(outd, "reports.bin"), np.uint32).reshape(-1, 8)
        assert reps[i].tolist() == SR.report_words(rep) + [0] * 4, (what, reps[i], rep)
        state = np.fromfile(os.path.join(outd, "state.bin"), np.uint32).reshape(-1, 6)
        assert state[i, :3].view(np.int32).tolist() == list(off) and state[i, 3:].view(F).tolist() == [float(F(v)) for v in q["origin"]], what

    for mw in SC.MIN_WEIGHTS:
        for n, s in enumerate(SC.shifts(vol)):
            ind, outd = os.path.join(tmp, "in_%d_%d" % (mw, n)), os.path.join(tmp, "out_%d_%d" % (mw, n))
            write_emul_case(ind, p, old, [SR.shift_params(s, mw)])
            run_emul(exe, ind, outd)
            check(outd, 0, *SC.reference(vol, colour, s, mw), (vol, colour, s, mw))
    seq = [s for s in SC.shifts(vol) if all(abs(s[a]) < SC.VOLUMES[vol][a] for a in range(3))]
    ind, outd = os.path.join(tmp, "in_seq"), os.path.join(tmp, "out_seq")
    write_emul_case(ind, p, old, [SR.shift_params(s, 1) for s in seq])
    run_emul(exe, ind, outd)
    cur, q, off = old, p, (0, 0, 0)
    for i, s in enumerate(seq):
        cur, q, off, pts, rep = SR.shift(cur, q, SR.shift_params(s, 1), off, p["origin"])
        check(outd, i, cur, q, off, pts, rep, (vol, colour, "sequence", i, s))
    return ind


@pytest.mark.parametrize("colour", (False, True))
@pytest.mark.parametrize("vol", VOLS)
def test_shared_header_equals_the_reference(emul_shift, vol, colour, tmp_path):
    _emul_against_numpy(emul_shift, vol, colour, str(tmp_path))


def test_shared_header_under_sanitizers(tmp_path):
    """The same program built once with ASAN + UBSAN and run as its own executable: a read outside a plane, an overflowing integer (a
    shift of 2^24 on a small box, n + delta) and a leak are reports, and a report is a failure."""
    exe = _build_emul(str(tmp_path), True)
    for vol in VOLS:
        ind = _emul_against_numpy(exe, vol, vol != "v8x6x5", str(tmp_path / vol))
    assert subprocess.run([exe], env=SAN_ENV, capture_output=True).returncode == 2
    assert subprocess.run([exe, str(tmp_path / "absent"), str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2
    p, old = SC.params("v8x6x5", False), SC.volume("v8x6x5", False)
    for bad in (dict(shift=(1 << 24, 0, 0), min_weight=0), dict(shift=((1 << 24) + 1, 0, 0), min_weight=1), dict(shift=(0, -(1 << 31), 0), min_weight=1)):
        write_emul_case(str(tmp_path / "bad"), p, old, [bad])
        run_emul(exe, str(tmp_path / "bad"), str(tmp_path / "bad_out"), rc=2)
    # the offset is a sum: two shifts that pass 2^24 together
    write_emul_case(str(tmp_path / "sum"), p, old, [SR.shift_params((0, 0, 1 << 24)), SR.shift_params((0, 0, 1))])
    run_emul(exe, str(tmp_path / "sum"), str(tmp_path / "sum_out"), rc=2)
    write_emul_case(str(tmp_path / "back"), p, old, [SR.shift_params((0, 0, 1 << 24)), SR.shift_params((0, 0, -(1 << 25)))])
    run_emul(exe, str(tmp_path / "back"), str(tmp_path / "back_out"))
    blob = bytearray(open(os.path.join(ind, "case.bin"), "rb").read())
    blob[0:4] = struct.pack("<i", 6)  # nx no multiple of 4
    open(os.path.join(ind, "case.bin"), "wb").write(bytes(blob))
    assert subprocess.run([exe, ind, str(tmp_path)], env=SAN_ENV, capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------- the follow rule
def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return tuple(float(F(v)) for v in R.ravel())


def _poses(count, seed):
    """(params, R, t, follow params): dyadic volumes, random rotations, camera centres up to a few volumes away from the centre"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = (int(rng.integers(1, 17)) * 4, int(rng.integers(4, 65)), int(rng.integers(4, 65)))
        voxel = 2.0 ** -int(rng.integers(3, 8))
        origin = tuple(float(int(v)) * voxel for v in rng.integers(-4000, 4000, 3))
        p = T.params(*n, voxel, origin, 4 * voxel)
        R = _rotation(rng)
        c = np.array(origin) + np.array(n) * voxel * rng.uniform(-3.0, 4.0, 3)
        t = tuple(float(F(v)) for v in -(np.array(R).reshape(3, 3) @ c))
        margin = int(rng.integers(0, 12))
        quantum = int(rng.integers(1, max(margin, 1) + 1))
        out.append((p, R, t, SR.follow_params((float(F(rng.normal() * 0.2)), float(F(rng.normal() * 0.2)), float(F(rng.uniform(0.0, 3.0)))), margin, quantum)))
    return out


def test_follow_rule_equals_numpy_and_keeps_its_two_properties(emul_shift, tmp_path):
    poses = _poses(300, 5) + [(T.params(8, 8, 8, 0.25, (0.0, 0.0, 0.0), 1.0), T.IDENTITY, (0.0, 0.0, 0.0), SR.follow_params((1.0, 1.0, 1.0), 0, 1)),
                              (T.params(8, 8, 8, 0.25, (0.0, 0.0, 0.0), 1.0), T.IDENTITY, (-3e38, 3e38, 0.0), SR.follow_params((3e38, -3e38, 1.0), 3, 2))]
    want = [SR.follow_plan(*rec) for rec in poses]
    assert want[-2] == (0, 0, 0) and want[-1] == (1 << 30, -(1 << 30), 0)
    got = [A.tsdf_follow_plan(c_params(p), R, t, c_follow_params(fp)) for p, R, t, fp in poses]
    assert got == want
    ind, outd = str(tmp_path / "in"), str(tmp_path / "out")
    write_emul_case(ind, SC.params("v8x6x5", False), SC.volume("v8x6x5", False), [], poses)
    run_emul(emul_shift, ind, outd)
    assert np.fromfile(os.path.join(outd, "follow.bin"), np.int32).reshape(-1, 3).tolist() == [list(w) for w in want]
    moved = 0
    for (p, R, t, fp), s in zip(poses[:-1], want[:-1]):
        n = (p["nx"], p["ny"], p["nz"])
        Rm, d = np.array(R, np.float64).reshape(3, 3), np.array(fp["anchor"], np.float64) - np.array(t, np.float64)
        off_centre = Rm.T @ d - (np.array(p["origin"], np.float64) + np.array(n) * p["voxel"] / 2.0)
        for a in range(3):
            # the sign of a shift follows the anchor; no shift inside the margin; a shift never overshoots the anchor
            if s[a] != 0:
                assert np.sign(s[a]) == np.sign(off_centre[a]) and abs(s[a]) * p["voxel"] <= abs(off_centre[a]) + 1e-9 and s[a] % fp["quantum"] == 0
            assert (s[a] != 0) or abs(off_centre[a]) / p["voxel"] <= fp["margin"] + 1e-6 or fp["quantum"] > abs(off_centre[a]) / p["voxel"]
        # applied, the next plan is zero (quantum <= margin; dyadic geometry: |shift| * voxel and the new origin are exact)
        assert fp["quantum"] <= max(fp["margin"], 1)
        if fp["quantum"] <= fp["margin"]:
            q = dict(p)
            q["origin"] = SR.origin_after(p["origin"], s, p["voxel"])
            assert all(np.float64(q["origin"][a]) == np.float64(p["origin"][a]) + s[a] * np.float64(p["voxel"]) for a in range(3))
            assert SR.follow_plan(q, R, t, fp) == (0, 0, 0) and A.tsdf_follow_plan(c_params(q), R, t, c_follow_params(fp)) == (0, 0, 0), (p, s)
            moved += s != (0, 0, 0)
    assert moved > 100


# ---------------------------------------------------------------------------------------------- the surface
def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name in A.TSDF_SHIFT_ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(" % name, text), name
    for phrase in ("origin[a] = origin0[a] + (float)offset[a] * voxel", "CHANGE WITH EVERY NON-ZERO SHIFT", "shift[a] = quantum * trunc(p / quantum) if |p| > margin",
                   "An old voxel LEAVES iff (i - sx, j - sy, k - sz) lies outside the box", "handed out at\n * most once"):
        assert phrase in text, phrase
    for lib in (A.LIB_PATH, os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(A.TSDF_SHIFT_ENTRY_POINTS) <= names, lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adcensus_c_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(adc_tsdf_shift_params), offsetof(adc_tsdf_shift_params, min_weight),\n'
                   ' offsetof(adc_tsdf_shift_params, flags), offsetof(adc_tsdf_shift_params, reserved_), sizeof(adc_tsdf_shift_report), offsetof(adc_tsdf_shift_report, points),\n'
                   ' sizeof(adc_tsdf_follow_params), offsetof(adc_tsdf_follow_params, margin), offsetof(adc_tsdf_follow_params, quantum), offsetof(adc_tsdf_follow_params, reserved_));\n'
                   ' return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    Sp, Sr, Fp = A.TsdfShiftParams, A.TsdfShiftReport, A.TsdfFollowParams
    assert got == [C.sizeof(Sp), Sp.min_weight.offset, Sp.flags.offset, Sp.reserved_.offset, C.sizeof(Sr), Sr.points.offset, C.sizeof(Fp), Fp.margin.offset,
                   Fp.quantum.offset, Fp.reserved_.offset]
    assert got == [32, 12, 16, 20, 32, 12, 32, 12, 16, 20]
    assert [f[0] for f in Sr._fields_] == list(SR.SHIFT_FIELDS) + ["reserved_"]
    assert A.TSDF_SHIFT_MAX_OFFSET == SR.MAX_OFFSET == 1 << 24


def test_every_refusal_comes_before_a_hip_call():
    """No device here: each of these returns 1 with a message without touching HIP.  A block of ones stands in for a handle that has a
    volume and a Match pending, the last check but one -- its offset words read 0x01010101, 65793 voxels short of 2^24, which is what
    the offset rule is tried on; a zeroed block for an idle handle without a volume."""
    L = A.lib()
    vp = C.c_void_p
    idle = C.cast(C.create_string_buffer(1 << 20), vp)
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), vp)
    dev = vp(4096)
    rep = A.TsdfShiftReport()

    def refused(rc, *words):
        msg = A.last_error()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    def ref(x):
        return None if x is None else C.byref(x)

    good = A.TsdfShiftParams((-70000, -80000, -90000))
    for who, call in (("adc_tsdf_shift_device", lambda h, sp, pts=dev, cap=8, cnt=None: L.adc_tsdf_shift_device(h, ref(sp), pts, cap, cnt)),
                      ("adc_tsdf_shift", lambda h, sp, pts=dev, cap=8, cnt=None: L.adc_tsdf_shift(h, ref(sp), pts, cap, C.byref(rep)))):
        refused(call(None, good), who, "null handle")
        refused(call(busy, None), who, "null params")
        for mw in (0, 65536, 0xFFFFFFFF):
            refused(call(busy, A.TsdfShiftParams((1, 0, 0), mw)), who, "min_weight")
        for fl in (1, 2, 0x80000000):
            refused(call(busy, A.TsdfShiftParams((1, 0, 0), 1, fl)), who, "unknown flag")
        for k in range(3):
            sp = A.TsdfShiftParams((-70000, -80000, -90000))
            sp.reserved_[k] = 1
            refused(call(busy, sp), who, "reserved")
        refused(call(busy, good, None, 1), who, "null points with a capacity")
        refused(call(idle, good), who, "no volume")
        refused(call(idle, A.TsdfShiftParams((0, 0, 0))), who, "no volume")
        for s in ((-65793, -65793, -65793), (-100000, -70000, -0x01010101), (-(1 << 25), -(1 << 25), -(1 << 25))):
            refused(call(busy, A.TsdfShiftParams(s)), who, "Match is pending")
            refused(call(busy, A.TsdfShiftParams(s, 65535), None, 0), who, "Match is pending")
    for bad in (4097, 4100, 4104):
        refused(L.adc_tsdf_shift_device(busy, C.byref(good), vp(bad), 8, None), "adc_tsdf_shift_device", "d_points must be 16-byte aligned")
    for bad in (4097, 4098, 4099):
        refused(L.adc_tsdf_shift_device(busy, C.byref(good), dev, 8, vp(bad)), "adc_tsdf_shift_device", "d_count must be 4-byte aligned")
    # the report, the offset
    refused(L.adc_get_tsdf_shift_report(None, C.byref(rep)), "adc_get_tsdf_shift_report", "null argument")
    refused(L.adc_get_tsdf_shift_report(idle, None), "adc_get_tsdf_shift_report", "null argument")
    refused(L.adc_get_tsdf_shift_report(idle, C.byref(rep)), "adc_get_tsdf_shift_report", "no shift call has completed")
    off, org = (C.c_int32 * 3)(), (C.c_float * 3)()
    refused(L.adc_tsdf_get_offset(None, off, org), "adc_tsdf_get_offset", "null argument")
    refused(L.adc_tsdf_get_offset(idle, None, None), "adc_tsdf_get_offset", "null argument")
    refused(L.adc_tsdf_get_offset(idle, off, org), "adc_tsdf_get_offset", "no volume")
    # the follow rule
    p, R, t, fp = c_params(T.params(8, 8, 8, 0.25, (0.0, 0.0, 0.0), 1.0)), (C.c_float * 9)(*T.IDENTITY), (C.c_float * 3)(), A.TsdfFollowParams()
    out = (C.c_int32 * 3)()
    assert L.adc_tsdf_follow_plan(C.byref(p), R, t, C.byref(fp), out) == 0
    for args in ((None, R, t, C.byref(fp), out), (C.byref(p), None, t, C.byref(fp), out), (C.byref(p), R, None, C.byref(fp), out), (C.byref(p), R, t, None, out),
                 (C.byref(p), R, t, C.byref(fp), None)):
        refused(L.adc_tsdf_follow_plan(*args), "adc_tsdf_follow_plan", "null argument")
    refused(L.adc_tsdf_follow_plan(C.byref(c_params(T.params(6, 8, 8, 0.25, (0.0, 0.0, 0.0), 1.0))), R, t, C.byref(fp), out), "adc_tsdf_follow_plan", "multiple of 4")
    for kw, why in ((dict(anchor=(float("nan"), 0, 0)), "anchor"), (dict(anchor=(0, float("inf"), 0)), "anchor"), (dict(margin=-1), "margin"), (dict(quantum=0), "quantum"),
                    (dict(quantum=-4), "quantum")):
        refused(L.adc_tsdf_follow_plan(C.byref(p), R, t, C.byref(A.TsdfFollowParams(**kw)), out), "adc_tsdf_follow_plan", why)
    bad = A.TsdfFollowParams()
    bad.reserved_[2] = 1
    refused(L.adc_tsdf_follow_plan(C.byref(p), R, t, C.byref(bad), out), "adc_tsdf_follow_plan", "reserved")
    refused(L.adc_tsdf_follow_plan(C.byref(p), (C.c_float * 9)(*([float("inf")] * 9)), t, C.byref(fp), out), "adc_tsdf_follow_plan", "R has a non-finite")
    refused(L.adc_tsdf_follow_plan(C.byref(p), R, (C.c_float * 3)(0, float("nan"), 0), C.byref(fp), out), "adc_tsdf_follow_plan", "t has a non-finite")
    with pytest.raises(ValueError):
        A.tsdf_follow_plan(p, T.IDENTITY, (0, 0, 0), A.TsdfFollowParams(quantum=0))


def test_offset_rule_on_a_block_of_ones():
    """the handle's offset words read 0x01010101 = 2^24 + 65793: already past the bound, so only a shift that brings an axis back is
    let through to the next check, and it must bring EVERY axis back"""
    L = A.lib()
    busy = C.cast(C.create_string_buffer(b"\x01" * (1 << 20), 1 << 20), C.c_void_p)
    back = -65793
    for s, through in (((back, back, back), True), ((back + 1, back, back), False), ((back, back, 0), False), ((1, 1, 1), False), ((back - (1 << 25), back, back), True),
                       ((back - (1 << 25) - 1, back, back), False), ((-(1 << 31), back, back), False)):
        rc = L.adc_tsdf_shift_device(busy, C.byref(A.TsdfShiftParams(s)), None, 0, None)
        assert rc == 1 and ("Match is pending" if through else "would pass 2^24") in A.last_error(), (s, A.last_error())


# ---------------------------------------------------------------------------------------------- the CLI on the stub, under sanitizers
def test_cli_tsdf_shift_under_sanitizers(tmp_path):
    """--tsdf-shift in the ASAN / UBSAN build of the CLI on the stub C ABI, whose shift is tsdf_shift.h run serially: the flag's parsing,
    the report line, <out>-tsdf-left.ply and <out>-tsdf.ply equal tests/tsdf_shift_ref.py on the volume tests/tsdf_ref.py fuses from the
    run's own .pfm; every other file of the run is byte-identical to a run without the flag."""
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
    spec = "32,24,32,0.03125,-0.625,-0.5,0.375,0.09375"
    p = T.params(32, 24, 32, 0.03125, (-0.625, -0.5, 0.375), 0.09375, flags=T.COLOR)

    def run(pref, *extra, rc=0):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "-3", "29", str(tmp_path / pref), *extra], env=SAN_ENV,
                           capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == rc, r.stdout
        return r.stdout

    for bad in ("", "1,2", "1,2,x", "1,2,3,0", "1,2,3,65536", "1,2,3,4,5", "16777217,0,0", "0,-16777217,0", "1,2,3x", "1.5,2,3"):
        assert "--tsdf-shift refused" in run("bad", "--tsdf", spec, *calib_arg, "--tsdf-shift", bad, rc=255), bad
    assert "--tsdf-shift refused: it needs --tsdf" in run("bad", *calib_arg, "--tsdf-shift", "1,0,0", rc=255)
    run("plain", "--tsdf", spec, *calib_arg)
    names = sorted(f[len("plain"):] for f in os.listdir(tmp_path) if (f.startswith("plain-") or f.startswith("plain.")) and not f.endswith("-tsdf.ply"))
    assert len(names) >= 4
    m = read_pfm(str(tmp_path / "plain.pfm"))
    vol, rep = T.integrate(T.empty(p), p, T.frame(calib), m, bgr)
    assert rep["updated"] > 500
    for pref, arg, s, mw in (("s1", "5,-3,2", (5, -3, 2), 1), ("s2", "-4,0,6,1", (-4, 0, 6), 1), ("s3", "0,0,0", (0, 0, 0), 1), ("s4", "0,24,0", (0, 24, 0), 1),
                             ("s5", "5,-3,2,2", (5, -3, 2), 2)):  # (one frame: no voxel has the weight 2, nothing is handed out)
        out = run(pref, "--tsdf", spec, *calib_arg, "--tsdf-shift", arg)
        for suffix in names:
            assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / pref) + suffix, "rb").read(), (pref, suffix)
        new, q, off, left, srep = SR.shift(vol, p, SR.shift_params(s, mw))
        pts, xrep = T.extract(new, q, 1)
        for got, want in ((read_tsdf_ply(str(tmp_path / pref) + "-tsdf-left.ply"), left), (read_tsdf_ply(str(tmp_path / pref) + "-tsdf.ply"), pts)):
            want = want.copy()
            want["pad"] = 0
            assert got.tobytes() == want.tobytes(), pref
        assert "TSDF shift %d,%d,%d: %u voxels moved, %u left, %u of them seen; %u leaving surface points\n" % (
            *s, srep["moved_nonempty"], srep["left_nonempty"], srep["left_seen"], srep["points"]) in out, out
        assert "%u voxels seen, %u surface points\n" % (xrep["voxels_seen"], xrep["points"]) in out, out
        assert (len(left) > 0) == (s != (0, 0, 0) and mw == 1) and (len(pts) == 0) == (pref == "s4"), (pref, len(left), len(pts))
    # the ray cast of the shifted volume reads the new origin
    run("r0", "--tsdf", spec, *calib_arg, "--tsdf-raycast", "40,30,35,20,15")
    run("r1", "--tsdf", spec, *calib_arg, "--tsdf-raycast", "40,30,35,20,15", "--tsdf-shift", "0,0,0")
    run("r2", "--tsdf", spec, *calib_arg, "--tsdf-raycast", "40,30,35,20,15", "--tsdf-shift", "6,0,0")
    ray = [open(str(tmp_path / n) + "-ray.pfm", "rb").read() for n in ("r0", "r1", "r2")]
    assert ray[0] == ray[1] != ray[2]
