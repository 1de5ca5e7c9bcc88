"""CPU tier of the speckle filter: tests/speckle_ref.py (the definition the GPU tests hold the kernels to) against a brute-force
search on random and hand-built maps, the figures of the reference's own maps, and the new surface of the C ABI, the Python mirror,
the facade and the CLI -- declared, exported, NULL-handle / bad-argument returns, and a malformed --speckle refused before a device
is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import adcensus_amd as A
from tests import cases
from tests.speckle_patterns import patterns
from tests.speckle_ref import largest, speckle_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")
ENTRY_POINTS = ["adc_set_speckle_filter", "adc_filter_speckles_device", "adc_get_speckle_stats"]
F = np.float32
INF = F(np.inf)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def brute_force(disp, max_size, max_diff):
    """The definition word for word: a breadth-first search from every unlabelled valid pixel in raster order."""
    d = np.ascontiguousarray(disp, F)
    h, w = d.shape
    md = F(max_diff)
    labels = np.full((h, w), -1, np.int32)
    out = d.copy()
    comps = removed_c = removed_p = 0
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if not np.isfinite(d[y, x]) or labels[y, x] >= 0:
                    continue
                comps += 1
                labels[y, x] = y * w + x
                todo, members = [(y, x)], [(y, x)]
                while todo:
                    cy, cx = todo.pop()
                    for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                        if 0 <= ny < h and 0 <= nx < w and labels[ny, nx] < 0 and np.isfinite(d[ny, nx]) and \
                                np.abs(F(d[cy, cx] - d[ny, nx])) <= md:
                            labels[ny, nx] = y * w + x
                            todo.append((ny, nx))
                            members.append((ny, nx))
                if max_size > 0 and len(members) <= max_size:
                    removed_c += 1
                    removed_p += len(members)
                    for my, mx in members:
                        out[my, mx] = INF
    return out, labels, (comps, removed_c, removed_p)


def _same_result(got, want, what):
    assert np.array_equal(_u32(got[0]), _u32(want[0])), what + ": map"
    assert np.array_equal(got[1], want[1]), what + ": labels"
    assert got[2] == want[2], (what, got[2], want[2])


def test_reference_against_brute_force_on_random_maps():
    rng = np.random.default_rng(2024)
    for t in range(40):
        h, w = int(rng.integers(1, 24)), int(rng.integers(1, 90))
        d = (np.round(rng.random((h, w)) * float(rng.choice([2, 4, 8]))) * 0.5).astype(F)
        d[rng.random((h, w)) < float(rng.choice([0, 0.1, 0.4]))] = INF
        d[rng.random((h, w)) < 0.03] = np.nan
        d[rng.random((h, w)) < 0.03] = -np.inf
        d[rng.random((h, w)) < 0.1] *= F(-1)  # negative values and -0.0
        max_size = int(rng.choice([0, 1, 3, 10, 100, h * w]))
        max_diff = float(rng.choice([0.0, 0.5, 1.0]))
        got, want = speckle_ref(d, max_size, max_diff), brute_force(d, max_size, max_diff)
        _same_result(got, want, "random map %d (%dx%d, %d, %g)" % (t, w, h, max_size, max_diff))
        untouched = ~np.isfinite(d)
        assert np.array_equal(_u32(got[0])[untouched], _u32(d)[untouched])  # NaN / -inf / +inf keep their bits


@pytest.mark.parametrize("size", [(70, 13), (9, 31), (130, 3), (1, 17), (66, 1)])
def test_reference_against_brute_force_on_the_patterns(size):
    w, h = size
    for name, (d, max_size, max_diff) in patterns(w, h).items():
        _same_result(speckle_ref(d, max_size, max_diff), brute_force(d, max_size, max_diff), "%s %dx%d" % (name, w, h))


def test_the_patterns_mean_what_they_say():
    w, h = 70, 13
    p = patterns(w, h)
    comps = {k: speckle_ref(*v)[2] for k, v in p.items()}
    assert comps["constant"] == (1, 0, 0) and comps["all_invalid"] == (0, 0, 0)
    assert comps["serpentine"] == (1, 0, 0) and comps["serpentine_removed"] == (1, 1, w * h)
    assert comps["spiral"][0] == 1 and comps["comb"][0] == 1
    assert comps["checker_valid_invalid"] == ((w * h + 1) // 2,) * 3 and comps["checker_two_disparities"] == (w * h,) * 3
    assert comps["ramp_le_edge"] == (1, 0, 0)                    # steps of exactly max_diff join (<=)
    assert comps["ramp_below_edge"] == (w, w, w * h)             # one ulp less: columns, each of size h == max_size, removed (<=)
    assert comps["ramp_below_edge_kept"] == (w, 0, 0)            # max_size + 1 pixels: kept
    assert comps["ramp_offset_rows"] == (w * h, w * h, w * h)
    c, rc, rp = comps["blocks"]
    assert c == 2 * rc and rp == 12 * rc and rc > 0              # the 12-pixel blocks go, the 13-pixel ones stay
    # a smooth ramp is one component however far its ends are apart; signs are kept; -0.0 == +0.0
    assert speckle_ref(np.arange(50, dtype=F).reshape(1, 50), 10, 1.0)[2] == (1, 0, 0)
    assert speckle_ref(np.array([[-1.0, 1.0]], F), 1, 1.0)[2] == (2, 2, 2)
    assert speckle_ref(np.array([[-0.0, 0.0]], F), 1, 0.0)[2] == (1, 0, 0)


# valid px | (100, 1.0): components, removed components, removed px, largest | (400, 1.0): removed px | (50, 0.5): components, removed px
TABLE = {
    "q_9x20_d8": (180, (6, 5, 79, 101), 180, (9, 80)),
    "noise_160x90_d128": (14400, (809, 789, 6287, 2645), 9479, (1103, 6688)),
    "s2_320x180_d128": (57600, (9, 3, 24, 52094), 24, (19, 90)),
}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_figures_on_the_reference_maps(port_oracle, name):
    """The filter bites on the reference's own final maps, and both outcomes occur (components removed, components kept)."""
    left, right, opt = cases.make_case(name)
    d = port_oracle.run(left, right, opt, stages=["disp_final"])["disp_final"]
    valid, a, b, c = TABLE[name]
    out, labels, st = speckle_ref(d, 100, 1.0)
    print(name, "valid", int(np.isfinite(d).sum()), "(100, 1.0):", st, "largest", largest(labels))
    assert int(np.isfinite(d).sum()) == valid
    assert st + (largest(labels),) == a
    assert int(np.isinf(out).sum() - np.isinf(d).sum()) == st[2]
    assert speckle_ref(d, 400, 1.0)[2][2] == b
    st50 = speckle_ref(d, 50, 0.5)[2]
    assert (st50[0], st50[2]) == c
    # idempotent on a whole map: removing a component changes no other one
    again = speckle_ref(out, 100, 1.0)
    assert np.array_equal(_u32(again[0]), _u32(out)) and again[2][1:] == (0, 0)


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"int\s+%s\s*\(\s*adc_handle\s*\*" % name, text), name
    assert re.search(r"int\s+adc_farm_set_speckle_filter\s*\(\s*adc_farm\s*\*", text)
    assert re.search(r"#define\s+ADC_PROV_SPECKLE\s+\(0x10\)", text) and A.PROV_SPECKLE == 0x10
    assert A.PROV_SPECKLE & ((A.PROV_LR_MASK) | (3 << A.PROV_FILL_SHIFT)) == 0  # above the four bits in use
    out = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS + ["adc_farm_set_speckle_filter"]) <= names


def test_null_handle_and_bad_arguments_are_refused():
    L = A.lib()
    assert L.adc_set_speckle_filter(None, 100, 1.0) == 1
    assert L.adc_filter_speckles_device(None, C.c_void_p(16), 100, 1.0, None) == 1
    assert L.adc_farm_set_speckle_filter(None, 100, 1.0) == 1
    a, b, c = C.c_uint32(7), C.c_uint32(8), C.c_uint32(9)
    assert L.adc_get_speckle_stats(None, C.byref(a), C.byref(b), C.byref(c)) == 1 and (a.value, b.value, c.value) == (7, 8, 9)
    st = A.ADCensusStereo()  # (not initialised: a NULL handle underneath)
    with pytest.raises(RuntimeError):
        st.set_speckle_filter(100, 1.0)
    assert st.filter_speckles_device(16, 100, 1.0) is False
    with pytest.raises(RuntimeError):
        st.speckle_stats()


def test_python_mirror_signatures():
    def params(f):
        return list(inspect.signature(f).parameters)
    assert params(A.ADCensusStereo.set_speckle_filter) == ["self", "max_size", "max_diff"]
    assert params(A.ADCensusStereo.filter_speckles_device) == ["self", "d_disp", "max_size", "max_diff", "d_labels"]
    assert params(A.ADCensusStereo.filter_speckles) == ["self", "disp", "max_size", "max_diff", "labels"]
    assert inspect.signature(A.ADCensusStereo.filter_speckles).parameters["labels"].default is False
    assert params(A.ADCensusStereo.speckle_stats) == ["self"]
    assert params(A.PairFarm.set_speckle_filter) == ["self", "max_size", "max_diff"]
    L = A.lib()
    assert L.adc_set_speckle_filter.argtypes == [C.c_void_p, C.c_int32, C.c_float]
    assert L.adc_filter_speckles_device.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p]


def test_facade_compiles_and_exports_the_setter(tmp_path):
    """A caller of the facade's new member compiles against include/ alone and links against the facade library; the reference's
    own caller still does (tests/test_reference_caller.py checks main.cpp itself)."""
    src = tmp_path / "caller.cpp"
    src.write_text('#include "ADCensusStereo.h"\n'
                   'int main() { ADCensusStereo s; ADCensusOption o; bool a = s.SetSpeckleFilter(100, 1.0f); bool b = s.SetSpeckleFilter(5, -1.0f);\n'
                   '  float32 d[4]; uint8 i[12] = {0}; return (a && !b && !s.Match(i, i, d) && !s.Initialize(0, 0, o)) ? 0 : 1; }\n')
    libdir = os.path.join(ROOT, "adcensus_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libadcensus.so")):
        pytest.fail("libadcensus.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "caller"),
                    "-L", libdir, "-ladcensus", "-ladcensus_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(libdir, "libadcensus.so")], capture_output=True, text=True, check=True).stdout
    assert "ADCensusStereo::SetSpeckleFilter(int, float)" in out
    # before Initialize the setter only checks and remembers; no device is needed to run this
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


def test_cli_rejects_a_malformed_speckle_flag(tmp_path):
    """Checked while the arguments are parsed: the images named here do not even exist."""
    cli = os.path.join(ROOT, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    for bad in (["--speckle"], ["--speckle", "100"], ["--speckle", "100,"], ["--speckle", "abc,1"], ["--speckle", "0,1.0"], ["--speckle", "-5,1.0"],
                ["--speckle", "100,-1"], ["--speckle", "100,nan"], ["--speckle", "100,inf"], ["--speckle", "100,1.0,7"], ["--speckle", "100,1.0x"]):
        r = subprocess.run([cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "0", "64", str(tmp_path / "out")] + bad,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--speckle needs SIZE,DIFF" in r.stdout and "Image Loading" not in r.stdout, (bad, r.stdout)
    r = subprocess.run([cli, str(tmp_path / "no_left.png"), str(tmp_path / "no_right.png"), "--speckle", "100,1.0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Image Loading" in r.stdout and "--speckle needs" not in r.stdout  # (a well-formed flag gets as far as the images)


def test_cli_speckle_under_sanitizers(tmp_path):
    """The flag's parsing and the facade's setter in the ASAN / UBSAN build on the stub C ABI (which checks the arguments and filters
    nothing): a run with the flag completes, and its files equal a run without it there."""
    from PIL import Image
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "adcensus_amd", "host"), "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cli = os.path.join(ROOT, "adcensus_amd", "build", "asan", "adcensus_cli_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    rgb = np.random.default_rng(5).integers(0, 256, (31, 45, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "l.png")
    Image.fromarray(rgb[:, ::-1].copy()).save(tmp_path / "r.png")

    def run(*extra):
        r = subprocess.run([cli, str(tmp_path / "l.png"), str(tmp_path / "r.png"), "0", "16", *extra], env=env, capture_output=True, text=True, timeout=300)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        return r

    assert run(str(tmp_path / "plain")).returncode == 0
    assert run("--speckle", "100,1.5", str(tmp_path / "spk")).returncode == 0
    assert run(str(tmp_path / "spk2"), "--speckle", "7,0", "--calib", "100,0.5,0,0,0").returncode == 0
    for suffix in ("-d.png", "-c.png", "-cloud.txt", ".pfm"):
        assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / "spk") + suffix, "rb").read(), suffix
    assert run(str(tmp_path / "bad"), "--speckle", "7,-2").returncode != 0 and not os.path.exists(str(tmp_path / "bad") + ".pfm")
