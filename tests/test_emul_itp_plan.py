"""CPU tier: the interpolation's plan (adcensus_amd/csrc/itp_plan.h, compiled alone under g++ by tests/emul/emul_itp_plan.cpp) --
the ONE predicate that says whether a handle walks the integer ray table, and the bytes adc_create allocates for the stage.
The byte counts are restated here from the layout (k_refine.hip before the header existed: two sets of three cell maps, 16-byte
aligned, then two padded code maps of pitch x rows + 64 bytes each, 16-byte aligned, + 64)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan():
    out_dir = os.path.join(ROOT, "tests", "emul", "_build")
    exe = os.path.join(out_dir, "emul_itp_plan")
    deps = [os.path.join(ROOT, "tests", "emul", "emul_itp_plan.cpp"), os.path.join(ROOT, "adcensus_amd", "csrc", "itp_plan.h"),
            os.path.join(ROOT, "adcensus_amd", "csrc", "adc_device_fn.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", deps[0], "-o", exe])

    def run(*triples):
        args = [str(v) for t in triples for v in t]
        lines = subprocess.check_output([exe] + args, text=True).splitlines()
        rows = [tuple(int(v) for v in l.split()) for l in lines[:-1]]
        return [dict(ok=bool(r[3]), alloc=r[4], cells=r[5], pitch=r[6], rows=r[7]) for r in rows], lines[-1]
    return run


def cell_maps(w, h):
    return ((2 * 3 * ((w + 1) // 2) * ((h + 1) // 2) + 15) & ~15) + 64


def with_code_maps(w, h, ms):
    pitch, rows = (w + 2 * ms + 8 + 3) & ~3, h + ms
    return ((2 * 3 * ((w + 1) // 2) * ((h + 1) // 2) + 15) & ~15) + 2 * ((pitch * rows + 64 + 15) & ~15) + 64


def test_predicate_edges(plan):
    r, _ = plan((4094, 3, 2047), (4095, 3, 2047), (64, 32, 30001), (4094, 2048, 2047))
    assert [x["ok"] for x in r] == [True, False, False, True]
    assert r[0]["pitch"] == 8196 and 2047 * r[0]["pitch"] == (1 << 24) - 4 and 2047 * r[1]["pitch"] >= 1 << 24
    # The search-range limit of 30000 (upload_tables' condition) never decides on its own: the pitch is at least 2 * ms + 9, so
    # ms * pitch < 2^24 already ends the table walk at ms = 2893 at the latest, whatever the width.  (64, 32, 30000) is therefore FALSE under
    # the conditions the launch has always tested -- the f64 walk ran there before this header existed, and runs there now; at
    # W = 64 the last search range on the table walk is 2878 (pitch 5828: 16 772 984 < 2^24).
    r, _ = plan((64, 32, 30000), (64, 32, 2878), (64, 32, 2879), (1, 1, 2893), (1, 1, 2894))
    assert [x["ok"] for x in r] == [False, True, False, True, False]
    # the other conditions: image sides below 2^20, a search range of at least 1
    r, _ = plan((1, 1, 1), (1, 1, 0), (0, 5, 9), ((1 << 20) - 1, 1, 1), (1 << 20, 1, 1), (1, 1 << 20, 1))
    assert [x["ok"] for x in r] == [True, False, False, True, False, False]


def test_pitch_times_rows_limit_on_both_sides(plan):
    """32-bit positions in the padded map: pitch * rows < 2^31.  ms = 15 (pitch = W + 38 rounded down to a multiple of 4) keeps ms * pitch far
    below 2^24; with H = 2^20 - 1 rows = 1048590, and 2^31 / 1048590 = 2047.97: pitch 2044 passes, 2048 does not."""
    r, _ = plan((2006, (1 << 20) - 1, 15), (2010, (1 << 20) - 1, 15))
    assert (r[0]["pitch"], r[1]["pitch"]) == (2044, 2048) and r[0]["rows"] == r[1]["rows"] == 1048590
    assert r[0]["pitch"] * r[0]["rows"] < 1 << 31 <= r[1]["pitch"] * r[1]["rows"]
    assert 15 * r[1]["pitch"] < 1 << 24
    assert [x["ok"] for x in r] == [True, False]


def test_byte_counts(plan):
    r, _ = plan((64, 32, 30001), (64, 32, 2878), (4094, 3, 2047), (4095, 3, 2047), (157, 83, 96), (1, 1, 9), (1920, 1080, 64))
    assert r[0]["alloc"] == r[0]["cells"] == cell_maps(64, 32)  # no table walk: the cell maps alone (the code maps would be 3.6 GB)
    assert r[3]["alloc"] == cell_maps(4095, 3)
    for x, (w, h, ms) in zip((r[1], r[2], r[4], r[5], r[6]), ((64, 32, 2878), (4094, 3, 2047), (157, 83, 96), (1, 1, 9), (1920, 1080, 64))):
        assert x["ok"] and x["alloc"] == with_code_maps(w, h, ms), (w, h, ms)
    assert with_code_maps(64, 32, 30001) > 3.6e9 > 1000 * r[0]["alloc"]


def test_search_range(plan):
    _, last = plan((1, 1, 1))
    assert last == "max_search 64 70 2147483648"
