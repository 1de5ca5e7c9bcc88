"""GPU tier: the set-up of the interpolation's table walk (k_itp_setup, k_refine.hip) -- one tile kernel that builds both passes' padded
code maps from one read of the disparity map and the labels.  The maps are read back through adc_debug_read_itp_code and compared, byte
for byte and padding included, with the maps tests/emul/emul_itp_code.cpp builds on the CPU map by map from the validity rule and
adc_itp_rowdist / adc_itp_coldist / adc_itp_skip of adc_device_fn.h; then the stage's result is compared with the oracle entered at
the interpolation.

A tile is 14 dwords (56 pixels) x 128 rows of the code map with a halo of 16 cells of 2 x 2 pixels; the shapes are 1 x 1, 3 x 2, less
than a tile, exactly one tile, and three tiles by three with the last one a single (cut) cell wide and high.  The range [-6, 10) and
[0, 15) pad the map by 10 and 15 columns on the left: the dwords then straddle the cells (gx & 3 = 2 and 3).

The same kernel clears the two list lengths in front of the list pass.  Every handle runs its maps one behind the other -- the empty map
(every pixel of a list a target) right in front of the full one (no target): list lengths left over from the run before would fill
valid pixels, which the comparison of the stage with the oracle shows."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from oracle.pyoracle import INTERP
from tests import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
VALID, OUTSIDE = 255, 254

SHAPES = ((1, 1), (3, 2), (41, 50), (52, 128), (113, 257))
RANGES = ((0, 16), (-6, 10), (0, 64), (0, 15))
CONTENTS = ("empty", "full", "corner", 0.01, 0.22, 0.78)


@pytest.fixture(scope="module")
def cpu_code_maps(tmp_path_factory):
    out_dir = os.path.join(ROOT, "tests", "emul", "_build")
    exe = os.path.join(out_dir, "emul_itp_code")
    deps = [os.path.join(ROOT, "tests", "emul", "emul_itp_code.cpp"), os.path.join(ROOT, "adcensus_amd", "csrc", "adc_device_fn.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", deps[0], "-o", exe])
    tmp = tmp_path_factory.mktemp("itp_code")

    def run(disp, label, ms):
        h, w = disp.shape
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([w, h, ms], np.int32).tobytes() + np.ascontiguousarray(disp, F).tobytes() + np.ascontiguousarray(label, np.uint8).tobytes())
        subprocess.check_call([exe, src, dst])
        pitch, rows = (w + 2 * ms + 8 + 3) & ~3, h + ms
        return np.fromfile(dst, np.uint8).reshape(2, rows, pitch)
    return run


@pytest.fixture(scope="module")
def oracle(ref_oracle, port_oracle):
    return pyoracle.stage_entry_oracle(ref_oracle, port_oracle)


def draw(content, w, h, seed):
    rng = np.random.default_rng(seed)
    values = (rng.integers(0, 14, (h, w)).astype(F) + rng.integers(0, 4, (h, w)).astype(F) / F(4)).astype(F)
    if content == "empty":
        valid = np.zeros((h, w), bool)
    elif content == "full":
        valid = np.ones((h, w), bool)
    elif content == "corner":
        valid = np.zeros((h, w), bool)
        valid[h - 1, w - 1] = True
    else:
        valid = rng.random((h, w)) < content
    disp = np.where(valid, values, INF).astype(F)
    label = rng.integers(0, 3, (h, w)).astype(np.uint8)
    img = (rng.integers(0, 8, (h, w, 3)) * 32).astype(np.uint8)
    return disp, label, img


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_code_maps_and_stage(hip, oracle, cpu_code_maps, shape):
    w, h = shape
    bad = []
    for dmin, dmax in RANGES:
        ms = max(abs(dmin), abs(dmax))
        opt = pyoracle.Option(min_disparity=dmin, max_disparity=dmax)
        st = hip.ADCensusStereo(device=0)
        assert st.Initialize(w, h, cases.to_product_option(opt)), hip.last_error()
        try:
            for n, content in enumerate(CONTENTS):
                disp, label, img = draw(content, w, h, seed=100 * w + 10 * ms + n)
                want_code = cpu_code_maps(disp, label, ms)
                want, _ = oracle.refine_from(INTERP, INTERP, disp, opt, left=img, label=label)
                st.debug_set_images(img, img)
                st.debug_write(hip.BUF_DISP_LEFT, disp)
                st.debug_write(hip.BUF_OUTLIER_LABEL, label)
                st.debug_run(hip.RUN_INTERPOLATION, 0)
                got = st.debug_read(hip.BUF_DISP_LEFT)
                for k in range(2):
                    code, gx = st.debug_read_itp_code(k)
                    assert gx == ms and code.shape == want_code[k].shape
                    diff = int((code != want_code[k]).sum())
                    if diff:
                        y, x = (int(v) for v in np.argwhere(code != want_code[k])[0])
                        bad.append("%dx%d [%d, %d) %s: code map %d differs in %d bytes, first (row %d, padded column %d) got %d want %d"
                                   % (w, h, dmin, dmax, content, k, diff, y, x, int(code[y, x]), int(want_code[k][y, x])))
                diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
                if diff:
                    bad.append("%dx%d [%d, %d) %s: the stage differs from the oracle on %d pixels" % (w, h, dmin, dmax, content, diff))
        finally:
            st.Release()
    assert not bad, bad[:10]


def test_the_corner_map_saturates(cpu_code_maps):
    """what the `corner` content is there for, on the CPU maps themselves: a pixel further than 16 cells from the only valid one carries the
    largest skip, 2 * 16 - 1 steps; one next to it carries none"""
    disp, label, _ = draw("corner", 113, 257, seed=1)
    code = cpu_code_maps(disp, label, 16)
    assert code[0, 0, 16] == 31 and code[0, 256, 16 + 112] == VALID and code[0, 256, 16 + 110] == 0 and code[0, 0, 15] == OUTSIDE
