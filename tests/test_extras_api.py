"""CPU tier: the provenance / confidence surface of the C ABI (adc_match_ex, adc_match_device_ex) -- declared, exported, the same
constants in the header and in the Python mirror, the NULL-handle contract -- and the rules of tests/extras_ref.py on hand-made
cost vectors (the definition the GPU tests compare the kernels with)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import adcensus_amd as A
from tests import extras_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adcensus_c_api.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_and_library_exports_the_entry_points():
    text = _header()
    assert re.search(r"int\s+adc_match_ex\s*\(\s*adc_handle\s*\*", text)
    assert re.search(r"int\s+adc_match_device_ex\s*\(\s*adc_handle\s*\*", text)
    out = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"adc_match_ex", "adc_match_device_ex"} <= names


def test_constants_agree_with_the_python_mirror():
    consts = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define\s+ADC_((?:LR|FILL|PROV)_\w+)\s+(\d+)", _header()))
    assert set(consts) == {"LR_CONSISTENT", "LR_MISMATCH", "LR_OCCLUSION", "FILL_WTA", "FILL_VOTING", "FILL_INTERPOLATION",
                           "FILL_NONE", "PROV_LR_MASK", "PROV_FILL_SHIFT"}
    for name, value in consts.items():
        assert getattr(A, name) == value, name
    assert (extras_ref.LR_MASK, extras_ref.FILL_SHIFT) == (A.PROV_LR_MASK, A.PROV_FILL_SHIFT)
    assert (extras_ref.FILL_WTA, extras_ref.FILL_VOTING, extras_ref.FILL_INTERPOLATION, extras_ref.FILL_NONE) == \
        (A.FILL_WTA, A.FILL_VOTING, A.FILL_INTERPOLATION, A.FILL_NONE)


def test_null_handle_is_refused():
    L = A.lib()
    img = np.zeros(12, np.uint8)
    disp = np.zeros(4, np.float32)
    prov = np.zeros(4, np.uint8)
    conf = np.zeros(4, np.float32)
    assert L.adc_match_ex(None, img.ctypes.data, img.ctypes.data, disp.ctypes.data, prov.ctypes.data, conf.ctypes.data) == 1
    assert L.adc_match_ex(None, img.ctypes.data, img.ctypes.data, disp.ctypes.data, None, None) == 1
    assert L.adc_match_device_ex(None, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), None) == 1
    st = A.ADCensusStereo()
    assert st.MatchEx(img, img, disp, prov, conf) is False  # (not initialised)


def _conf(costs):
    return extras_ref.confidence_from_costs(np.asarray(costs, np.float32)[None, :])[0]


def test_confidence_rules():
    f = np.float32
    # the first minimum: equal costs at d = 1 and 2 -> d1 = 1, so d = 2 is excluded and d = 3 holds c2
    assert _conf([3, 1, 1, 5]) == (f(5) - f(1)) / f(5)
    # another disparity two steps away ties with the minimum -> 0
    assert _conf([1, 5, 1]) == 0
    # neighbours of d1 never count, whatever they cost
    assert _conf([9, 0.5, 4, 0.5, 7]) == (f(0.5) - f(0.5)) / f(0.5) == 0
    assert _conf([9, 7, 0.5, 0.25, 8, 6]) == (f(6) - f(0.25)) / f(6)
    # empty set for c2 (D = 3, d1 = 1) -> 1; D = 3 with d1 at an end has a c2
    assert _conf([5, 1, 5]) == 1
    assert _conf([1, 5, 3]) == (f(3) - f(1)) / f(3)
    # c2 == 0 -> 0 (no 0 / 0)
    assert _conf([0, 3, 0]) == 0
    # f32 arithmetic, correctly rounded: one ulp apart
    a = f(1.0) + np.spacing(f(1.0))
    assert _conf([1.0, 9.0, a]).view(np.uint32) == ((a - f(1.0)) / a).view(np.uint32)
    # fill != 0 -> 0; arrays of pixels, values in [0, 1]
    rng = np.random.default_rng(3)
    cost = rng.random((7, 9, 40), dtype=np.float32) * 10
    fill = rng.integers(0, 4, (7, 9))
    conf = extras_ref.confidence_from_costs(cost, fill)
    assert conf.dtype == np.float32 and conf.shape == (7, 9)
    assert np.all(conf[fill != 0] == 0) and np.all((conf >= 0) & (conf <= 1))
    ref = extras_ref.confidence_from_costs(cost)
    assert np.array_equal(conf[fill == 0].view(np.uint32), ref[fill == 0].view(np.uint32))


def test_provenance_rules():
    from oracle import pyoracle
    inf = np.inf
    o = {"disp_left_wta": np.array([[3.0, inf, 2.5, inf, 1.0]], np.float32),
         "outlier_label": np.array([[0, 1, 2, 1, 2]], np.uint8),
         "disp_after_irv": np.array([[3.0, 4.0, inf, inf, 2.0]], np.float32)}
    assert extras_ref.provenance(o, pyoracle.Option()).tolist() == [[0, 1 | 1 << 2, 2 | 2 << 2, 1 | 2 << 2, 2 | 1 << 2]]
    assert extras_ref.provenance(o, pyoracle.Option(do_filling=0)).tolist() == [[0, 1 | 12, 2 | 12, 1 | 12, 2 | 12]]
    # no LR check: lr = 0 everywhere, a +inf winner-takes-all result has code 12
    assert extras_ref.provenance(o, pyoracle.Option(do_lr_check=0)).tolist() == [[0, 12, 0, 12, 0]]
