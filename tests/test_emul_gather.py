"""CPU tier: the gather form of the sparse small-ring aggregation launches (k_agg_gather + k_agg_apply).  The per-pixel arithmetic is
the device's own header (adcensus_amd/csrc/k_agg_gather.h, compiled under g++ by tests/emul/emul_gather.cpp); the eight passes
H V V H H V V H of the aggregation, run as gather launches on the port oracle's arms, support counts and cost volume, must give the
oracle's aggregated volume bit for bit -- with the three pass pairs as pair launches (the production sequence), and with every
pass as a launch of its own (non-dividing and dividing single form)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests import gather_patterns
from tests.test_gpu_sparse_agg import planted_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emul_gather():
    out_dir = os.path.join(ROOT, "tests", "emul", "_build")
    so = os.path.join(out_dir, "libadcensus_emul_gather.so")
    deps = [os.path.join(ROOT, "tests", "emul", "emul_gather.cpp"), os.path.join(ROOT, "adcensus_amd", "csrc", "adc_device_fn.h"),
            os.path.join(ROOT, "adcensus_amd", "csrc", "k_agg_gather.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", deps[0], "-o", so])
    lib = C.CDLL(so)
    lib.emul_gather_launch.restype = C.c_long
    return lib


def P(a):
    return a.ctypes.data_as(C.c_void_p)


CASES = {
    "noise": lambda: workloads.noise_pair(64, 48, seed=9700) + (16,),
    "noise_odd": lambda: workloads.noise_pair(67, 45, seed=9701) + (32,),
    "planted": lambda: planted_pair(64, 48, seed=9710) + (24,),      # runs at the image border, spans that overlap each other
    "planted_tall": lambda: planted_pair(50, 71, seed=9711) + (16,),
    "runs_6_9": lambda: gather_patterns.run_pair(64, 48, seed=9720) + (32,),  # arms up to 8 in both directions
    "runs_6_9_odd": lambda: gather_patterns.run_pair(61, 50, seed=9721) + (16,),
}


@pytest.fixture(scope="module")
def dumps(port_oracle):
    cache = {}

    def get(name):
        if name not in cache:
            left, right, d = CASES[name]()
            o = port_oracle.run(left, right, pyoracle.Option(max_disparity=d), stages=["arms", "sup_count_h", "sup_count_v", "cost_init", "cost_aggr"])
            cache[name] = (left.shape[1], left.shape[0], d, o)
        return cache[name]
    return get


def _differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


@pytest.mark.parametrize("name", sorted(CASES))
def test_gather_launches_equal_the_oracle(emul_gather, dumps, name):
    w, h, d, o = dumps(name)
    ah, av = gather_patterns.arm_maxima(o["arms"])
    if name.startswith("runs"):
        assert 5 <= ah <= 8 and 5 <= av <= 8 and max(ah, av) == 8, (ah, av)  # the case is what it is meant to be
    sup_h, sup_v = o["sup_count_h"], o["sup_count_v"]  # divisor of the dividing V pass (H-first iterations) / of the dividing H pass

    def launch(vol, vert, divide, pair):
        other = np.empty_like(vol)
        n = emul_gather.emul_gather_launch(P(vol), P(other), P(o["arms"]), P(sup_h if vert else sup_v), w, h, d, vert, divide, pair)
        assert n > 0
        return n

    # production sequence of the short-arm plan: H | V+V | H+H | V+V | H (the last one dividing)
    vol = o["cost_init"].copy()
    launch(vol, 0, 0, 0)
    for vert in (1, 0, 1):
        launch(vol, vert, 1, 1)
    launch(vol, 0, 1, 0)
    assert _differing(vol, o["cost_aggr"]) == 0
    # every pass a launch of its own: H | V/ | V | H/ | H | V/ | V | H/
    vol = o["cost_init"].copy()
    launch(vol, 0, 0, 0)
    for vert, divide in ((1, 1), (1, 0), (0, 1), (0, 0), (1, 1), (1, 0), (0, 1)):
        launch(vol, vert, divide, 0)
    assert _differing(vol, o["cost_aggr"]) == 0
