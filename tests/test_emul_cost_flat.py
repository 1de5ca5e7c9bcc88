"""CPU tier: the element-wise first aggregation pass of the short-arm plan (k_cost_agg_flat, k_cost.hip).  The per-pixel arithmetic is
the device's own header (adcensus_amd/csrc/k_cost_flat.h, compiled under g++ by tests/emul/emul_cost_flat.cpp, which restates the
kernel's walk around it); its volume must equal, bit for bit, the definition of that pass built from the port oracle's dumps: per
element the sequential f32 sum from 0.0f over the pixel's clipped horizontal span t = -arm_left .. +arm_right of cost_init(x + t, y, d)
(cross_aggregator.cpp:327-394 over cost_computor.cpp:82-121), and 0.0f in the padding lanes d >= D."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases, gather_patterns
from tests.test_gpu_sparse_agg import planted_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emul_flat():
    out_dir = os.path.join(ROOT, "tests", "emul", "_build")
    so = os.path.join(out_dir, "libadcensus_emul_cost_flat.so")
    deps = [os.path.join(ROOT, "tests", "emul", "emul_cost_flat.cpp"), os.path.join(ROOT, "adcensus_amd", "csrc", "k_cost_flat.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", deps[0], "-o", so])
    lib = C.CDLL(so)
    lib.emul_cost_flat_launch.restype = C.c_int
    return lib


def P(a):
    return a.ctypes.data_as(C.c_void_p)


PAIRS = {
    "n2w": lambda: cases.OPT_PAIRS["n2w"][0](),
    "s2": lambda: cases.OPT_PAIRS["s2"][0](),
    "s2w": lambda: cases.OPT_PAIRS["s2w"][0](),
    "flat": lambda: cases.OPT_PAIRS["flat"][0](),
    "planted": lambda: planted_pair(64, 48, seed=9810),
    "runs_2_5": lambda: gather_patterns.run_pair(67, 45, seed=9820, lengths=(2, 3, 4, 5)),
    "ends": lambda: end_runs_pair(131, 24, seed=9830),  # a tile remainder of 3 pixels; arms 1..4 at x = 0 and at x = W - 1
}
# (min_disparity, disparity range): a negative and a positive offset, padding lanes (100 of 128), two 128-float chunks
RANGES = {"m10_128": (-10, 128), "0_100": (0, 100), "p5_256": (5, 256)}


def end_runs_pair(w, h, seed):
    """Noise pair with runs of 2..5 equal pixels that start in the first and that end in the last pixel of a row."""
    left, right = (a.copy() for a in workloads.noise_pair(w, h, seed=seed))
    for j, n in enumerate((2, 3, 4, 5)):
        left[2 + 5 * j, 0:n] = left[2 + 5 * j, 0]
        left[4 + 5 * j, w - n:w] = left[4 + 5 * j, w - 1]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def span_sums(cost, arms, dp):
    """The definition: [H][W][dp] f32, sequential sums in the order t = -left .. +right from +0.0f; padding lanes 0.0f."""
    h, w, d = cost.shape
    xs = np.arange(w)[None, :]
    lo = np.minimum(arms[..., 0].astype(np.int64), xs)
    hi = np.minimum(arms[..., 1].astype(np.int64), w - 1 - xs)
    acc = np.zeros((h, w, d), np.float32)
    for t in range(-int(lo.max()), int(hi.max()) + 1):
        take = (t >= -lo) & (t <= hi)  # (the clipped span keeps x + t inside the row)
        ys, xx = np.nonzero(take)
        acc[ys, xx] = acc[ys, xx] + cost[ys, xx + t]
    out = np.zeros((h, w, dp), np.float32)
    out[..., :d] = acc
    return out


@pytest.mark.parametrize("rng_name", sorted(RANGES))
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_flat_first_pass_equals_the_definition(emul_flat, port_oracle, pair, rng_name):
    left, right = PAIRS[pair]()
    dmin, d = RANGES[rng_name]
    h, w = left.shape[:2]
    dp = (d + 127) // 128 * 128
    # columns whose right pixel lies left of the image, and (negative offset) right of it
    assert 0 - dmin < 0 or d > 1 - dmin, "some x - disparity < 0"
    assert dmin >= 0 or (w - 1) - dmin >= w, "some x - disparity >= W"
    opt = pyoracle.Option(min_disparity=dmin, max_disparity=dmin + d)
    o = port_oracle.run(left, right, opt, stages=["census_left", "census_right", "cost_init", "arms"])
    arms = o["arms"]
    ah = gather_patterns.arm_maxima(arms)[0]
    if pair in ("planted", "runs_2_5", "ends"):
        assert 1 <= ah <= 4, ah
        assert arms[:, 0, 1].max() >= 1 and arms[:, w - 1, 0].max() >= 1  # spans that start / end with the row
    if pair == "ends":
        assert {1, 2, 3, 4} <= set(np.unique(arms[:, 0, 1]).tolist()) and {1, 2, 3, 4} <= set(np.unique(arms[:, w - 1, 0]).tolist())
    want = span_sums(o["cost_init"], arms, dp)
    if dmin > 0:
        assert (o["cost_init"][:, :dmin, 0] == 1.0).all()  # (out-of-image marker: cost 1)
    if dmin < 0:
        assert (o["cost_init"][:, w + dmin:, 0] == 1.0).all()
    left = np.ascontiguousarray(left)
    right = np.ascontiguousarray(right)
    for cap in sorted({max(1, ah), max(1, ah) + 1}):  # the depth known exactly, and assumed with a margin
        got = np.full((h, w, dp), np.nan, np.float32)
        rc = emul_flat.emul_cost_flat_launch(P(got), P(left), P(right), P(o["census_left"]), P(o["census_right"]), P(arms), w, h, dmin, d, dp,
                                             cap, opt.lambda_ad, opt.lambda_census)
        assert rc == 0, rc
        bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        assert bad == 0, (cap, bad)
