"""GPU tier: every Match entry point is a view of one request.  Each older entry point (adc_match_ex, adc_match_out, adc_match_device_ex,
adc_match_device_out) against its adc_*_products twin, on one handle and with the same request: the map, every product, the cloud
count and the points are byte-identical, and on the fault-injection build both make the same number of HIP calls.  That the bytes are
the RIGHT ones is pinned by tests/test_gpu_extras.py, test_gpu_outputs.py and test_gpu_products.py against the oracle.  Every output
buffer is poisoned (0xA5) first."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests.test_gpu_outputs import DeviceBuffers, _handle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
F = np.float32
W, H, D = 128, 80, 32  # the pair of tests/products_fault_probe.py: every product and the cloud scan's tile logic are live
N = W * H
CALIB = (3740.0, 0.16, 64.0, 40.0, 0.5)  # doffs > 0: every finite pixel is a point
GUARD = 8  # poisoned points behind the cloud's capacity


def _poison(n, dtype):
    return np.frombuffer(bytearray([POISON]) * (n * np.dtype(dtype).itemsize), dtype)


class HostSet:
    """poisoned host destinations of one call: the map, the four maps the older generations know, a cloud of `cap` points + GUARD"""

    def __init__(self, A, cap, inside=None):
        sizes = (("disp", F, N), ("prov", np.uint8, N), ("conf", F, N), ("depth", F, N), ("disp8", np.uint8, N), ("cloud", A.POINT_DTYPE, cap + GUARD))
        at = 0 if inside is None else (-inside.ctypes.data) % 64
        for name, dt, count in sizes:
            nbytes = count * np.dtype(dt).itemsize
            a = _poison(count, dt) if inside is None else inside[at:at + nbytes].view(dt)
            at += (nbytes + 63) // 64 * 64
            setattr(self, name, a if name == "cloud" else a.reshape(H, W))
        self.cap = cap
        self.count = None

    def snapshot(self, which):
        return {k: getattr(self, k).tobytes() for k in which}, self.count


class DeviceSet:
    """the same in device memory"""

    def __init__(self, A, dev, cap):
        self.dev, self.cap, self.A = dev, cap, A
        self.sizes = dict(disp=4 * N, prov=N, conf=4 * N, depth=4 * N, disp8=N, cloud=16 * (cap + GUARD), word=16)
        self.p = {k: dev.alloc(v) for k, v in self.sizes.items()}

    def poison(self):
        for k, v in self.sizes.items():
            self.dev.put(self.p[k], np.full(v, POISON, np.uint8))

    def snapshot(self, which, count):
        return {k: self.dev.get(self.p[k], self.sizes[k], np.uint8).tobytes() for k in which}, (count, int(self.dev.get(self.p["word"], 1, np.uint32)[0]))


EX, OUT = ("disp", "prov", "conf"), ("disp", "depth", "disp8", "cloud")


@pytest.mark.parametrize("mode", ["plain", "speckle", "budget"])
def test_older_entry_points_equal_their_products_twins(hip, mode):
    """plain handle; speckle filter (50, 1.0) set; voting budget forced to 4 kernels before every Match, so that adc_wait continues
    the chain and delivers again (counter 1 must move with every call).  Pageable destinations, a cloud capacity of half the count,
    destinations inside a registered range (and that such a range is written in place), then the device forms with a full and a
    halved capacity."""
    A = hip
    left, right = workloads.structured_pair(W, H, D, seed=31)
    st, dev = _handle(A, W, H, pyoracle.Option(max_disparity=D)), DeviceBuffers(A)
    big = _poison(64 * N, np.uint8)
    A.host_register(big)

    def run(call):
        over = st.debug_counter(1)
        if mode == "budget":
            st.debug_set_budget(4)
        assert call(), A.last_error()
        if mode == "budget":
            assert st.debug_counter(1) == over + 1, "the voting continuation path was not taken"

    def host_pair(which, cap, inside=None):
        """(older entry point, products twin) -> their snapshots"""
        if inside is not None:
            inside[:] = POISON
        a = HostSet(A, cap, inside)
        if which is EX:
            run(lambda: st.MatchEx(left, right, a.disp, a.prov, a.conf))
        else:
            run(lambda: st.MatchOut(left, right, a.disp, CALIB, a.depth, a.cloud[:cap], a.disp8))
            a.count = st.cloud_count()
        got_a = a.snapshot(which)
        if inside is not None:
            inside[:] = POISON
        b = HostSet(A, cap, inside)
        req = (A.Products.from_arrays(provenance=b.prov, confidence=b.conf) if which is EX else
               A.Products.from_arrays(calib=CALIB, depth=b.depth, cloud=b.cloud[:cap], disp8=b.disp8))
        run(lambda: st.MatchProducts(left, right, b.disp, req))
        if which is OUT:
            b.count = st.cloud_count()
            assert int(req.count[0]) == b.count
        return got_a, b.snapshot(which)

    def device_pair(which, cap, ds):
        dl, dr = ds.left, ds.right
        ds.poison()
        if which is EX:
            run(lambda: st.match_device_ex(dl, dr, ds.p["disp"], ds.p["prov"], ds.p["conf"]) and st.wait())
        else:
            run(lambda: st.match_device_out(dl, dr, ds.p["disp"], CALIB, ds.p["depth"], ds.p["cloud"], cap, ds.p["word"], ds.p["disp8"]) and st.wait())
        got_a = ds.snapshot(which, st.cloud_count() if which is OUT else None)
        ds.poison()
        req = (A.Products.from_addresses(ds.p["prov"], ds.p["conf"]) if which is EX else
               A.Products.from_addresses(calib=CALIB, depth=ds.p["depth"], cloud=ds.p["cloud"], cloud_capacity=cap, cloud_count=ds.p["word"], disp8=ds.p["disp8"]))
        run(lambda: st.match_device_products(dl, dr, ds.p["disp"], req) and st.wait())
        return got_a, ds.snapshot(which, st.cloud_count() if which is OUT else None)

    def cloud_written(cloud_bytes, count, cap):
        k = 16 * min(count, cap)
        assert k == 0 or bytes([POISON]) * 16 not in (cloud_bytes[:16], cloud_bytes[k - 16:k]), "the first / last point was not written"
        assert cloud_bytes[k:] == bytes([POISON]) * (len(cloud_bytes) - k), "written behind the last point"

    try:
        if mode == "speckle":
            st.set_speckle_filter(50, 1.0)
        # ---- host forms, pageable destinations
        old, new = host_pair(EX, N)
        assert old == new, "adc_match_ex / adc_match_products differ"
        assert bytes([POISON]) * 64 not in (old[0]["disp"][:64], old[0]["prov"][:64], old[0]["conf"][:64]), "nothing was delivered"
        old, new = host_pair(OUT, N)
        assert old == new, "adc_match_out / adc_match_products differ"
        full, count = old
        assert 0 < count <= N
        cloud_written(full["cloud"], count, N)
        # ---- a capacity below the count truncates the same way: the first cap points of the full cloud, the whole count
        half = count // 2
        old, new = host_pair(OUT, half)
        assert old == new and old[1] == count
        assert old[0]["cloud"][:16 * half] == full["cloud"][:16 * half]
        cloud_written(old[0]["cloud"], count, half)
        assert {k: v for k, v in old[0].items() if k != "cloud"} == {k: v for k, v in full.items() if k != "cloud"}
        # ---- destinations inside a registered range hold the same bytes ...
        old, new = host_pair(EX, N, big)
        assert old == new
        old, new = host_pair(OUT, N, big)
        assert old == new == (full, count)
        # ... and are written in place (one resolver decides it for every entry point): once the device is idle and before adc_wait
        # has run, an asynchronous Match has filled its registered destinations, while pageable ones still wait in the staging blocks
        for inside in (big, None):
            if inside is not None:
                inside[:] = POISON
            s = HostSet(A, N, inside)
            req = A.Products.from_arrays(provenance=s.prov, confidence=s.conf, calib=CALIB, depth=s.depth, disp8=s.disp8)
            assert st.match_async_products(left, right, s.disp, req), A.last_error()
            assert A.lib().adc_device_synchronize() == 0
            early = [getattr(s, k).tobytes()[:64] for k in ("disp", "prov", "conf", "depth", "disp8")]
            assert st.wait(), A.last_error()
            if inside is None:
                assert all(e == bytes([POISON]) * 64 for e in early), "a pageable destination was written before adc_wait"
            else:
                assert bytes([POISON]) * 64 not in early, "a registered destination was not written in place"
            assert s.snapshot(("disp", "depth", "disp8"))[0] == {k: full[k] for k in ("disp", "depth", "disp8")}
        # ---- device forms: the caller's device buffers, written directly
        for cap in (N, half):
            ds = DeviceSet(A, dev, cap)
            ds.left, ds.right = dev.new(left), dev.new(right)
            old, new = device_pair(EX, cap, ds)
            assert old == new, "adc_match_device_ex / adc_match_device_products differ"
            old, new = device_pair(OUT, cap, ds)
            assert old == new and old[1] == (count, count), "adc_match_device_out / adc_match_device_products differ"
            assert old[0]["disp"] == full["disp"] and old[0]["depth"] == full["depth"] and old[0]["disp8"] == full["disp8"]
            assert old[0]["cloud"][:16 * min(cap, count)] == full["cloud"][:16 * min(cap, count)]
            cloud_written(old[0]["cloud"], count, cap)
    finally:
        dev.free()
        st.Release()
        A.host_unregister(big)


def test_one_path_makes_the_same_hip_calls():
    """The fault-injection build counts the hooked HIP calls of a warm call: each older entry point makes exactly those of its products
    twin (and again the same when called once more), and more than the plain entry point, so the count does see the products' calls.
    tests/match_request_probe.py runs in its own interpreter."""
    fault_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip_faultinj.so")
    if not os.path.exists(fault_lib):
        pytest.fail("libadcensus_hip_faultinj.so not built (make -C adcensus_amd/csrc)")
    env = dict(os.environ, ADC_HIP_LIB=fault_lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "match_request_probe.py")], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    o = json.loads([l for l in r.stdout.splitlines() if l.startswith("REQUEST_PROBE ")][-1][len("REQUEST_PROBE "):])
    print(o)
    for name, (older, twin, again) in o.items():
        assert older == twin == again, (name, o)
    # two maps: two kernels and two staging copies; three outputs: memset, three launches, count read-back, two staging copies, cloud copy-out
    assert o["ex"][0] >= o["plain"][0] + 4 and o["out"][0] >= o["plain"][0] + 8, o
    assert o["device_ex"][0] >= o["device_plain"][0] + 2 and o["device_out"][0] >= o["device_plain"][0] + 5, o
