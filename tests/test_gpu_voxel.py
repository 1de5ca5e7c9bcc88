"""GPU tier of the voxel-grid filter of the cloud (adc_set_cloud_voxel_grid; adcensus_amd/csrc/k_voxel.hip) against tests/voxel_ref.py:
the records byte for byte, the count, the device count word and the report -- on constructed maps through adc_reproject_device (tile and
table edges, one voxel per octant, a leaf near the pixel footprint, the crop's inclusive ends, invalid pixels, a pose, capacities), then
through every path that delivers a cloud (synchronous, asynchronous, device-resident, the farm), behind the speckle filter and an input
format, behind a redo of adc_wait, and after clearing the grid."""
import ctypes as C

import numpy as np
import pytest

from adcensus_amd import workloads
from oracle import pyoracle
from tests import cases, outputs_ref, voxel_ref
from tests.test_gpu_outputs import CONE_CALIB, POISON, DeviceBuffers, _handle, _reproject

pytestmark = pytest.mark.gpu

F = np.float32
OPT16 = pyoracle.Option(max_disparity=16)


def _calib(w, h, doffs=0.0):
    return (100.0, 0.5, w / 2.0, h / 2.0, doffs)  # Z = 50 / |d|: about 0.8 .. 50 on the maps below


def _ramp(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return (F(10) + F(0.05) * xs.astype(F) + F(0.02) * ys.astype(F)).astype(F)  # a slanted plane: long runs of pixels in one voxel


def _noise(w, h, seed, holes=0.1):
    rng = np.random.default_rng(seed)
    v = (F(1) + rng.random((h, w), dtype=F) * F(59)).astype(F)
    v[rng.random((h, w)) < 0.1] *= F(-1)
    v[rng.random((h, w)) < holes] = F(np.inf)
    return v


def _image(w, h):
    return np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _set(st, g):
    st.set_cloud_voxel_grid(float(g["leaf"]), float(g["z_min"]), float(g["z_max"]), g["pose"])


def _check_cloud(what, got, count, want, report, want_report, capacity=None):
    """got: the caller's whole buffer (POISON behind what was written)"""
    n = len(want) if capacity is None else min(len(want), capacity)
    assert count == len(want), "%s: count %d, expected %d" % (what, count, len(want))
    assert report == want_report, "%s: report %s, expected %s" % (what, report, want_report)
    assert got[:n].tobytes() == want[:n].tobytes(), "%s: the records differ" % what
    assert got[n:].tobytes() == bytes([POISON]) * (16 * (len(got) - n)), what + ": written behind the last record"


def _check(A, st, dev, what, disp, left, calib, g, capacity=None):
    want, want_report = voxel_ref.voxel_cloud(disp, left, calib, g)
    _set(st, g)
    _, cloud, count, _, word = _reproject(A, st, dev, disp, left, calib, want=("cloud",), capacity=capacity)
    assert word == count, what
    _check_cloud(what, cloud, count, want, st.voxel_report(), want_report, capacity)
    dev.free()
    return want, want_report


@pytest.mark.parametrize("w,h", [(70, 37), (64, 32), (1, 1), (1, 130)])
def test_shapes(hip, w, h):
    """Three ragged tiles; W * H a power of two (load factor exactly 0.5); a single pixel; a single column -- smooth and noisy maps, a
    leaf with many points per voxel and one near the footprint."""
    A = hip
    st, dev = _handle(A, w, h, OPT16), DeviceBuffers(A)
    try:
        for name, disp in (("ramp", _ramp(w, h)), ("noise", _noise(w, h, 3))):
            for leaf in (0.5, 0.02):
                _check(A, st, dev, "%s %dx%d leaf %g" % (name, w, h, leaf), disp, _image(w, h), _calib(w, h), voxel_ref.grid(leaf))
    finally:
        dev.free()
        st.Release()


def test_one_voxel_per_octant_and_none(hip):
    """leaf 1e8: every point in one of four voxels (X, Y of both signs, Z > 0) -- maximal contention, n > 255, f == 1.0f at the tiny
    negative u; leaf 1e-7: Z * inv >= 2^20 everywhere, nothing is kept and nothing written."""
    A = hip
    w, h = 70, 37
    disp, left = _noise(w, h, 5), _image(w, h)
    st, dev = _handle(A, w, h, OPT16), DeviceBuffers(A)
    try:
        want, rep = _check(A, st, dev, "leaf 1e8", disp, left, _calib(w, h), voxel_ref.grid(1e8))
        assert 2 <= len(want) <= 4 and want["pad"].max() == 255 and rep["points_kept"] == rep["points_valid"] > 1000
        assert (want["x"] < 0).any() and (want["x"] == 0).any()  # (mq = 65535 at ix = -1; ix = 0)
        want, rep = _check(A, st, dev, "leaf 1e-7", disp, left, _calib(w, h), voxel_ref.grid(1e-7))
        assert len(want) == 0 and rep["points_kept"] == 0 and rep["voxels"] == 0 and rep["points_valid"] > 1000
    finally:
        dev.free()
        st.Release()


def test_leaf_near_the_pixel_footprint(hip):
    A = hip
    w, h = 130, 33
    disp, left = _noise(w, h, 7, holes=0.0), _image(w, h)
    st, dev = _handle(A, w, h, OPT16), DeviceBuffers(A)
    try:
        want, rep = _check(A, st, dev, "footprint", disp, left, _calib(w, h), voxel_ref.grid(0.005))
        assert np.median(want["pad"]) == 1 and rep["voxels"] > 0.9 * rep["points_kept"]
    finally:
        dev.free()
        st.Release()


def test_crop_ends_are_inclusive(hip):
    A = hip
    w, h = 70, 37
    disp, left, calib = _noise(w, h, 9), _image(w, h), _calib(w, h)
    z, valid = outputs_ref.depth(disp, calib)
    zs = np.sort(z[valid])
    lo, hi = zs[len(zs) // 4], zs[3 * len(zs) // 4]
    st, dev = _handle(A, w, h, OPT16), DeviceBuffers(A)
    try:
        _, rep = _check(A, st, dev, "crop", disp, left, calib, voxel_ref.grid(0.5, lo, hi))
        assert rep["points_kept"] == int(((zs >= lo) & (zs <= hi)).sum()) and rep["points_kept"] < rep["points_valid"]
        _, rep = _check(A, st, dev, "crop to one value", disp, left, calib, voxel_ref.grid(0.5, lo, lo))
        assert rep["points_kept"] == int((zs == lo).sum()) >= 1
        _, rep = _check(A, st, dev, "z_max = +inf", disp, left, calib, voxel_ref.grid(0.5, lo, np.inf))
        assert rep["points_kept"] == int((zs >= lo).sum())
    finally:
        dev.free()
        st.Release()


def test_invalid_pixels(hip):
    """+inf, -inf and NaN pixels, and a doffs that makes s <= 0 for the small disparities"""
    A = hip
    w, h = 70, 37
    disp, left = _noise(w, h, 11), _image(w, h)
    flat = disp.reshape(-1)
    flat[5::17] = F(-np.inf)
    flat[7::19] = F(np.nan)
    st, dev = _handle(A, w, h, OPT16), DeviceBuffers(A)
    try:
        _, rep0 = _check(A, st, dev, "invalid", disp, left, _calib(w, h), voxel_ref.grid(0.3))
        _, rep1 = _check(A, st, dev, "doffs -30", disp, left, _calib(w, h, -30.0), voxel_ref.grid(0.3))
        assert 0 < rep1["points_valid"] < rep0["points_valid"] < w * h
    finally:
        dev.free()
        st.Release()


def test_pose(hip):
    A = hip
    w, h = 70, 37
    a = np.deg2rad(30.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], F)
    t = np.array([-1.0, 0.5, -3.5], F)
    disp, left, calib = _ramp(w, h), _image(w, h), _calib(w, h)
    st, dev = _handle(A, w, h, OPT16), DeviceBuffers(A)
    try:
        want, _ = _check(A, st, dev, "pose", disp, left, calib, voxel_ref.grid(0.25, pose=(R, t)))
        plain, _ = voxel_ref.voxel_cloud(disp, left, calib, voxel_ref.grid(0.25))
        assert (want["z"] < 0).any() and (want["z"] > 0).any() and (plain["z"] > 0).all()  # (the translation moves points across octants)
    finally:
        dev.free()
        st.Release()


def test_capacity(hip):
    A = hip
    w, h = 70, 37
    disp, left, calib, g = _noise(w, h, 13), _image(w, h), _calib(w, h), voxel_ref.grid(0.2)
    count = len(voxel_ref.voxel_cloud(disp, left, calib, g)[0])
    assert 10 < count < w * h
    st, dev = _handle(A, w, h, OPT16), DeviceBuffers(A)
    try:
        for cap in (0, count - 1, w * h):
            _check(A, st, dev, "capacity %d" % cap, disp, left, calib, g, capacity=cap)
    finally:
        dev.free()
        st.Release()


def _want_of(disp, left, calib, g):
    return voxel_ref.voxel_cloud(disp, left, calib, g)


def test_cone_through_match_products(hip):
    """450 x 375 through a real Match: the voxel cloud of the delivered map; depth and disp8 of the same request are untouched."""
    A = hip
    left, right, opt = cases.make_case("cone")
    h, w = left.shape[:2]
    g = voxel_ref.grid(0.05)
    st = _handle(A, w, h, opt)
    try:
        _set(st, g)
        got = st.match_products(left, right, CONE_CALIB, depth=True, cloud=True, disp8=True)
        want, want_report = _want_of(got["disparity"], left, CONE_CALIB, g)
        assert got["cloud_count"] == len(want) == st.cloud_count() and got["cloud"].tobytes() == want.tobytes()
        assert st.voxel_report() == want_report and 0 < want_report["voxels"] < want_report["points_kept"] // 4
        want_z, _, want_g = outputs_ref.outputs(got["disparity"], left, CONE_CALIB)
        assert got["depth"].tobytes() == want_z.tobytes() and got["disp8"].tobytes() == want_g.tobytes()
    finally:
        st.Release()


def test_every_delivery_path(hip):
    """synchronous host, asynchronous with adc_wait, device-resident, and a farm of 2 pipelines with 3 pairs"""
    A = hip
    w, h, n = 96, 64, 96 * 64
    calib, g = _calib(w, h), voxel_ref.grid(0.4)
    pairs = [workloads.structured_pair(w, h, 16, seed=21), workloads.noise_pair(w, h, seed=22), workloads.structured_pair(w, h, 16, seed=23)]
    st, dev = _handle(A, w, h, OPT16), DeviceBuffers(A)
    try:
        _set(st, g)
        left, right = pairs[0]
        got = st.match_products(left, right, calib, cloud=True)
        want, want_report = _want_of(got["disparity"], left, calib, g)
        assert len(want) > 10 and got["cloud_count"] == len(want) and got["cloud"].tobytes() == want.tobytes() and st.voxel_report() == want_report
        # asynchronous: a capacity below the count, nothing behind it
        cap = len(want) - 3
        buf = np.frombuffer(bytes([POISON]) * (16 * (cap + 2)), A.POINT_DTYPE).copy()
        d = np.empty((h, w), F)
        req = A.Products.from_arrays(calib=calib, cloud=buf[:cap])
        assert st.match_async_products(left, right, d, req) and st.wait(), A.last_error()
        assert d.tobytes() == got["disparity"].tobytes() and int(req.count[0]) == len(want)
        _check_cloud("async", buf, st.cloud_count(), want, st.voxel_report(), want_report, cap)
        # device-resident
        dl, dr, dd = dev.new(left), dev.new(right), dev.alloc(4 * n)
        pc, pn = dev.alloc(16 * (n + 1), POISON), dev.alloc(16, POISON)
        preq = A.Products.from_addresses(calib=calib, cloud=pc, cloud_capacity=n, cloud_count=pn)
        assert st.match_device_products(dl, dr, dd, preq) and st.wait(), A.last_error()
        assert int(dev.get(pn, 1, np.uint32)[0]) == len(want)
        _check_cloud("device", dev.get(pc, n + 1, A.POINT_DTYPE), st.cloud_count(), want, st.voxel_report(), want_report)
    finally:
        dev.free()
        st.Release()
    farm = A.PairFarm(w, h, cases.to_product_option(OPT16), device=0, pipelines=2)
    try:
        farm.set_cloud_voxel_grid(float(g["leaf"]))
        held = []
        for left, right in pairs:
            buf = np.frombuffer(bytes([POISON]) * (16 * n), A.POINT_DTYPE).copy()
            d = np.empty((h, w), F)
            req = A.Products.from_arrays(calib=calib, cloud=buf)
            farm.submit(left.copy(), right.copy(), d, req)
            held.append((left, d, buf, req))
        assert farm.drain() == 3
        counts = []
        for i, (left, d, buf, req) in enumerate(held):
            want, _ = _want_of(d, left, calib, g)
            counts.append(len(want))
            assert int(req.count[0]) == len(want), "farm pair %d" % i
            n_w = len(want)
            assert buf[:n_w].tobytes() == want.tobytes() and buf[n_w:].tobytes() == bytes([POISON]) * (16 * (n - n_w)), "farm pair %d" % i
        assert len(set(counts)) > 1  # (the pairs differ: a count delivered with the wrong pair would show)
        farm.set_cloud_voxel_grid(None)
        left, right = pairs[1]
        buf, d = np.zeros(n, A.POINT_DTYPE), np.empty((h, w), F)
        req = A.Products.from_arrays(calib=calib, cloud=buf)
        farm.wait(farm.submit(left, right, d, req))
        plain = outputs_ref.cloud(d, left, calib)
        assert int(req.count[0]) == len(plain) and buf[:len(plain)].tobytes() == plain.tobytes()
    finally:
        farm.close()


def test_behind_the_speckle_filter_and_an_input_format(hip):
    """Pixels the speckle filter removed contribute nothing (the cloud is that of the delivered map); with an input format set the
    colours are those of the converted left image."""
    A = hip
    w, h = 96, 64
    src_l, src_r = workloads.noise_pair(w, h, seed=31)
    raw_l, raw_r = np.ascontiguousarray(src_l[..., 1]), np.ascontiguousarray(src_r[..., 1])
    left = np.repeat(raw_l[..., None], 3, 2)  # (ADC_PIX_GRAY8: B = G = R = the sample)
    calib, g = _calib(w, h), voxel_ref.grid(0.4)
    st = _handle(A, w, h, OPT16)
    try:
        st.set_speckle_filter(50, 1.0)
        for side in (A.SIDE_LEFT, A.SIDE_RIGHT):
            st.set_input_format(side, A.RawFormat(w, h, 0, A.PIX_GRAY8))
        _set(st, g)
        got = st.match_products(raw_l, raw_r, calib, cloud=True)
        assert st.speckle_stats()[2] > 0 and np.isinf(got["disparity"]).any()
        want, want_report = _want_of(got["disparity"], left, calib, g)
        assert got["cloud_count"] == len(want) and got["cloud"].tobytes() == want.tobytes() and st.voxel_report() == want_report
        assert want_report["points_valid"] == int((np.isfinite(got["disparity"]) & (got["disparity"] != 0)).sum())
        assert (want["r"] == want["g"]).all() and (want["g"] == want["b"]).all()
    finally:
        st.Release()


def test_behind_a_redo(hip):
    """One armed median fallback (the existing debug hook): the voxel cloud describes the redone map."""
    A = hip
    w, h, d = 240, 330, 32
    left, right = workloads.structured_pair(w, h, d, seed=11)
    calib, g = _calib(w, h), voxel_ref.grid(0.3)
    st = _handle(A, w, h, pyoracle.Option(max_disparity=d, do_filling=0))
    try:
        _set(st, g)
        first = st.match_products(left, right, calib, cloud=True)
        fall = st.debug_counter(0)
        st.debug_run(A.RUN_MEDIAN, 100)
        got = st.match_products(left, right, calib, cloud=True)
        assert st.debug_counter(0) == fall + 1, "the median fallback path was not taken"
        assert got["disparity"].tobytes() == first["disparity"].tobytes()
        want, want_report = _want_of(got["disparity"], left, calib, g)
        assert got["cloud_count"] == len(want) and got["cloud"].tobytes() == want.tobytes() and st.voxel_report() == want_report
    finally:
        st.Release()


def test_set_clear_and_refusals(hip):
    A = hip
    L = A.lib()
    w, h = 70, 37
    disp, left, calib = _noise(w, h, 15), _image(w, h), _calib(w, h)
    st, dev = _handle(A, w, h, OPT16), DeviceBuffers(A)
    try:
        _check(A, st, dev, "set", disp, left, calib, voxel_ref.grid(0.3))
        # a cloud without a calibration while a grid is set: refused, nothing enqueued
        dd, dl, pc = dev.new(disp), dev.new(left), dev.alloc(16 * w * h, POISON)
        assert not st.reproject_device(dd, dl, None, None, pc, w * h, None, None) and "calibration" in A.last_error()
        assert dev.get(pc, w * h * 16, np.uint8).tobytes() == bytes([POISON]) * (16 * w * h)
        dev.free()
        st.clear_cloud_voxel_grid()
        for cal in (calib, None):
            _, cloud, count, _, word = _reproject(A, st, dev, disp, left, cal, want=("cloud",))
            want = outputs_ref.cloud(disp, left, cal)
            assert count == word == len(want) and cloud[:count].tobytes() == want.tobytes() and not cloud[:count]["pad"].any()
            dev.free()
        # the setters while a Match is pending
        pair = workloads.structured_pair(w, h, 16, seed=3)
        d = np.empty((h, w), F)
        grid = A.VoxelGrid(0.3)
        assert st.match_async(pair[0], pair[1], d)
        assert L.adc_set_cloud_voxel_grid(st._h, C.byref(grid)) == 1 and "pending" in A.last_error()
        assert L.adc_clear_cloud_voxel_grid(st._h) == 1 and "pending" in A.last_error()
        assert st.wait()
        assert L.adc_set_cloud_voxel_grid(st._h, C.byref(grid)) == 0 and L.adc_clear_cloud_voxel_grid(st._h) == 0
    finally:
        dev.free()
        st.Release()


def test_cli_voxel(hip, tmp_path):
    """adcensus_cli ... --calib ... --voxel on Cone: the PLY payload and the rows of -cloud.txt are the voxel cloud of the map the run
    wrote (<out>.pfm); the map and the depth are those of a run without the flag."""
    import os
    import subprocess

    from PIL import Image

    from tests.test_outputs_api import read_pfm, read_ply
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "adcensus_amd", "bin", "adcensus_cli")
    if not os.path.exists(cli):
        pytest.fail("adcensus_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
    left, right, _ = cases.make_case("cone")
    Image.fromarray(np.ascontiguousarray(left[:, :, ::-1])).save(tmp_path / "left.png")
    Image.fromarray(np.ascontiguousarray(right[:, :, ::-1])).save(tmp_path / "right.png")
    env = dict(os.environ, ADC_VERBOSE="0")
    for pref, extra in (("cal", []), ("vox", ["--voxel", "0.05,9.5,20"])):
        out = subprocess.run([cli, str(tmp_path / "left.png"), str(tmp_path / "right.png"), "0", "64", str(tmp_path / pref), "--calib", "3740,0.16,225,187.5,0"] + extra,
                             capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
    for suffix in (".pfm", "-depth.pfm", "-d.png"):
        assert open(str(tmp_path / "cal") + suffix, "rb").read() == open(str(tmp_path / "vox") + suffix, "rb").read(), suffix
    want, rep = voxel_ref.voxel_cloud(read_pfm(str(tmp_path / "vox") + ".pfm"), left, CONE_CALIB, voxel_ref.grid(0.05, 9.5, 20.0))
    assert "%d valid points, %d kept, %d voxels" % (rep["points_valid"], rep["points_kept"], rep["voxels"]) in out.stdout
    assert 0 < rep["voxels"] < rep["points_kept"] < rep["points_valid"]
    n, rows = read_ply(str(tmp_path / "vox") + "-cloud.ply")
    assert n == len(rows) == len(want)
    for name in ("x", "y", "z"):
        assert np.array_equal(rows[name].view(np.uint32), want[name].view(np.uint32)), name
    assert all(np.array_equal(rows[c], want[c]) for c in "rgb")
    lines = open(str(tmp_path / "vox") + "-cloud.txt").read().splitlines()
    assert lines == ["%f %f %f %d %d %d" % (p["x"], p["y"], p["z"], p["r"], p["g"], p["b"]) for p in want]
