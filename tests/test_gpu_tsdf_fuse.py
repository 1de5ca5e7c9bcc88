"""GPU tier of the stereo-aware TSDF fusion (adcensus_amd/csrc/k_tsdf_fuse.hip): the two kernels against tests/tsdf_fuse_ref.py bit for
bit on every case of tests/tsdf_fuse_cases.py -- the weight map into a poisoned buffer at an odd address whose bytes behind the map
must stay poisoned, the whole volume through adc_tsdf_download after every frame, both reports; the identity with
adc_tsdf_integrate_device; the host entry points; calls enqueued back to back and in front of a ray cast and a track with one
adc_wait; refusals on a real handle; and the accuracy figures of tests/tsdf_fuse_checks.py with the kernels as the integrator."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from tests import tsdf_fuse_cases as FC
from tests import tsdf_fuse_checks as FK
from tests import tsdf_fuse_ref as FR
from tests import tsdf_raycast_ref as RR
from tests import tsdf_ref as T
from tests import tsdf_track_cases as KC
from tests import tsdf_track_ref as TR
from tests.test_gpu_outputs import POISON, DeviceBuffers, _handle
from tests.test_tsdf_api import c_frame, c_params
from tests.test_tsdf_fuse_api import c_fuse_params, c_weight_params, fuse_words, weight_words
from tests.test_tsdf_raycast_api import c_view
from tests.test_tsdf_track_api import c_track_params

pytestmark = pytest.mark.gpu

F = np.float32
TAIL = 64  # poisoned bytes behind every output buffer
OPT = pyoracle.Option(max_disparity=16)
RESULT_BYTES = 960


def _frep(rep):
    return [getattr(rep, k) for k in FR.FUSE_FIELDS] + list(rep.reserved_)


def _wrep(rep):
    return [getattr(rep, k) for k in FR.WEIGHT_FIELDS] + list(rep.reserved_)


def _same_volume(what, got, want):
    assert np.array_equal(got[0], want[0]), (what, "voxel words", int((got[0] != want[0]).sum()))
    assert (got[1] is None) == (want[1] is None), what
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "colour words", int((got[1] != want[1]).sum()))


def _weights(A, st, dev, m, fr, wp, prov, conf, what, wait=True):
    """adc_tsdf_weights_device into a poisoned buffer that starts at an odd address -> (device address, weight map, report words)"""
    H, W = m.shape
    base = dev.alloc(1 + W * H + TAIL, POISON)
    ok = st.tsdf_weights_device(dev.new(m), c_frame(fr), base + 1, c_weight_params(wp), None if prov is None else dev.new(prov), None if conf is None else dev.new(conf))
    assert ok, what + ": " + A.last_error()
    if not wait:
        return base + 1, None, None
    assert st.wait(), what + ": " + A.last_error()
    raw = dev.get(base, 1 + W * H + TAIL, np.uint8)
    assert raw[0] == POISON and (raw[1 + W * H:] == POISON).all(), what + ": written outside the weight map"
    return base + 1, raw[1:1 + W * H].reshape(H, W), _wrep(st.tsdf_fuse_report()[1])


def _open(A, c):
    W, H = c["size"]
    st = _handle(A, W, H, OPT)
    assert st.tsdf_create(c_params(c["params"])), A.last_error()
    if c["init"] is not None:
        st.tsdf_upload(*c["init"])
    return st


@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_kernels_equal_the_reference(hip, name):
    A = hip
    c, r = FC.case(name), FC.reference(name)
    st, dev = _open(A, c), DeviceBuffers(A)
    try:
        assert st.tsdf_fuse_report() == (None, None)
        for i, (f, want, rep, wmap, wrep) in enumerate(zip(c["frames"], r["volumes"], r["reports"], r["wmaps"], r["wreports"])):
            what = "%s frame %d" % (name, i)
            d_w = None
            if f["weight"] is not None:
                d_w = dev.new(f["weight"])
            elif f["wparams"] is not None:
                d_w, got_w, got_rep = _weights(A, st, dev, f["map"], f["frame"], f["wparams"], f["prov"], f["conf"], what)
                assert np.array_equal(got_w, wmap), (what, "weights", int((got_w != wmap).sum()))
                assert got_rep == weight_words(wrep), (what, got_rep, wrep)
            d_map = dev.new(f["map"])
            ok = st.tsdf_fuse_device(d_map, c_frame(f["frame"]), d_w, c_fuse_params(f["fp"]), None if f["image"] is None else dev.new(f["image"]))
            assert ok and st.wait(), what + ": " + A.last_error()
            assert _frep(st.tsdf_fuse_report()[0]) == fuse_words(rep), (what, _frep(st.tsdf_fuse_report()[0]), rep)
            _same_volume(what, st.tsdf_download(), want)
            assert dev.get(d_map, f["map"].shape, F).tobytes() == f["map"].tobytes(), what  # (the inputs are only read)
    finally:
        dev.free()
        st.Release()


@pytest.mark.parametrize("name", FC.WEIGHT_CASE_NAMES)
def test_weight_kernel_equals_the_reference(hip, name):
    """the device form (no volume exists on the handle) and the host form"""
    A = hip
    c = FC.weight_case(name)
    want, rep = FC.weight_reference(name)
    W, H = c["size"]
    st, dev = _handle(A, W, H, OPT), DeviceBuffers(A)
    try:
        _, got, got_rep = _weights(A, st, dev, c["map"], c["frame"], c["wparams"], c["prov"], c["conf"], name)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        assert got_rep == weight_words(rep), (name, got_rep, rep)
        w, hrep = st.tsdf_weights(c["map"], c_frame(c["frame"]), c_weight_params(c["wparams"]), c["prov"], c["conf"])
        assert np.array_equal(w, want) and _wrep(hrep) == weight_words(rep), name
    finally:
        dev.free()
        st.Release()


@pytest.mark.parametrize("name", FC.IDENTITY_CASES + ("long_row",))
def test_without_weights_and_flag_the_fuse_is_the_integrate(hip, name):
    """d_weight NULL with no flag, NULL params, and a weight map of all ones: the volume bytes and the four common counts of
    adc_tsdf_integrate_device on the same frames"""
    A = hip
    c = FC.case(name)
    W, H = c["size"]
    st, dev = _open(A, c), DeviceBuffers(A)
    try:
        ones = dev.new(np.ones((H, W), np.uint8))
        ptrs = [(dev.new(f["map"]), None if f["image"] is None else dev.new(f["image"]), c_frame(f["frame"])) for f in c["frames"]]
        vols, reps = [], []
        for d_m, d_i, fr in ptrs:
            assert st.tsdf_integrate_device(d_m, fr, d_i) and st.wait(), A.last_error()
            rep = st.tsdf_report()[0]
            vols.append(st.tsdf_download())
            reps.append([rep.in_frustum, rep.no_depth, 0, rep.occluded, rep.updated, 0, 0, 0])
        for d_w, params in ((None, None), (None, A.TsdfFuseParams()), (ones, None), (ones, A.TsdfFuseParams(0, 7.0))):
            assert st.tsdf_reset(), A.last_error()
            for (d_m, d_i, fr), vol, rep in zip(ptrs, vols, reps):
                assert st.tsdf_fuse_device(d_m, fr, d_w, params, d_i) and st.wait(), A.last_error()
                assert _frep(st.tsdf_fuse_report()[0]) == rep, (name, _frep(st.tsdf_fuse_report()[0]), rep)
                _same_volume(name, st.tsdf_download(), vol)
    finally:
        dev.free()
        st.Release()


def test_host_entry_points_and_refusals_on_a_real_handle(hip):
    A = hip
    c, r = FC.case("disparity_specials"), FC.reference("disparity_specials")
    st, dev = _open(A, c), DeviceBuffers(A)
    try:
        for i, (f, want, rep, wmap, wrep) in enumerate(zip(c["frames"], r["volumes"], r["reports"], r["wmaps"], r["wreports"])):
            w, got = st.tsdf_weights(f["map"], c_frame(f["frame"]), c_weight_params(f["wparams"]), f["prov"], f["conf"])
            assert np.array_equal(w, wmap) and _wrep(got) == weight_words(wrep), i
            got = st.tsdf_fuse(f["map"], c_frame(f["frame"]), w, c_fuse_params(f["fp"]), f["image"])
            assert _frep(got) == fuse_words(rep), i
            _same_volume("host frame %d" % i, st.tsdf_download(), want)
        before = st.tsdf_download()
        f = c["frames"][0]
        d_map, fr = dev.new(f["map"]), c_frame(f["frame"])
        for call, why in ((lambda: st.tsdf_fuse_device(d_map + 2, fr), "4-byte aligned"),
                          (lambda: st.tsdf_fuse_device(d_map, fr, None, A.TsdfFuseParams(2, 0.0)), "unknown flag"),
                          (lambda: st.tsdf_fuse_device(d_map, fr, None, A.TsdfFuseParams(1, -1.0)), "interp_gap"),
                          (lambda: st.tsdf_weights_device(d_map, fr, None), "null weight"),
                          (lambda: st.tsdf_weights_device(d_map, fr, d_map, A.TsdfWeightParams(depth_power=3)), "depth_power"),
                          (lambda: st.tsdf_weights_device(d_map, fr, d_map, None, None, d_map + 1), "d_confidence must be 4-byte aligned")):
            assert not call() and why in A.last_error(), (why, A.last_error())
        assert st.wait()
        _same_volume("after refusals", st.tsdf_download(), before)
        # an image without a colour volume is refused, not ignored
        assert st.tsdf_create(c_params(dict(c["params"], flags=0))), A.last_error()
        assert not st.tsdf_fuse_device(d_map, fr, None, None, dev.new(f["image"])) and "colour volume" in A.last_error()
        assert st.tsdf_destroy() and not st.tsdf_fuse_device(d_map, fr) and "no volume" in A.last_error()
    finally:
        dev.free()
        st.Release()


def test_two_fuses_back_to_back_then_ray_cast_and_track_with_one_wait(hip):
    """The corner at 64 x 48 into the chain's 64 x 48 x 40 volume: weights, fuse at A, weights, fuse at A again (the second weights call
    overwrites nothing the first fuse still reads: each has its own map), a ray cast from A and a track of the frame rendered at SMALL
    -- six calls enqueued with no wait between them, one adc_wait.  Everything equals the chain of the numpy references."""
    A = hip
    W, H = 64, 48
    c = dict(KC.scene(W, H, KC.A_POSE, KC.SMALL))
    focal, _, cx, cy, _ = c["frame"]["calib"]
    p = T.params(64, 48, 40, 0.04, (-1.28, -0.96, 1.0), 0.16)
    at_a, _ = KC.render(c["planes"], W, H, focal, cx, cy, *KC.A_POSE)
    fr = T.frame(c["frame"]["calib"], *KC.A_POSE, kind=T.FROM_DEPTH)
    wps = (FR.weight_params((16, 4, 1, 0), 0.0, 0, 4, 1.5), FR.weight_params((3, 0, 0, 0), 0.0, 0, 0, 1.0))
    fp = FR.fuse_params(FR.FUSE_BILINEAR, 0.2)
    vol, reps = T.empty(p), []
    for wp in wps:
        w, wrep = FR.weights(at_a, fr, wp)
        vol, rep = FR.fuse(vol, p, fr, at_a, None, w, fp)
        reps.append(rep)
    voxel, trunc = F(p["voxel"]), F(p["trunc"])
    step = float(voxel * F(0.5))
    v = RR.view(W, H, focal, cx, cy, *KC.A_POSE, z_near=float(voxel), z_far=3.0e38, step=step, skip=max(float(trunc * F(0.5)), step), max_steps=16384)
    cast = RR.raycast(vol, p, v)
    want = TR.track(c["map"], None, c["frame"], TR.model(W, H, focal, cx, cy, *KC.A_POSE), cast["depth"], cast["normals"], c["params"])
    st, dev = _handle(A, W, H, OPT), DeviceBuffers(A)
    try:
        assert st.tsdf_create(c_params(p)), A.last_error()
        d_at_a, d_map = dev.new(at_a), dev.new(np.ascontiguousarray(c["map"], F))
        d_depth, d_normals = dev.alloc(4 * W * H + TAIL, POISON), dev.alloc(16 * W * H + TAIL, POISON)
        d_res = dev.alloc(RESULT_BYTES + TAIL, POISON)
        for wp in wps:
            d_w = dev.alloc(W * H + TAIL, POISON)
            assert st.tsdf_weights_device(d_at_a, c_frame(fr), d_w, c_weight_params(wp)), A.last_error()
            assert st.tsdf_fuse_device(d_at_a, c_frame(fr), d_w, c_fuse_params(fp)), A.last_error()
        view = c_view(v)
        assert st.tsdf_raycast_device(view, d_depth, d_normals), A.last_error()
        assert st.track_device(d_map, c_frame(c["frame"]), view, d_depth, d_normals, c_track_params(c["params"]), None, d_res), A.last_error()
        assert st.wait(), A.last_error()
        assert _frep(st.tsdf_fuse_report()[0]) == fuse_words(reps[-1]) and _wrep(st.tsdf_fuse_report()[1]) == weight_words(wrep)
        _same_volume("chain", st.tsdf_download(), vol)
        assert dev.get(d_depth, (H, W), F).tobytes() == cast["depth"].tobytes() and dev.get(d_normals, (H, W, 4), F).tobytes() == cast["normals"].tobytes()
        assert bytes(st.track_result()) == TR.result_bytes(want)
    finally:
        dev.free()
        st.Release()


def test_accuracy_figures_with_the_kernels_as_the_integrator(hip):
    """tests/tsdf_fuse_checks.py (a) and (b) with adc_tsdf_fuse / adc_tsdf_weights in place of the numpy integrator: the kernels are
    bit-exact, so the figures are the reference's own (profiles/tsdf_fuse_accuracy.md); printed, and asserted as on the CPU."""
    A = hip
    handles = {}

    def handle(shape, p):
        key = (shape, tuple(sorted((k, str(v)) for k, v in p.items())))
        if key not in handles:
            for st in handles.values():
                st.Release()
            handles.clear()
            handles[key] = _handle(A, shape[1], shape[0], OPT)
            assert handles[key].tsdf_create(c_params(p)), A.last_error()
        return handles[key]

    def fuse(vol, p, fr, m, image, weight, fp):
        st = handle(m.shape, p)
        st.tsdf_upload(*vol)
        rep = st.tsdf_fuse(m, c_frame(fr), weight, c_fuse_params(fp), image)
        return st.tsdf_download(), {k: getattr(rep, k) for k in FR.FUSE_FIELDS}

    def weights(m, fr, wp, prov, conf):
        st = handle(m.shape, T.params(*FK.NOISE_VOLUME, max_weight=1024))
        w, rep = st.tsdf_weights(m, c_frame(fr), c_weight_params(wp), prov, conf)
        return w, {k: getattr(rep, k) for k in FR.WEIGHT_FIELDS}

    try:
        near, bil = FK.check_staircase(fuse, False), FK.check_staircase(fuse, True)
        print("staircase chain on the kernels, nearest :", near)
        print("staircase chain on the kernels, bilinear:", bil)
        assert near["final"] > 0.1 * near["initial"] and not FK.chain_criterion(near)
        assert bil["final"] <= bil["voxel"] and bil["final"] <= 0.1 * bil["initial"]
        m = FK.check_noise(fuse, weights)
        print("noise scene on the kernels:", m)
        assert m["ratio"] <= FK.NOISE_BOUND < 0.75 and abs(m["ratio"] - FK.NOISE_MEASURED_RATIO) < 5e-4
    finally:
        for st in handles.values():
            st.Release()
