"""Helper of tests/test_gpu_streams.py (run in an interpreter of its own, because the scanline switch ADC_SO_FAST is read once per
process): python tests/stream_probe.py GEOMETRY OPTION_SET [TABLE.npz]   |   python tests/stream_probe.py repeat NAME COUNT

Runs the streams of tests/streams.py for one geometry and option set, each on a handle of its own, the entry point rotating per Match
over match, match_async + wait and match_device + wait.  Every map is compared with the oracle's disp_final bit for bit (TABLE.npz:
"want_<image key>" arrays computed by the caller; without it the probe asks the oracle itself); a wrong pixel is recorded and the
stream goes on.  A Match that returns an error ends the probe at once with status 3: nothing more runs on the GPU after a failed HIP
call.  After every Match the debug counters COUNTERS are recorded.  Prints one line "RESULT <json>":
{"thresholds": {"17", "21", "23"}, "streams": {name: [{"key", "entry", "bad", "c": {counter: value}}, ...]}}.

repeat: ONE pair matched COUNT times on one handle (the way out of a hold, under switches that are read once per process), same rules,
counters REPEAT_COUNTERS; RESULT {"rows": [{"bad", "c"}]}.  NAME: n2w (tests/cases.py: 160x48 noise, D = 128) or med528 (528x400 noise,
D = 16; when the first Match left the speculative bands on, a "seam differed" verdict is armed for the second through the debug hook,
so that both holds of the median are set whichever seam failed by itself) or lam11 (160x48, D = 128, lambda_ad = lambda_census = 1, cross_t1 = 2, cross_t2 = 1: the n2w
noise pair once -- its saturated cost fails the scanline seams whatever the warm-up, cases.OPT_SEAMS_MAY_FAIL -- then the structured s2w
pair, whose costs keep their contrast under that lambda and whose arms the low colour thresholds keep short enough for the tail to move)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COUNTERS = (2, 4, 10, 11, 13, 16, 18, 19, 20, 22)


def _stop(out, what):
    print("ERROR " + what, flush=True)
    print("RESULT " + json.dumps(out), flush=True)
    os._exit(3)


def main(geometry, option_set, table_path=None):
    import adcensus_amd as A
    from tests import cases, streams
    w, h, dmin, dmax = streams.GEOMETRIES[geometry]
    opt = streams.option(geometry, option_set)
    keys = streams.image_keys(geometry)
    if table_path:
        with np.load(table_path) as z:
            want = {k: z["want_" + k] for k in keys}
    else:
        from oracle import pyoracle
        want = {k: v["want"] for k, v in streams.oracle_table(pyoracle.load("auto"), geometry, option_set).items()}
    imgs = {k: streams.image(geometry, k) for k in keys}
    lib = A.lib()
    n = w * h
    out = {"thresholds": {}, "streams": {}}
    dl, dr, dd = lib.adc_device_malloc(n * 3), lib.adc_device_malloc(n * 3), lib.adc_device_malloc(n * 4)
    if not (dl and dr and dd):
        _stop(out, "adc_device_malloc")
    turn = 0
    for name, order in streams.stream_orders(geometry).items():
        st = A.ADCensusStereo(device=0)
        if not st.Initialize(w, h, cases.to_product_option(opt)):
            _stop(out, "Initialize: " + A.last_error())
        out["thresholds"] = {str(c): st.debug_counter(c) for c in (17, 21, 23)}
        rows = out["streams"][name] = []
        for key in streams.expand(geometry, order):
            left, right = imgs[key]
            entry = streams.ENTRIES[turn % len(streams.ENTRIES)]
            turn += 1
            got = np.full((h, w), -1.0, np.float32)
            if entry == "match":
                ok = st.Match(left, right, got)
            elif entry == "match_async":
                ok = st.match_async(left, right, got) and st.wait()
            else:
                ok = lib.adc_memcpy_h2d(dl, left.ctypes.data, n * 3) == 0 and lib.adc_memcpy_h2d(dr, right.ctypes.data, n * 3) == 0
                ok = ok and st.match_device(dl, dr, dd) and st.wait()
                ok = ok and lib.adc_memcpy_d2h(got.ctypes.data, dd, n * 4) == 0
            if not ok:
                _stop(out, "%s, Match %d (%s, %s): %s" % (name, len(rows), key, entry, A.last_error()))
            bad = int((got.view(np.uint32) != want[key].view(np.uint32)).sum())
            rows.append({"key": key, "entry": entry, "bad": bad, "c": {str(c): st.debug_counter(c) for c in COUNTERS}})
        st.Release()
    for p in (dl, dr, dd):
        lib.adc_device_free(p)
    print("RESULT " + json.dumps(out), flush=True)


REPEAT_COUNTERS = (0, 2, 4, 5, 7, 8, 13, 15)


def repeat(name, count):
    import adcensus_amd as A
    from adcensus_amd import workloads
    from oracle import pyoracle
    from tests import cases
    if name == "n2w":
        (left, right), opt = cases.OPT_PAIRS["n2w"][0](), pyoracle.Option(**cases.OPT_PAIRS["n2w"][1])
    elif name == "med528":
        (left, right), opt = workloads.noise_pair(528, 400, seed=22), pyoracle.Option(max_disparity=16)
    elif name == "lam11":
        (left, right), opt = cases.OPT_PAIRS["n2w"][0](), pyoracle.Option(max_disparity=128, lambda_ad=1, lambda_census=1, cross_t1=2, cross_t2=1)
    else:
        raise SystemExit("unknown pair " + name)
    orc = pyoracle.load("auto")
    want = orc.run(left, right, opt, stages=["disp_final"])["disp_final"]
    later = None
    if name == "lam11":
        l2, r2 = cases.OPT_PAIRS["s2w"][0]()
        later = (l2, r2, orc.run(l2, r2, opt, stages=["disp_final"])["disp_final"])
    h, w = left.shape[:2]
    out = {"rows": []}
    st = A.ADCensusStereo(device=0)
    if not st.Initialize(w, h, cases.to_product_option(opt)):
        _stop(out, "Initialize: " + A.last_error())
    got = np.empty((h, w), np.float32)
    for k in range(count):
        got[:] = -1.0
        if later is not None and k == 1:
            left, right, want = later
        if not st.Match(left, right, got):
            _stop(out, "Match %d: %s" % (k, A.last_error()))
        out["rows"].append({"bad": int((got.view(np.uint32) != want.view(np.uint32)).sum()), "c": {str(c): st.debug_counter(c) for c in REPEAT_COUNTERS}})
        if name == "med528" and k == 0 and st.debug_counter(8) > 0:
            st.debug_run(A.RUN_MEDIAN, 101)
    st.Release()
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "repeat":
        repeat(sys.argv[2], int(sys.argv[3]))
    else:
        main(*sys.argv[1:4])
