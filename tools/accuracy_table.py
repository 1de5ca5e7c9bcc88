#!/usr/bin/env python3
"""The project's accuracy table: the three Middlebury pairs that come with ground truth (tests/golden/*_gt.npz), twelve runs each,
every run changing one thing against the default, scored on the device (adc_set_ground_truth / adc_evaluate) and summarised with
adcensus_amd/evaluation.py.  Runs on one MI355X.

    python tools/accuracy_table.py [--out profiles/accuracy.md] [--cpu-oracle]

--cpu-oracle needs no GPU: the maps come from the test suite's CPU oracle (oracle/, the build the GPU tier pins the product to bit for
bit; provenance and confidence from tests/extras_ref.py, the speckle filter from tests/speckle_ref.py) and are scored with the numpy
definition tests/eval_ref.py -- the same integers by construction, minutes instead of seconds.

Runs: default; do_filling = 0; do_lr_check = 0; do_discontinuity_adjustment = 1; the speckle filter (200 pixels, 1.0); each paper mode
alone, each pair of them, all three (adc_set_paper_modes; provenance and confidence are not defined there: no per-fill split, no
confidence columns)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adcensus_amd as A  # noqa: E402
from adcensus_amd import evaluation  # noqa: E402
from tests import cases  # noqa: E402

THRESHOLDS = [0.5, 1.0, 2.0, 4.0]
C5, SO, RA = A.PAPER_CENSUS5X5, A.PAPER_SO_SUM, A.PAPER_RIGHT_ARMS
RUNS = [("default", {}, None, 0), ("do_filling = 0", {"do_filling": 0}, None, 0), ("do_lr_check = 0", {"do_lr_check": 0}, None, 0),
        ("discontinuity adjustment", {"do_discontinuity_adjustment": 1}, None, 0), ("speckle filter 200, 1.0", {}, (200, 1.0), 0),
        ("paper: 5x5 census", {}, None, C5), ("paper: averaged scanline paths", {}, None, SO), ("paper: right-image arms", {}, None, RA),
        ("paper: census + paths", {}, None, C5 | SO), ("paper: census + arms", {}, None, C5 | RA), ("paper: paths + arms", {}, None, SO | RA),
        ("paper: all three", {}, None, C5 | SO | RA)]
PAIRS = [("cone", "Cone", 64), ("cloth3", "Cloth3", 128), ("wood2", "Wood2", 128)]


def pct(rates):
    return " / ".join("%.2f" % (100.0 * r) for r in rates)


def cpu_oracle_report(left, right, z, dmax, kw, speckle, paper):
    """One run without a device: the CPU oracle's maps through the numpy definition, packed into an EvalReport."""
    import ctypes as C
    from oracle import pyoracle
    from tests import eval_ref, extras_ref
    from tests.speckle_ref import speckle_ref
    opt = pyoracle.Option(max_disparity=dmax, **kw)
    if paper:
        d, prov, conf = pyoracle.load("port").run(left, right, opt, stages=["disp_final"], paper_modes=paper)["disp_final"], None, None
    else:
        dump = pyoracle.load("auto").run(left, right, opt, stages=extras_ref.STAGES)
        d = dump["disp_final"]
        prov, conf = extras_ref.extras(dump, opt)
    if speckle:
        filtered = speckle_ref(d, *speckle)[0]
        prov = np.where(np.isfinite(d) & ~np.isfinite(filtered), prov | A.PROV_SPECKLE, prov).astype(np.uint8)
        d = filtered
    g, gr = eval_ref.decode_gt(z["left"], eval_ref.GT_U8, float(z["scale"])), eval_ref.decode_gt(z["right"], eval_ref.GT_U8, float(z["scale"]))
    words = eval_ref.to_words(eval_ref.evaluate(d, g, eval_ref.nonocc_from_right(g, gr, 1.0), THRESHOLDS, prov, conf)[0])
    rep = A.EvalReport()
    C.memmove(C.byref(rep), words.ctypes.data, words.nbytes)
    rep.n_thresholds, rep.occ_thres, rep.has_right_gt, rep.has_provenance, rep.has_confidence = len(THRESHOLDS), 1.0, 1, int(prov is not None), int(conf is not None)
    for k, t in enumerate(THRESHOLDS):
        rep.thresholds[k] = t
    return rep


def row(name, s):
    cells = [name]
    for m in ("all", "nonocc"):
        cells += ["%.2f" % (100.0 * s[m]["invalid_rate"]), pct(s[m]["bad_rate"]), "%.4f" % s[m]["mean"], "%.4f" % s[m]["rms"]]
    if s["by_fill"]:
        known = max(1, s["all"]["pixels"])
        cells.append(", ".join("%.1f (%.1f)" % (100.0 * v["pixels"] / known, 100.0 * v["bad_rate"][1]) for v in s["by_fill"].values()))
        c = s["confidence"]
        cells.append("%.4f / %.4f / %.4f" % (c["area"], c["oracle_area"], c["random_area"]))
    else:
        cells += ["-", "-"]
    return "| " + " | ".join(cells) + " |"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--cpu-oracle", action="store_true")
    a = ap.parse_args()
    how = "the test suite's CPU oracle and the numpy definition, no device" if a.cpu_oracle else "one MI355X (%s)" % A.lib().adc_version().decode()
    out = ["# Accuracy against the Middlebury ground truth", "",
           "`tools/accuracy_table.py%s`: %s.  Ground truth: `tests/golden/*_gt.npz`; non-occluded = left-right cross-check of the two"
           % (" --cpu-oracle" if a.cpu_oracle else "", how),
           "ground-truth views within 1 px.  bad = share of the mask's pixels whose error exceeds 0.5 / 1 / 2 / 4 px (invalid pixels are",
           "counted in their own column, not as bad); mean and RMS in pixels over the valid pixels of the mask.  fill = share of the known",
           "pixels per provenance class (winner-takes-all / region voting / interpolation / none) with its bad > 1 px rate.  AUSC = area",
           "under the sparsification curve of the confidence (bad > 0.5 px among the measured pixels; lower is better), next to the area of",
           "the best possible ranking (by true error) and of a random one.", ""]
    notes = {}
    for key, title, dmax in PAIRS:
        left, right, _ = cases.make_case(key)
        z = np.load(os.path.join(cases.GOLDEN_DIR, key + "_gt.npz"))
        h, w = left.shape[:2]
        out += ["## %s (%d x %d, disparities 0-%d)" % (title, w, h, dmax), "",
                "| run | all: invalid % | all: bad 0.5 / 1 / 2 / 4 % | all: mean | all: RMS | nonocc: invalid % | nonocc: bad 0.5 / 1 / 2 / 4 % | nonocc: mean | nonocc: RMS | fill share % (bad > 1 %): wta, voting, interpolation, none | AUSC / best / random |",
                "|---|---|---|---|---|---|---|---|---|---|---|"]
        for name, kw, speckle, paper in RUNS:
            if a.cpu_oracle:
                s = evaluation.summarize(cpu_oracle_report(left, right, z, dmax, kw, speckle, paper))
                out.append(row(name, s))
                notes[(key, name)] = s
                print(out[-1], flush=True)
                continue
            st = A.ADCensusStereo(device=0)
            assert st.Initialize(w, h, A.ADCensusOption(max_disparity=dmax, **kw)), A.last_error()
            st.set_ground_truth(z["left"], z["right"], scale=float(z["scale"]))
            if speckle:
                st.set_speckle_filter(*speckle)
            if paper:
                st.set_paper_modes(paper)
                d, prov, conf = st.match(left, right), None, None
            else:
                d, prov, conf = st.match_ex(left, right)
            rep, _, _ = st.evaluate(d, prov, conf, THRESHOLDS, err=False, cls=False)
            st.Release()
            s = evaluation.summarize(rep)
            out.append(row(name, s))
            notes[(key, name)] = s
        out.append("")
    # what the table shows, in the table's own numbers
    def bad1(key, name, mask="nonocc"):
        return 100.0 * notes[(key, name)][mask]["bad_rate"][1]
    deltas = {name: [bad1(k, name) - bad1(k, "default") for k, _, _ in PAIRS] for name, _, _, paper in RUNS if paper}
    best = min(deltas, key=lambda n: sum(deltas[n]))
    out += ["## What the table shows", "",
            "Paper modes: against the default, the non-occluded bad > 1 px rate moves by %s points (Cone, Cloth3, Wood2) with all three modes on; "
            "the mode or combination with the lowest sum over the three pairs is \"%s\" (%s points), and single modes range from %+.2f to %+.2f points."
            % (", ".join("%+.2f" % v for v in deltas["paper: all three"]), best[len("paper: "):], ", ".join("%+.2f" % v for v in deltas[best]),
               min(min(deltas[n]) for n in list(deltas)[:3]), max(max(deltas[n]) for n in list(deltas)[:3])), ""]
    conf = [notes[(k, "default")]["confidence"] for k, _, _ in PAIRS]
    out += ["Confidence: removing pixels from the lowest confidence up lowers the error rate of the rest on every pair -- the area under the sparsification "
            "curve is %s of the random ranking's (Cone, Cloth3, Wood2), while the best possible ranking reaches %s: the confidence ranks errors, with "
            "room left." % (", ".join("%.0f %%" % (100.0 * c["area"] / c["random_area"]) for c in conf),
                            ", ".join("%.0f %%" % (100.0 * c["oracle_area"] / c["random_area"]) for c in conf)), ""]
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
