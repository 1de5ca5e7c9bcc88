"""Derived figures of an evaluation report (adc_eval_report / adcensus_amd.EvalReport): rates, mean, RMS, the sparsification curve
of the confidence.  Plain Python on the report's integers; not part of the ABI (include/adcensus_c_api.h has the definitions the
integers follow)."""

ERR_UNITS = 1024.0  # eq is in 1/1024 pixel
FILL_NAMES = ("wta", "voting", "interpolation", "none")


def _stats(s, n_thresholds, with_rms):
    pixels, invalid = int(s.pixels), int(s.invalid)
    valid = pixels - invalid
    out = {"pixels": pixels, "invalid": invalid, "valid": valid,
           "invalid_rate": invalid / pixels if pixels else 0.0,
           # Middlebury's convention: the rate is over the mask's pixels, invalid ones are not counted as bad
           "bad": [int(s.bad[k]) for k in range(n_thresholds)],
           "bad_rate": [int(s.bad[k]) / pixels if pixels else 0.0 for k in range(n_thresholds)],
           "mean": int(s.sum_err_q) / ERR_UNITS / valid if valid else 0.0}
    if with_rms:
        out["rms"] = (int(s.sum_sq_err_q) / (ERR_UNITS * ERR_UNITS) / valid) ** 0.5 if valid else 0.0
    return out


def sparsification(conf_pixels, conf_bad):
    """Bins sorted from low confidence up; after removing bins 0 .. i-1 the error rate of the pixels that remain.  Returns (curve,
    area): curve[i] = (fraction removed, error rate of the rest), for i = 0 .. bins; area = trapezoid integral over the fraction
    removed (lower is better; a confidence that ranks errors perfectly removes all bad pixels first)."""
    px, bad = [int(v) for v in conf_pixels], [int(v) for v in conf_bad]
    total, total_bad = sum(px), sum(bad)
    curve, removed, removed_bad = [], 0, 0
    for i in range(len(px) + 1):
        rest = total - removed
        curve.append((removed / total if total else 0.0, (total_bad - removed_bad) / rest if rest else 0.0))
        if i < len(px):
            removed += px[i]
            removed_bad += bad[i]
    area = sum((b[0] - a[0]) * (a[1] + b[1]) / 2.0 for a, b in zip(curve, curve[1:]))
    return curve, area


def oracle_area(pixels, bad):
    """Area under the sparsification curve of the best possible ranking (every bad pixel removed before any good one): the rate
    falls from r = bad / pixels as (r - x) / (1 - x) until x = r."""
    if not pixels or not bad:
        return 0.0
    r = bad / pixels
    if r >= 1.0:
        return 1.0
    import math
    return r + (1.0 - r) * math.log(1.0 - r)  # integral of (r - x) / (1 - x) over [0, r]


def summarize(report):
    n = int(report.n_thresholds)
    out = {"thresholds": [float(report.thresholds[k]) for k in range(n)], "occ_thres": float(report.occ_thres),
           "all": _stats(report.all, n, True), "nonocc": _stats(report.nonocc, n, True),
           "occlusion_defined": bool(report.has_right_gt or report.has_nonocc_mask),
           "by_fill": {}, "speckle_removed_known": int(report.speckle_removed_known)}
    if report.has_provenance:
        out["by_fill"] = {FILL_NAMES[f]: _stats(report.by_fill[f], n, False) for f in range(4)}
    if report.has_provenance and report.has_confidence and n > 0:
        curve, area = sparsification(report.conf_pixels, report.conf_bad)
        px, bad = sum(int(v) for v in report.conf_pixels), sum(int(v) for v in report.conf_bad)
        out["confidence"] = {"pixels": px, "bad": bad, "curve": curve, "area": area, "oracle_area": oracle_area(px, bad),
                             "random_area": bad / px if px else 0.0}
    return out
