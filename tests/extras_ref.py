"""The provenance and confidence maps of adc_match_ex (include/adcensus_c_api.h), computed in numpy from the oracle's stage dumps
cost_so, disp_left_wta, outlier_label and disp_after_irv -- the definition the GPU tests hold the product to, bit for bit."""
import numpy as np

LR_MASK, FILL_SHIFT = 3, 2
FILL_WTA, FILL_VOTING, FILL_INTERPOLATION, FILL_NONE = 0, 1, 2, 3
STAGES = ["cost_so", "disp_left_wta", "outlier_label", "disp_after_irv", "disp_final"]  # what a test asks the oracle for


def provenance(o, opt):
    """uint8 [H][W]: lr | fill << 2 (lr = outlier_label, 0 without an LR check)."""
    wta = o["disp_left_wta"]
    lr = o["outlier_label"].astype(np.uint8) if opt.do_lr_check else np.zeros(wta.shape, np.uint8)
    fill = np.where(np.isfinite(wta), FILL_WTA, FILL_NONE)
    if opt.do_lr_check and opt.do_filling:
        filled = np.where(np.isfinite(o["disp_after_irv"]), FILL_VOTING, FILL_INTERPOLATION)
    else:
        filled = np.full(wta.shape, FILL_NONE)
    fill = np.where(lr != 0, filled, fill)
    return (lr | (fill << FILL_SHIFT)).astype(np.uint8)


def confidence_from_costs(cost, fill=None):
    """float32 [...]: over the last axis (the costs C[d] of a pixel) c1 = min C, d1 = the lowest d with C[d] == c1, c2 = min over
    |d - d1| >= 2; (c2 - c1) / c2 in f32, 0 when c2 == 0, 1 when that set is empty; 0 wherever fill != 0."""
    cost = np.asarray(cost, np.float32)
    d = cost.shape[-1]
    d1 = np.argmin(cost, axis=-1)  # (first occurrence: the lowest d among equal minima)
    c1 = np.take_along_axis(cost, d1[..., None], axis=-1)[..., 0]
    far = np.abs(np.arange(d) - d1[..., None]) >= 2
    c2 = np.where(far, cost, np.float32(np.inf)).min(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        conf = (c2 - c1) / c2  # (float32 operands: correctly rounded)
    conf = np.where(c2 == 0, np.float32(0), conf)
    conf = np.where(~far.any(axis=-1), np.float32(1), conf).astype(np.float32)
    if fill is not None:
        conf = np.where(fill != FILL_WTA, np.float32(0), conf).astype(np.float32)
    return conf


def confidence(o, prov, rows=64):
    """float32 [H][W] from the oracle's cost_so (in row blocks: a 1080p volume is 1 GB)."""
    cost = o["cost_so"]
    fill = prov >> FILL_SHIFT
    out = np.empty(prov.shape, np.float32)
    for y in range(0, prov.shape[0], rows):
        out[y:y + rows] = confidence_from_costs(cost[y:y + rows], fill[y:y + rows])
    return out


def extras(o, opt):
    """(provenance, confidence) of an oracle dump with STAGES."""
    prov = provenance(o, opt)
    return prov, confidence(o, prov)
