"""The 16-bit fixed-point disparity product of adc_products (include/adcensus_c_api.h: disp16) computed in numpy -- the definition
the GPU tests hold k_disp16 to, bit for bit -- and the helpers the products tests share: every product of one oracle run.  Every
operand is np.float32, so every operation rounds once to binary32."""
import numpy as np

from tests import extras_ref, outputs_ref, speckle_ref

F = np.float32
PROV_SPECKLE = 0x10


def disp16(disp, scale):
    """uint16, same shape: a = |d|; a not finite (+inf, -inf, NaN) -> 0; otherwise p = a * scale (one rounding),
    q = min(max(p, 1), 65535), pixel = uint16(q) truncating.  0 means invalid and nothing else."""
    a = np.abs(np.asarray(disp, F))
    finite = np.isfinite(a)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(finite, a, F(0)) * F(scale)  # (an overflowing product is +inf and saturates)
    q = np.minimum(np.maximum(p, F(1)), F(65535))
    return np.where(finite, q.astype(np.uint16), np.uint16(0)).astype(np.uint16)


def decode(pixels, scale):
    """The ADC_GT_U16 decode: g = v / scale in f32, 0 = unknown (+inf)."""
    v = np.asarray(pixels, np.uint16)
    return np.where(v == 0, F(np.inf), v.astype(F) / F(scale)).astype(F)


STAGES = extras_ref.STAGES  # what a test asks the oracle for


def products(o, opt, left_bgr, calib, scale, speckle=None):
    """Every product of one Match from an oracle dump with STAGES: a dict with disparity (the delivered map), provenance, confidence,
    depth (None without a calibration), cloud, disp8, disp16.  speckle = (max_size, max_diff): the filter's definition is applied to
    the map first, ADC_PROV_SPECKLE marks what it removed."""
    prov, conf = extras_ref.extras(o, opt)
    disp = o["disp_final"]
    if speckle is not None:
        filtered = speckle_ref.speckle_ref(disp, speckle[0], speckle[1])[0]
        removed = np.isfinite(disp) & ~np.isfinite(filtered)
        prov = np.where(removed, prov | PROV_SPECKLE, prov).astype(np.uint8)
        disp = filtered
    z, pts, g = outputs_ref.outputs(disp, left_bgr, calib)
    return {"disparity": disp, "provenance": prov, "confidence": conf, "depth": z, "cloud": pts, "disp8": g, "disp16": disp16(disp, scale)}
