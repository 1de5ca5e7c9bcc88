"""adcensus_amd -- MI355X-native AD-Census stereo matcher (host-side Python mirror).

The product is the C-ABI shared library ``adcensus_amd/lib/libadcensus_hip.so`` (hand-written HIP
kernels for gfx950, built by ``adcensus_amd/csrc/Makefile``) plus the C++ facade
``include/ADCensusStereo.h``.  This module is a thin ctypes mirror of that facade
(``ADCensusStereo.Initialize / Match / Reset``, ``ADCensusOption`` -- same names, argument meaning
and error behaviour as the reference's ADCensusStereo.h:14-41 / adcensus_types.h:45-75) used by the
tests and by bench.py.  There is NO CPU fallback: if the HIP library is missing or no GPU is
visible, construction / Initialize fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ADC_HIP_LIB") or os.path.join(_HERE, "lib", "libadcensus_hip.so")  # (override: A/B builds, tools/)

# stage / buffer ids (include/adcensus_c_api.h)
STAGES = ["cost", "arms", "aggregate", "scanline", "wta", "refine"]
(BUF_GRAY_LEFT, BUF_GRAY_RIGHT, BUF_CENSUS_LEFT, BUF_CENSUS_RIGHT, BUF_ARMS, BUF_SUPCOUNT_H, BUF_SUPCOUNT_V,
 BUF_VOLUME_A, BUF_DISP_LEFT, BUF_DISP_RIGHT, BUF_OUTLIER_LABEL) = range(11)
(RUN_GRAY_CENSUS, RUN_COST, RUN_ARMS, RUN_AGGREGATE, RUN_SCANLINE, RUN_WTA, RUN_LRCHECK, RUN_REGION_VOTING,
 RUN_INTERPOLATION, RUN_DISCONTINUITY, RUN_MEDIAN) = range(11)
MAX_DISP_RANGE = 2047
PAPER_CENSUS5X5, PAPER_SO_SUM, PAPER_RIGHT_ARMS = 1, 2, 4  # adc_set_paper_modes (opt-in, not the reference's behaviour)
# provenance codes of match_ex (adc_match_ex): code = lr | (fill << PROV_FILL_SHIFT)
LR_CONSISTENT, LR_MISMATCH, LR_OCCLUSION = 0, 1, 2
FILL_WTA, FILL_VOTING, FILL_INTERPOLATION, FILL_NONE = 0, 1, 2, 3
PROV_LR_MASK, PROV_FILL_SHIFT = 3, 2
PROV_SPECKLE = 0x10  # set by a Match with the speckle filter on, at the pixels the filter removed (ADC_PROV_SPECKLE)
PIX_BGR8, PIX_RGB8, PIX_GRAY8, PIX_BGRA8 = 0, 1, 2, 3  # adc_raw_format.format (ADC_PIX_*)
PIX_GRAY16 = 0x10  # camera layouts (include/adcensus_c_api.h); codes 4..15 stay invalid
PIX_BAYER_RGGB8, PIX_BAYER_GRBG8, PIX_BAYER_GBRG8, PIX_BAYER_BGGR8 = 0x20, 0x21, 0x22, 0x23
PIX_BAYER_RGGB16, PIX_BAYER_GRBG16, PIX_BAYER_GBRG16, PIX_BAYER_BGGR16 = 0x30, 0x31, 0x32, 0x33
PIX_YUYV, PIX_UYVY, PIX_NV12 = 0x40, 0x41, 0x42
# bytes per pixel of a row (NV12: of a luma row; its chroma plane follows, RawFormat.nbytes)
PIX_BYTES = {PIX_BGR8: 3, PIX_RGB8: 3, PIX_GRAY8: 1, PIX_BGRA8: 4, PIX_GRAY16: 2, PIX_YUYV: 2, PIX_UYVY: 2, PIX_NV12: 1,
             PIX_BAYER_RGGB8: 1, PIX_BAYER_GRBG8: 1, PIX_BAYER_GBRG8: 1, PIX_BAYER_BGGR8: 1,
             PIX_BAYER_RGGB16: 2, PIX_BAYER_GRBG16: 2, PIX_BAYER_GBRG16: 2, PIX_BAYER_BGGR16: 2}


def pix_bits(fmt, bits):
    """ADC_PIX_BITS: the format word of a 16-bit layout with its significant bits (9..16; 0 = 16)."""
    return int(fmt) | (int(bits) << 8)
SIDE_LEFT, SIDE_RIGHT = 0, 1  # ADC_SIDE_*
GT_U8, GT_U16, GT_F32 = 0, 1, 2  # adc_gt.format (ADC_GT_*)
GT_DTYPES = {GT_U8: np.uint8, GT_U16: np.uint16, GT_F32: np.float32}
EVAL_MAX_THRESHOLDS, EVAL_ERR_BINS, EVAL_CONF_BINS = 4, 256, 256
EVAL_KNOWN, EVAL_VALID, EVAL_BAD, EVAL_OCCLUDED = 1, 2, 4, 8  # bits of the class map (ADC_EVAL_*)
REG_FROM_DISPARITY, REG_FROM_DEPTH = 0, 1  # input kind of a registration (ADC_REG_FROM_*)
REG_NO_SPLAT, REG_PRETEST = 1, 2  # flags of register_depth (ADC_REG_NO_SPLAT, ADC_REG_PRETEST)
REG_MAX_SPLAT = 8


class ADCensusOption(C.Structure):
    """Mirror of struct ADCensusOption (adcensus_types.h:45-75) == adc_option of the C ABI."""
    _fields_ = [
        ("min_disparity", C.c_int32), ("max_disparity", C.c_int32),
        ("lambda_ad", C.c_int32), ("lambda_census", C.c_int32),
        ("cross_L1", C.c_int32), ("cross_L2", C.c_int32),
        ("cross_t1", C.c_int32), ("cross_t2", C.c_int32),
        ("so_p1", C.c_float), ("so_p2", C.c_float),
        ("so_tso", C.c_int32), ("irv_ts", C.c_int32),
        ("irv_th", C.c_float), ("lrcheck_thres", C.c_float),
        ("do_lr_check", C.c_uint8), ("do_filling", C.c_uint8),
        ("do_discontinuity_adjustment", C.c_uint8), ("reserved_", C.c_uint8),
    ]

    def __init__(self, **kw):
        super().__init__()
        lib().adc_option_default(C.byref(self))
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


class Calib(C.Structure):
    """adc_calib: Middlebury calib.txt convention, Z = baseline * focal_px / (d + doffs)."""
    _fields_ = [("focal_px", C.c_float), ("baseline", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("doffs", C.c_float)]


class Point(C.Structure):
    """adc_point: 16 bytes."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("r", C.c_uint8), ("g", C.c_uint8), ("b", C.c_uint8), ("pad", C.c_uint8)]


class Outputs(C.Structure):
    """adc_outputs: the request of adc_match_out (host addresses) / adc_match_device_out / adc_reproject_device (device addresses)."""
    _fields_ = [("calib", C.POINTER(Calib)), ("depth", C.c_void_p), ("cloud", C.c_void_p), ("cloud_capacity", C.c_uint64),
                ("cloud_count", C.c_void_p), ("disp8", C.c_void_p)]


class Products(C.Structure):
    """adc_products: every optional product of one Match -- provenance / confidence (adc_match_ex), an embedded Outputs (adc_match_out)
    and the 16-bit fixed-point map disp16 with its scale.  Host addresses for adc_match_products / adc_match_async_products /
    adc_farm_submit_products, device addresses for adc_match_device_products.  from_arrays() builds one from numpy arrays and keeps
    them alive."""
    _fields_ = [("provenance", C.c_void_p), ("confidence", C.c_void_p), ("out", Outputs), ("disp16", C.c_void_p),
                ("disp16_scale", C.c_float), ("reserved_", C.c_uint32)]

    @classmethod
    def from_addresses(cls, provenance=None, confidence=None, calib=None, depth=None, cloud=None, cloud_capacity=0, cloud_count=None,
                       disp8=None, disp16=None, disp16_scale=256.0):
        c = _calib(calib)
        req = cls(provenance, confidence, Outputs(C.pointer(c) if c is not None else None, depth, cloud, int(cloud_capacity), cloud_count, disp8),
                  disp16, float(disp16_scale), 0)
        req._keep = [c]
        return req

    @classmethod
    def from_arrays(cls, provenance=None, confidence=None, calib=None, depth=None, cloud=None, disp8=None, disp16=None, disp16_scale=256.0):
        """Host request from C-contiguous numpy arrays (None: not requested): provenance uint8, confidence float32, depth float32, disp8
        uint8, disp16 uint16 [H][W]; cloud a POINT_DTYPE array whose length is the capacity.  With a cloud, `count` (a uint32 array of one
        element, written at delivery) is part of the request."""
        for a, dt in ((provenance, np.uint8), (confidence, np.float32), (depth, np.float32), (disp8, np.uint8), (disp16, np.uint16), (cloud, POINT_DTYPE)):
            assert a is None or (a.dtype == dt and a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"]), dt
        count = np.zeros(1, np.uint32) if cloud is not None else None
        adr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        req = cls.from_addresses(adr(provenance), adr(confidence), calib, adr(depth), adr(cloud), 0 if cloud is None else cloud.size, adr(count),
                                 adr(disp8), adr(disp16), disp16_scale)
        req._keep += [provenance, confidence, depth, cloud, disp8, disp16, count]
        req.count = count
        return req

    def sizes_ok(self, n):
        """every map array from_arrays() was given holds n elements"""
        return all(a is None or a.dtype == POINT_DTYPE or a.size in (1, n) for a in getattr(self, "_keep", [])[1:])


class RawFormat(C.Structure):
    """adc_raw_format: geometry of the raw images of one side while rectification is on (pitch_bytes 0: tightly packed rows)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("pitch_bytes", C.c_int32), ("format", C.c_int32)]

    def __init__(self, width=0, height=0, pitch_bytes=0, format=PIX_BGR8):
        super().__init__(int(width), int(height), int(pitch_bytes) or int(width) * PIX_BYTES.get(int(format) & 0xff, 0), int(format))

    @property
    def nbytes(self):
        luma = self.height * self.pitch_bytes
        return luma // 2 * 3 if (self.format & 0xff) == PIX_NV12 else luma  # (NV12: the chroma plane behind the luma plane)


class CameraModel(C.Structure):
    """adc_camera_model: intrinsics, Brown-Conrady distortion, rectifying rotation R (9 values, row-major), new intrinsics."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("k1", C.c_float), ("k2", C.c_float), ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float),
                ("R", C.c_float * 9),
                ("new_fx", C.c_float), ("new_fy", C.c_float), ("new_cx", C.c_float), ("new_cy", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        self.R = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, (C.c_float * 9)(*[float(x) for x in v]) if k == "R" else float(v))


class GroundTruth(C.Structure):
    """adc_gt: one view's ground truth as the caller holds it (host array, ADC_GT_* format, row pitch in bytes, scale)."""
    _fields_ = [("data", C.c_void_p), ("format", C.c_int32), ("pitch_bytes", C.c_int32), ("scale", C.c_float), ("reserved_", C.c_int32)]

    def __init__(self, array=None, scale=1.0, format=None, pitch_bytes=0):
        """array: a 2-D uint8 / uint16 / float32 numpy array (kept alive by this object); its row stride becomes the pitch."""
        super().__init__()
        if array is not None:
            a = np.asarray(array)
            if format is None:
                format = {np.dtype(np.uint8): GT_U8, np.dtype(np.uint16): GT_U16, np.dtype(np.float32): GT_F32}[a.dtype]
            if a.ndim != 2 or a.strides[1] != a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
                a = np.ascontiguousarray(a)
            self._keep = a
            self.data = a.ctypes.data
            pitch_bytes = pitch_bytes or a.strides[0]
        self.format, self.pitch_bytes, self.scale = int(0 if format is None else format), int(pitch_bytes), float(scale)


class EvalParams(C.Structure):
    """adc_eval_params: up to EVAL_MAX_THRESHOLDS bad-pixel thresholds (finite, >= 0)."""
    _fields_ = [("n_thresholds", C.c_int32), ("thresholds", C.c_float * EVAL_MAX_THRESHOLDS)]

    def __init__(self, thresholds=(1.0,)):
        super().__init__()
        ts = [float(t) for t in thresholds]
        self.n_thresholds = len(ts)  # (more than four: the library refuses the call)
        for k, t in enumerate(ts[:EVAL_MAX_THRESHOLDS]):
            self.thresholds[k] = t


class EvalMaskStats(C.Structure):
    _fields_ = [("pixels", C.c_uint64), ("invalid", C.c_uint64), ("bad", C.c_uint64 * EVAL_MAX_THRESHOLDS), ("sum_err_q", C.c_uint64),
                ("sum_sq_err_q", C.c_uint64), ("err_hist", C.c_uint64 * EVAL_ERR_BINS)]


class EvalFillStats(C.Structure):
    _fields_ = [("pixels", C.c_uint64), ("invalid", C.c_uint64), ("bad", C.c_uint64 * EVAL_MAX_THRESHOLDS), ("sum_err_q", C.c_uint64)]


class EvalReport(C.Structure):
    """adc_eval_report: integer counters (all / nonocc masks, the four fill classes, confidence bins) and the echo of the request;
    adcensus_amd.evaluation.summarize turns it into rates, mean, RMS and the sparsification curve."""
    _fields_ = [("all", EvalMaskStats), ("nonocc", EvalMaskStats), ("by_fill", EvalFillStats * 4), ("speckle_removed_known", C.c_uint64),
                ("conf_pixels", C.c_uint64 * EVAL_CONF_BINS), ("conf_bad", C.c_uint64 * EVAL_CONF_BINS),
                ("thresholds", C.c_float * EVAL_MAX_THRESHOLDS), ("n_thresholds", C.c_int32), ("occ_thres", C.c_float),
                ("has_right_gt", C.c_uint8), ("has_nonocc_mask", C.c_uint8), ("has_provenance", C.c_uint8), ("has_confidence", C.c_uint8),
                ("reserved_", C.c_int32)]

    def words(self):
        """The counters in declaration order as a uint64 array (everything in front of the echo)."""
        return np.frombuffer(bytes(self), np.uint64, EvalReport.thresholds.offset // 8).copy()


class RegTarget(C.Structure):
    """adc_reg_target: the camera depth is registered into -- size, intrinsics, Brown-Conrady distortion, R (row-major, left-rectified
    -> target coordinates) and t (unit of the calibration's baseline).  Defaults: R = I, everything else 0."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("k1", C.c_float), ("k2", C.c_float), ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float), ("R", C.c_float * 9),
                ("t", C.c_float * 3)]

    def __init__(self, **kw):
        super().__init__()
        self.R[0] = self.R[4] = self.R[8] = 1.0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            if k in ("R", "t"):
                v = (C.c_float * (9 if k == "R" else 3))(*[float(x) for x in np.asarray(v, np.float32).ravel()])
            setattr(self, k, v)


class RegReport(C.Structure):
    """adc_reg_report: source pixels with a valid Z, those with a non-empty footprint, target pixels filled."""
    _fields_ = [("src_valid", C.c_uint32), ("src_projected", C.c_uint32), ("dst_filled", C.c_uint32), ("reserved_", C.c_uint32)]


NORMALS_MAX_RADIUS = 7  # ADC_NORMALS_MAX_RADIUS


class NormalsParams(C.Structure):
    """adc_normals_params: radius r in [1, 7] (a (2r+1) x (2r+1) window), max_diff in (0, 64] pixels of disparity (the gate that keeps
    a window from fitting across a depth step), min_points in [3, (2r+1)^2]; flags and the reserved words 0."""
    _fields_ = [("radius", C.c_int32), ("max_diff", C.c_float), ("min_points", C.c_int32), ("flags", C.c_uint32), ("reserved_", C.c_uint32 * 4)]

    def __init__(self, radius=2, max_diff=1.0, min_points=5, flags=0):
        super().__init__()
        self.radius, self.max_diff, self.min_points, self.flags = int(radius), float(max_diff), int(min_points), int(flags)


class NormalsReport(C.Structure):
    """adc_normals_report: usable centres, and of those the fitted ones, those with fewer than min_points taps, the degenerate ones."""
    _fields_ = [("usable", C.c_uint32), ("fitted", C.c_uint32), ("few_points", C.c_uint32), ("degenerate", C.c_uint32)]


MESH_MAX_STEP = 16  # ADC_MESH_MAX_STEP


class MeshParams(C.Structure):
    """adc_mesh_params: max_diff >= 0 pixels of disparity (+inf: no gate) joins two lattice pixels into an edge; step in [1, 16]: every
    step-th column and row forms the lattice; flags and the reserved words 0."""
    _fields_ = [("max_diff", C.c_float), ("step", C.c_int32), ("flags", C.c_uint32), ("reserved_", C.c_uint32 * 5)]

    def __init__(self, max_diff=1.0, step=1, flags=0):
        super().__init__()
        self.max_diff, self.step, self.flags = float(max_diff), int(step), int(flags)


class MeshReport(C.Structure):
    """adc_mesh_report: valid lattice pixels, vertices, triangles, cells that emit two triangles / one; triangles = 2 * cells_two + cells_one."""
    _fields_ = [("lattice_valid", C.c_uint32), ("vertices", C.c_uint32), ("triangles", C.c_uint32), ("cells_two", C.c_uint32), ("cells_one", C.c_uint32),
                ("reserved_", C.c_uint32 * 3)]


TSDF_COLOR = 0x1  # ADC_TSDF_COLOR: a colour word per voxel
TSDF_MAX_DIM = 2048  # ADC_TSDF_MAX_DIM
TSDF_ENTRY_POINTS = ("adc_tsdf_create", "adc_tsdf_reset", "adc_tsdf_destroy", "adc_tsdf_integrate_device", "adc_tsdf_integrate", "adc_tsdf_extract_device",
                     "adc_tsdf_extract", "adc_get_tsdf_report", "adc_tsdf_get_volume_device", "adc_tsdf_download", "adc_tsdf_upload")


class TsdfParams(C.Structure):
    """adc_tsdf_params: nx, ny, nz voxels (each in [4, 2048], nx a multiple of 4, at most 2^30 in all) of edge `voxel`; origin = the
    world position of the corner of voxel (0, 0, 0); the truncation distance trunc; the crop z_min <= Zc <= z_max of the camera-frame
    Z; max_weight in [1, 65535]; flags (TSDF_COLOR); the reserved words 0."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("voxel", C.c_float), ("origin", C.c_float * 3), ("trunc", C.c_float),
                ("z_min", C.c_float), ("z_max", C.c_float), ("max_weight", C.c_uint32), ("flags", C.c_uint32), ("reserved_", C.c_uint32 * 4)]

    def __init__(self, nx=0, ny=0, nz=0, voxel=0.0, origin=(0.0, 0.0, 0.0), trunc=0.0, z_min=0.0, z_max=float("inf"), max_weight=64, flags=0):
        super().__init__()
        self.nx, self.ny, self.nz, self.voxel, self.trunc = int(nx), int(ny), int(nz), float(voxel), float(trunc)
        self.origin = (C.c_float * 3)(*[float(v) for v in origin])
        self.z_min, self.z_max, self.max_weight, self.flags = float(z_min), float(z_max), int(max_weight), int(flags)


class TsdfFrame(C.Structure):
    """adc_tsdf_frame: what the map holds (REG_FROM_DISPARITY / REG_FROM_DEPTH), the calibration, and R (row-major) / t, which take a
    WORLD point into the rectified left camera frame: Xc = R * Xw + t.  Defaults: disparity, R = I, t = 0."""
    _fields_ = [("kind", C.c_int32), ("calib", Calib), ("R", C.c_float * 9), ("t", C.c_float * 3), ("flags", C.c_uint32), ("reserved_", C.c_uint32 * 5)]

    def __init__(self, calib=None, R=None, t=None, kind=0, flags=0):
        super().__init__()
        self.kind, self.flags = int(kind), int(flags)
        if calib is not None:
            self.calib = _calib(calib)
        self.R = (C.c_float * 9)(*[float(x) for x in np.asarray((1, 0, 0, 0, 1, 0, 0, 0, 1) if R is None else R, np.float32).ravel()])
        self.t = (C.c_float * 3)(*[float(x) for x in np.asarray((0, 0, 0) if t is None else t, np.float32).ravel()])


class TsdfReport(C.Structure):
    """adc_tsdf_report: voxels that projected into the image, and of those the ones whose pixel has no depth, the ones further than
    trunc behind the surface, the ones updated."""
    _fields_ = [("in_frustum", C.c_uint32), ("no_depth", C.c_uint32), ("occluded", C.c_uint32), ("updated", C.c_uint32), ("reserved_", C.c_uint32 * 4)]


class TsdfExtractParams(C.Structure):
    """adc_tsdf_extract_params: min_weight in [1, 65535] both voxels of a crossing need; the reserved words 0."""
    _fields_ = [("min_weight", C.c_uint32), ("reserved_", C.c_uint32 * 7)]

    def __init__(self, min_weight=1):
        super().__init__()
        self.min_weight = int(min_weight)


class TsdfExtractReport(C.Structure):
    """adc_tsdf_extract_report: voxels with w >= min_weight, surface points (crossings) whatever the capacity."""
    _fields_ = [("voxels_seen", C.c_uint32), ("points", C.c_uint32), ("reserved_", C.c_uint32 * 6)]


TSDF_FUSE_ENTRY_POINTS = ("adc_tsdf_weights_device", "adc_tsdf_weights", "adc_tsdf_fuse_device", "adc_tsdf_fuse", "adc_get_tsdf_fuse_report")
TSDF_W_SCALE_CONFIDENCE = 1
TSDF_FUSE_BILINEAR = 1


class TsdfWeightParams(C.Structure):
    """adc_tsdf_weight_params: the base weight of each fill class (FILL_WTA, _VOTING, _INTERPOLATION, _NONE), the confidence below
    which a measured pixel gets 0, flags (TSDF_W_SCALE_CONFIDENCE), the power (0, 2, 4) of z_ref / Z the weight falls with; the
    reserved words 0.  The defaults are those of a NULL params."""
    _fields_ = [("class_weight", C.c_uint8 * 4), ("min_confidence", C.c_float), ("flags", C.c_uint32), ("depth_power", C.c_uint32), ("z_ref", C.c_float),
                ("reserved_", C.c_uint32 * 11)]

    def __init__(self, class_weight=(16, 4, 1, 0), min_confidence=0.0, flags=0, depth_power=4, z_ref=1.0):
        super().__init__()
        self.class_weight = (C.c_uint8 * 4)(*[int(v) for v in class_weight])
        self.min_confidence, self.flags, self.depth_power, self.z_ref = float(min_confidence), int(flags), int(depth_power), float(z_ref)


class TsdfWeightReport(C.Structure):
    """adc_tsdf_weight_report: pixels with depth, with a weight above 0, measured pixels below min_confidence, weights of 255."""
    _fields_ = [("valid", C.c_uint32), ("nonzero", C.c_uint32), ("below_confidence", C.c_uint32), ("saturated", C.c_uint32), ("reserved_", C.c_uint32 * 4)]


class TsdfFuseParams(C.Structure):
    """adc_tsdf_fuse_params: flags (TSDF_FUSE_BILINEAR) and the largest spread of the four map values around a projection, in the
    map's own unit, over which they are still interpolated; the reserved words 0."""
    _fields_ = [("flags", C.c_uint32), ("interp_gap", C.c_float), ("reserved_", C.c_uint32 * 6)]

    def __init__(self, flags=0, interp_gap=0.0):
        super().__init__()
        self.flags, self.interp_gap = int(flags), float(interp_gap)


class TsdfFuseReport(C.Structure):
    """adc_tsdf_fuse_report: as TsdfReport, with the voxels whose pixel has the weight 0 and the ones that read the map interpolated."""
    _fields_ = [("in_frustum", C.c_uint32), ("no_depth", C.c_uint32), ("unweighted", C.c_uint32), ("occluded", C.c_uint32), ("updated", C.c_uint32),
                ("interpolated", C.c_uint32), ("reserved_", C.c_uint32 * 2)]


TSDF_SHIFT_ENTRY_POINTS = ("adc_tsdf_shift_device", "adc_tsdf_shift", "adc_get_tsdf_shift_report", "adc_tsdf_get_offset", "adc_tsdf_follow_plan")
TSDF_SHIFT_MAX_OFFSET = 1 << 24  # the largest |total offset| of a volume, in voxels


class TsdfShiftParams(C.Structure):
    """adc_tsdf_shift_params: the shift in voxels (the window moves by +shift in the world), min_weight in [1, 65535] of the leaving
    surface points; flags and the reserved words 0."""
    _fields_ = [("shift", C.c_int32 * 3), ("min_weight", C.c_uint32), ("flags", C.c_uint32), ("reserved_", C.c_uint32 * 3)]

    def __init__(self, shift=(0, 0, 0), min_weight=1, flags=0):
        super().__init__()
        self.shift = (C.c_int32 * 3)(*[int(v) for v in shift])
        self.min_weight, self.flags = int(min_weight), int(flags)


class TsdfShiftReport(C.Structure):
    """adc_tsdf_shift_report: voxels that stayed with a voxel word other than 0; leaving voxels with one; leaving voxels with
    w >= min_weight; leaving surface points whatever the capacity."""
    _fields_ = [("moved_nonempty", C.c_uint32), ("left_nonempty", C.c_uint32), ("left_seen", C.c_uint32), ("points", C.c_uint32), ("reserved_", C.c_uint32 * 4)]


class TsdfFollowParams(C.Structure):
    """adc_tsdf_follow_params: the camera-frame point that should stay near the volume's centre, the distance in voxels it may stray
    (margin >= 0) and the step of a shift (quantum >= 1); the reserved words 0."""
    _fields_ = [("anchor", C.c_float * 3), ("margin", C.c_int32), ("quantum", C.c_int32), ("reserved_", C.c_uint32 * 3)]

    def __init__(self, anchor=(0.0, 0.0, 2.5), margin=8, quantum=4):
        super().__init__()
        self.anchor = (C.c_float * 3)(*[float(v) for v in anchor])
        self.margin, self.quantum = int(margin), int(quantum)


def tsdf_follow_plan(params, R, t, follow=None):
    """How far to shift so that the anchor of a pose stays near the volume's centre (adc_tsdf_follow_plan; pure: no handle, no device).
    params a TsdfParams with the CURRENT origin; R (9, row-major) and t (3) take a world point into the camera frame; follow a
    TsdfFollowParams or None for the defaults.  Returns (sx, sy, sz).  Raises when refused."""
    f = TsdfFollowParams() if follow is None else follow
    Rc = (C.c_float * 9)(*[float(v) for v in R])
    tc = (C.c_float * 3)(*[float(v) for v in t])
    out = (C.c_int32 * 3)()
    if lib().adc_tsdf_follow_plan(C.byref(params), Rc, tc, C.byref(f), out) != 0:
        raise ValueError("adc_tsdf_follow_plan refused: " + last_error())
    return tuple(out)


TSDF_MESH_ENTRY_POINTS = ("adc_tsdf_mesh_device", "adc_tsdf_mesh", "adc_get_tsdf_mesh_report")


class TsdfMeshReport(C.Structure):
    """adc_tsdf_mesh_report: voxels with w >= min_weight; vertices (the crossings) and triangles whatever the capacities; cells whose
    eight corners are seen, and those of them that emit at least one triangle."""
    _fields_ = [("voxels_seen", C.c_uint32), ("vertices", C.c_uint32), ("triangles", C.c_uint32), ("cells_seen", C.c_uint32), ("cells_surface", C.c_uint32),
                ("reserved_", C.c_uint32 * 3)]


TSDF_RAYCAST_ENTRY_POINTS = ("adc_tsdf_raycast_device", "adc_tsdf_raycast", "adc_get_tsdf_raycast_report")
TSDF_RAY_MISS, TSDF_RAY_HIT, TSDF_RAY_NO_SURFACE, TSDF_RAY_BEHIND, TSDF_RAY_EXHAUSTED = range(5)  # ADC_TSDF_RAY_*


class TsdfRaycastParams(C.Structure):
    """adc_tsdf_raycast_params: the view (width, height in [1, 8192], focal_px, cx, cy; R row-major and t take a WORLD point into the
    camera frame, as in TsdfFrame), the range z_near < z_far of camera depth, the advance `step` between samples and `skip` (>= step)
    behind a sample in saturated free space, min_weight in [1, 65535], max_steps in [1, 16384] (no ray takes more samples); flags and
    the reserved words 0.  Defaults: R = I, t = 0, skip = step."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("focal_px", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("R", C.c_float * 9),
                ("t", C.c_float * 3), ("z_near", C.c_float), ("z_far", C.c_float), ("step", C.c_float), ("skip", C.c_float), ("min_weight", C.c_uint32),
                ("max_steps", C.c_uint32), ("flags", C.c_uint32), ("reserved_", C.c_uint32 * 8)]

    def __init__(self, width=0, height=0, focal_px=0.0, cx=0.0, cy=0.0, R=None, t=None, z_near=0.0, z_far=0.0, step=0.0, skip=None, min_weight=1,
                 max_steps=4096, flags=0):
        super().__init__()
        self.width, self.height, self.focal_px, self.cx, self.cy = int(width), int(height), float(focal_px), float(cx), float(cy)
        self.R = (C.c_float * 9)(*[float(x) for x in np.asarray((1, 0, 0, 0, 1, 0, 0, 0, 1) if R is None else R, np.float32).ravel()])
        self.t = (C.c_float * 3)(*[float(x) for x in np.asarray((0, 0, 0) if t is None else t, np.float32).ravel()])
        self.z_near, self.z_far, self.step, self.skip = float(z_near), float(z_far), float(step), float(step if skip is None else skip)
        self.min_weight, self.max_steps, self.flags = int(min_weight), int(max_steps), int(flags)


class TsdfRaycastReport(C.Structure):
    """adc_tsdf_raycast_report: rays = width * height and how many of them ended with each status (they sum to rays); the number of
    samples of all rays as two 32-bit halves (`samples` joins them)."""
    _fields_ = [("rays", C.c_uint32), ("miss", C.c_uint32), ("hit", C.c_uint32), ("no_surface", C.c_uint32), ("behind", C.c_uint32), ("exhausted", C.c_uint32),
                ("samples_lo", C.c_uint32), ("samples_hi", C.c_uint32), ("reserved_", C.c_uint32 * 8)]

    @property
    def samples(self):
        return self.samples_lo | (self.samples_hi << 32)


TRACK_ENTRY_POINTS = ("adc_track_device", "adc_tsdf_track", "adc_get_track_result")
TRACK_CONVERGED, TRACK_MAX_ITERATIONS, TRACK_LOST, TRACK_DEGENERATE, TRACK_DIVERGED = range(5)  # ADC_TRACK_*
TRACK_MAX_ITERATIONS_LIMIT = 32


class TrackParams(C.Structure):
    """adc_track_params: iterations in [1, 32], stride in [1, 16], the distance gate max_dist (> 0), the angle gate min_cos in [-1, 1],
    z_far (> 0: the farthest depth that takes part and the scale of the rotation columns), min_pixels >= 6, the convergence thresholds
    eps_rot / eps_trans, the largest admissible step max_rot / max_trans, damping >= 0 (times the diagonal), pivot_ratio in [0, 1);
    flags and the reserved words 0.  The defaults are those of a NULL pointer: API defaults, not measured optima."""
    _fields_ = [("iterations", C.c_uint32), ("stride", C.c_uint32), ("max_dist", C.c_float), ("min_cos", C.c_float), ("z_far", C.c_float), ("min_pixels", C.c_uint32),
                ("eps_rot", C.c_float), ("eps_trans", C.c_float), ("max_rot", C.c_float), ("max_trans", C.c_float), ("damping", C.c_float), ("pivot_ratio", C.c_float),
                ("flags", C.c_uint32), ("reserved_", C.c_uint32 * 3)]

    def __init__(self, iterations=10, stride=1, max_dist=0.1, min_cos=0.8, z_far=8.0, min_pixels=64, eps_rot=1.0e-5, eps_trans=1.0e-5, max_rot=0.5, max_trans=0.5,
                 damping=0.0, pivot_ratio=1.0e-6, flags=0):
        super().__init__()
        self.iterations, self.stride, self.min_pixels, self.flags = int(iterations), int(stride), int(min_pixels), int(flags)
        self.max_dist, self.min_cos, self.z_far = float(max_dist), float(min_cos), float(z_far)
        self.eps_rot, self.eps_trans, self.max_rot, self.max_trans = float(eps_rot), float(eps_trans), float(max_rot), float(max_trans)
        self.damping, self.pivot_ratio = float(damping), float(pivot_ratio)


class TrackIteration(C.Structure):
    """adc_track_iteration: the used pixels, the rms residual and the norms of the step's rotation and translation of one solve"""
    _fields_ = [("used", C.c_uint32), ("rms", C.c_float), ("rot", C.c_float), ("trans", C.c_float)]


class TrackResult(C.Structure):
    """adc_track_result: status (TRACK_*), the number of solves run, the last accepted pose R (row-major) / t, world -> camera, ready
    for a TsdfFrame; the eight counts of the last reduce pass (the seven behind `pixels` sum to it); H (6 x 6, row-major) and b of the
    last solve, twist order rotation then translation, model camera frame; one TrackIteration per solve run."""
    _fields_ = [("status", C.c_uint32), ("solves", C.c_uint32), ("R", C.c_float * 9), ("t", C.c_float * 3), ("pixels", C.c_uint32), ("no_depth", C.c_uint32),
                ("outside", C.c_uint32), ("no_model", C.c_uint32), ("too_far", C.c_uint32), ("angle", C.c_uint32), ("out_of_range", C.c_uint32), ("used", C.c_uint32),
                ("H", C.c_double * 36), ("b", C.c_double * 6), ("iteration", TrackIteration * TRACK_MAX_ITERATIONS_LIMIT), ("reserved_", C.c_uint32 * 6)]


VOXEL_POSE = 0x1  # ADC_VOXEL_POSE: R, t of a VoxelGrid take the camera-frame point into the frame of the grid


class VoxelGrid(C.Structure):
    """adc_voxel_grid: leaf (edge of a voxel, unit of the calibration's baseline), the crop z_min <= Z <= z_max of the camera-frame Z,
    flags (VOXEL_POSE), and the pose R (row-major) / t looked at only with the flag."""
    _fields_ = [("leaf", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float), ("flags", C.c_uint32), ("R", C.c_float * 9),
                ("t", C.c_float * 3), ("reserved_", C.c_uint32 * 4)]

    def __init__(self, leaf=0.0, z_min=0.0, z_max=float("inf"), pose=None):
        """pose: None, or (R, t) with R 3x3 (or 9 numbers, row-major) and t 3 numbers."""
        super().__init__()
        self.leaf, self.z_min, self.z_max = float(leaf), float(z_min), float(z_max)
        self.R[0] = self.R[4] = self.R[8] = 1.0
        if pose is not None:
            R, t = pose
            self.R = (C.c_float * 9)(*[float(x) for x in np.asarray(R, np.float32).ravel()])
            self.t = (C.c_float * 3)(*[float(x) for x in np.asarray(t, np.float32).ravel()])
            self.flags = VOXEL_POSE


class VoxelReport(C.Structure):
    """adc_voxel_report: cloud-valid pixels, points kept after crop and range, voxels."""
    _fields_ = [("points_valid", C.c_uint32), ("points_kept", C.c_uint32), ("voxels", C.c_uint32)]


POINT_DTYPE = np.dtype({"names": ["x", "y", "z", "r", "g", "b", "pad"], "formats": ["<f4", "<f4", "<f4", "u1", "u1", "u1", "u1"],
                        "offsets": [0, 4, 8, 12, 13, 14, 15], "itemsize": 16})


def _calib(calib):
    """None, a Calib, or a sequence (focal_px, baseline, cx, cy, doffs) -> Calib or None."""
    if calib is None or isinstance(calib, Calib):
        return calib
    return Calib(*[float(v) for v in calib])


def _outputs(calib, depth, cloud, capacity, cloud_count, disp8):
    c = _calib(calib)
    req = Outputs(C.pointer(c) if c is not None else None, depth, cloud, int(capacity), cloud_count, disp8)
    req._keep = c
    return req


_lib = None


def lib():
    """Loads the C-ABI library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("HIP library missing: %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, u8p = C.c_void_p, C.c_int32, C.c_void_p
    L.adc_option_default.argtypes = [C.POINTER(ADCensusOption)]
    L.adc_option_default.restype = None
    L.adc_device_count.restype = C.c_int
    L.adc_version.restype = C.c_char_p
    L.adc_last_error.restype = C.c_char_p
    L.adc_create.argtypes = [i32, i32, C.POINTER(ADCensusOption), C.c_int]
    L.adc_create.restype = vp
    L.adc_destroy.argtypes = [vp]
    L.adc_destroy.restype = None
    for name in ("adc_match", "adc_match_async"):
        getattr(L, name).argtypes = [vp, u8p, u8p, vp]
        getattr(L, name).restype = C.c_int
    L.adc_match_device.argtypes = [vp, vp, vp, vp]
    L.adc_match_device.restype = C.c_int
    if hasattr(L, "adc_match_ex"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_match_ex.argtypes = [vp, u8p, u8p, vp, vp, vp]
        L.adc_match_ex.restype = C.c_int
        L.adc_match_device_ex.argtypes = [vp, vp, vp, vp, vp, vp]
        L.adc_match_device_ex.restype = C.c_int
    if hasattr(L, "adc_match_out"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_match_out.argtypes = [vp, u8p, u8p, vp, C.POINTER(Outputs)]
        L.adc_match_out.restype = C.c_int
        L.adc_match_device_out.argtypes = [vp, vp, vp, vp, C.POINTER(Outputs)]
        L.adc_match_device_out.restype = C.c_int
        L.adc_reproject_device.argtypes = [vp, vp, vp, C.POINTER(Outputs)]
        L.adc_reproject_device.restype = C.c_int
        L.adc_get_cloud_count.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.adc_get_cloud_count.restype = C.c_int
    if hasattr(L, "adc_match_products"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        for name in ("adc_match_products", "adc_match_async_products", "adc_match_device_products"):
            getattr(L, name).argtypes = [vp, vp, vp, vp, C.POINTER(Products)]
            getattr(L, name).restype = C.c_int
        L.adc_farm_submit_products.argtypes = [vp, u8p, u8p, vp, C.POINTER(Products), C.POINTER(C.c_uint64)]
        L.adc_farm_submit_products.restype = C.c_int
        L.adc_disp16_device.argtypes = [vp, vp, C.c_float, vp]
        L.adc_disp16_device.restype = C.c_int
    if hasattr(L, "adc_set_speckle_filter"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_set_speckle_filter.argtypes = [vp, i32, C.c_float]
        L.adc_set_speckle_filter.restype = C.c_int
        L.adc_filter_speckles_device.argtypes = [vp, vp, i32, C.c_float, vp]
        L.adc_filter_speckles_device.restype = C.c_int
        L.adc_get_speckle_stats.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.adc_get_speckle_stats.restype = C.c_int
        L.adc_farm_set_speckle_filter.argtypes = [vp, i32, C.c_float]
        L.adc_farm_set_speckle_filter.restype = C.c_int
    if hasattr(L, "adc_set_rectify_maps"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        for prefix in ("adc_", "adc_farm_"):
            getattr(L, prefix + "set_rectify_maps").argtypes = [vp, C.c_int, C.POINTER(RawFormat), vp, vp]
            getattr(L, prefix + "set_rectify_model").argtypes = [vp, C.c_int, C.POINTER(RawFormat), C.POINTER(CameraModel)]
            getattr(L, prefix + "clear_rectify").argtypes = [vp]
            for name in ("set_rectify_maps", "set_rectify_model", "clear_rectify"):
                getattr(L, prefix + name).restype = C.c_int
        if hasattr(L, "adc_set_input_format"):
            for name in ("adc_set_input_format", "adc_farm_set_input_format"):
                getattr(L, name).argtypes = [vp, C.c_int, C.POINTER(RawFormat)]
                getattr(L, name).restype = C.c_int
        L.adc_get_rectify_maps.argtypes = [vp, C.c_int, vp, vp, vp]
        L.adc_get_rectify_maps.restype = C.c_int
        L.adc_rectify_device.argtypes = [vp, C.c_int, vp, vp]
        L.adc_rectify_device.restype = C.c_int
    if hasattr(L, "adc_set_ground_truth"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_set_ground_truth.argtypes = [vp, C.POINTER(GroundTruth), C.POINTER(GroundTruth), vp, C.c_float]
        L.adc_clear_ground_truth.argtypes = [vp]
        L.adc_evaluate_device.argtypes = [vp, vp, vp, vp, C.POINTER(EvalParams), vp, vp]
        L.adc_evaluate.argtypes = [vp, vp, vp, vp, C.POINTER(EvalParams), vp, vp, C.POINTER(EvalReport)]
        L.adc_get_eval_report.argtypes = [vp, C.POINTER(EvalReport)]
        for name in ("adc_set_ground_truth", "adc_clear_ground_truth", "adc_evaluate_device", "adc_evaluate", "adc_get_eval_report"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "adc_set_register_target"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_set_register_target.argtypes = [vp, C.POINTER(RegTarget)]
        L.adc_clear_register_target.argtypes = [vp]
        L.adc_register_depth_device.argtypes = [vp, vp, C.c_int, C.POINTER(Calib), C.c_uint32, vp, vp]
        L.adc_align_color_device.argtypes = [vp, vp, C.c_int, C.POINTER(Calib), vp, vp, vp]
        L.adc_register_depth.argtypes = [vp, vp, C.c_int, C.POINTER(Calib), C.c_uint32, vp, vp, C.POINTER(RegReport)]
        L.adc_align_color.argtypes = [vp, vp, C.c_int, C.POINTER(Calib), vp, vp, vp]
        L.adc_get_register_report.argtypes = [vp, C.POINTER(RegReport)]
        for name in ("adc_set_register_target", "adc_clear_register_target", "adc_register_depth_device", "adc_align_color_device",
                     "adc_register_depth", "adc_align_color", "adc_get_register_report"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "adc_normals_device"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_normals_device.argtypes = [vp, vp, C.POINTER(Calib), C.POINTER(NormalsParams), vp, vp]
        L.adc_normals.argtypes = [vp, vp, C.POINTER(Calib), C.POINTER(NormalsParams), vp, vp, C.POINTER(NormalsReport)]
        L.adc_get_normals_report.argtypes = [vp, C.POINTER(NormalsReport)]
        for name in ("adc_normals_device", "adc_normals", "adc_get_normals_report"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "adc_mesh_device"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_mesh_device.argtypes = [vp, vp, vp, C.POINTER(Calib), C.POINTER(MeshParams), vp, C.c_uint64, vp, vp, C.c_uint64, vp]
        L.adc_mesh.argtypes = [vp, vp, vp, C.POINTER(Calib), C.POINTER(MeshParams), vp, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(MeshReport)]
        L.adc_get_mesh_report.argtypes = [vp, C.POINTER(MeshReport)]
        for name in ("adc_mesh_device", "adc_mesh", "adc_get_mesh_report"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "adc_tsdf_create"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_tsdf_create.argtypes = [vp, C.POINTER(TsdfParams)]
        L.adc_tsdf_reset.argtypes = [vp]
        L.adc_tsdf_destroy.argtypes = [vp]
        L.adc_tsdf_integrate_device.argtypes = [vp, vp, vp, C.POINTER(TsdfFrame)]
        L.adc_tsdf_integrate.argtypes = [vp, vp, vp, C.POINTER(TsdfFrame), C.POINTER(TsdfReport)]
        L.adc_tsdf_extract_device.argtypes = [vp, C.POINTER(TsdfExtractParams), vp, C.c_uint64, vp]
        L.adc_tsdf_extract.argtypes = [vp, C.POINTER(TsdfExtractParams), vp, C.c_uint64, C.POINTER(TsdfExtractReport)]
        L.adc_get_tsdf_report.argtypes = [vp, C.POINTER(TsdfReport), C.POINTER(TsdfExtractReport)]
        L.adc_tsdf_get_volume_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(TsdfParams)]
        L.adc_tsdf_download.argtypes = [vp, vp, vp]
        L.adc_tsdf_upload.argtypes = [vp, vp, vp]
    if hasattr(L, "adc_tsdf_mesh_device"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_tsdf_mesh_device.argtypes = [vp, C.POINTER(TsdfExtractParams), vp, C.c_uint64, vp, C.c_uint64, vp]
        L.adc_tsdf_mesh.argtypes = [vp, C.POINTER(TsdfExtractParams), vp, C.c_uint64, vp, C.c_uint64, C.POINTER(TsdfMeshReport)]
        L.adc_get_tsdf_mesh_report.argtypes = [vp, C.POINTER(TsdfMeshReport)]
        for name in TSDF_ENTRY_POINTS:
            getattr(L, name).restype = C.c_int
    if hasattr(L, "adc_tsdf_raycast_device"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_tsdf_raycast_device.argtypes = [vp, C.POINTER(TsdfRaycastParams), vp, vp, vp, vp]
        L.adc_tsdf_raycast.argtypes = [vp, C.POINTER(TsdfRaycastParams), vp, vp, vp, vp, C.POINTER(TsdfRaycastReport)]
        L.adc_get_tsdf_raycast_report.argtypes = [vp, C.POINTER(TsdfRaycastReport)]
        for name in TSDF_RAYCAST_ENTRY_POINTS:
            getattr(L, name).restype = C.c_int
    if hasattr(L, "adc_tsdf_fuse_device"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_tsdf_weights_device.argtypes = [vp, vp, vp, vp, C.POINTER(TsdfFrame), C.POINTER(TsdfWeightParams), vp]
        L.adc_tsdf_weights.argtypes = [vp, vp, vp, vp, C.POINTER(TsdfFrame), C.POINTER(TsdfWeightParams), vp, C.POINTER(TsdfWeightReport)]
        L.adc_tsdf_fuse_device.argtypes = [vp, vp, vp, vp, C.POINTER(TsdfFrame), C.POINTER(TsdfFuseParams)]
        L.adc_tsdf_fuse.argtypes = [vp, vp, vp, vp, C.POINTER(TsdfFrame), C.POINTER(TsdfFuseParams), C.POINTER(TsdfFuseReport)]
        L.adc_get_tsdf_fuse_report.argtypes = [vp, C.POINTER(TsdfFuseReport), C.POINTER(TsdfWeightReport)]
        for name in TSDF_FUSE_ENTRY_POINTS:
            getattr(L, name).restype = C.c_int
    if hasattr(L, "adc_tsdf_shift_device"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_tsdf_shift_device.argtypes = [vp, C.POINTER(TsdfShiftParams), vp, C.c_uint64, vp]
        L.adc_tsdf_shift.argtypes = [vp, C.POINTER(TsdfShiftParams), vp, C.c_uint64, C.POINTER(TsdfShiftReport)]
        L.adc_get_tsdf_shift_report.argtypes = [vp, C.POINTER(TsdfShiftReport)]
        L.adc_tsdf_get_offset.argtypes = [vp, C.POINTER(C.c_int32 * 3), C.POINTER(C.c_float * 3)]
        L.adc_tsdf_follow_plan.argtypes = [C.POINTER(TsdfParams), C.POINTER(C.c_float * 9), C.POINTER(C.c_float * 3), C.POINTER(TsdfFollowParams), C.POINTER(C.c_int32 * 3)]
        for name in TSDF_SHIFT_ENTRY_POINTS:
            getattr(L, name).restype = C.c_int
    if hasattr(L, "adc_track_device"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_track_device.argtypes = [vp, vp, vp, C.POINTER(TsdfFrame), C.POINTER(TsdfRaycastParams), vp, vp, C.POINTER(TrackParams), vp]
        L.adc_tsdf_track.argtypes = [vp, vp, C.POINTER(TsdfFrame), C.POINTER(TrackParams), C.POINTER(TrackResult)]
        L.adc_get_track_result.argtypes = [vp, C.POINTER(TrackResult)]
        for name in TRACK_ENTRY_POINTS:
            getattr(L, name).restype = C.c_int
    if hasattr(L, "adc_set_cloud_voxel_grid"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_set_cloud_voxel_grid.argtypes = [vp, C.POINTER(VoxelGrid)]
        L.adc_clear_cloud_voxel_grid.argtypes = [vp]
        L.adc_get_voxel_report.argtypes = [vp, C.POINTER(VoxelReport)]
        L.adc_farm_set_cloud_voxel_grid.argtypes = [vp, C.POINTER(VoxelGrid)]
        for name in ("adc_set_cloud_voxel_grid", "adc_clear_cloud_voxel_grid", "adc_get_voxel_report", "adc_farm_set_cloud_voxel_grid"):
            getattr(L, name).restype = C.c_int
    L.adc_wait.argtypes = [vp]
    L.adc_wait.restype = C.c_int
    L.adc_stage_name.argtypes = [C.c_int]
    L.adc_stage_name.restype = C.c_char_p
    L.adc_set_profiling.argtypes = [vp, C.c_int]
    L.adc_set_profiling.restype = None
    L.adc_set_verbose.argtypes = [vp, C.c_int]
    L.adc_set_verbose.restype = None
    L.adc_get_stage_ms.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
    L.adc_get_stage_ms.restype = C.c_int
    L.adc_get_aggregate_pass_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.adc_get_aggregate_pass_ms.restype = C.c_int
    L.adc_get_aggregate_info.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.adc_get_aggregate_info.restype = C.c_int
    L.adc_get_aggregate_kernel.argtypes = [vp]
    L.adc_get_aggregate_kernel.restype = C.c_char_p
    L.adc_host_register.argtypes = [vp, C.c_size_t]
    L.adc_host_register.restype = C.c_int
    L.adc_host_unregister.argtypes = [vp]
    L.adc_host_unregister.restype = C.c_int
    L.adc_set_paper_modes.argtypes = [vp, C.c_uint32]
    L.adc_set_paper_modes.restype = C.c_int
    L.adc_get_stream.argtypes = [vp]
    L.adc_get_stream.restype = vp
    L.adc_device_synchronize.restype = C.c_int
    L.adc_device_malloc.argtypes = [C.c_size_t]
    L.adc_device_malloc.restype = vp
    L.adc_device_free.argtypes = [vp]
    L.adc_device_free.restype = None
    L.adc_memcpy_h2d.argtypes = [vp, vp, C.c_size_t]
    L.adc_memcpy_h2d.restype = C.c_int
    L.adc_memcpy_d2h.argtypes = [vp, vp, C.c_size_t]
    L.adc_memcpy_d2h.restype = C.c_int
    L.adc_device_copy_ms.argtypes = [vp, vp, C.c_size_t, C.c_int]
    L.adc_device_copy_ms.restype = C.c_double
    if hasattr(L, "adc_device_copy_kernel_ms"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_device_copy_kernel_ms.argtypes = [vp, vp, C.c_size_t, C.c_int]
        L.adc_device_copy_kernel_ms.restype = C.c_double
    L.adc_debug_read.argtypes = [vp, C.c_int, vp]
    L.adc_debug_read.restype = C.c_int
    L.adc_debug_write.argtypes = [vp, C.c_int, vp]
    L.adc_debug_write.restype = C.c_int
    L.adc_debug_set_images.argtypes = [vp, u8p, u8p]
    L.adc_debug_set_images.restype = C.c_int
    L.adc_debug_run.argtypes = [vp, C.c_int, C.c_int]
    L.adc_debug_run.restype = C.c_int
    if hasattr(L, "adc_debug_read_itp_code"):  # (absent from A/B builds of older revisions, ADC_HIP_LIB)
        L.adc_debug_itp_code_geometry.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.adc_debug_itp_code_geometry.restype = C.c_int
        L.adc_debug_read_itp_code.argtypes = [vp, C.c_int, vp]
        L.adc_debug_read_itp_code.restype = C.c_int
    L.adc_farm_create.argtypes = [i32, i32, C.POINTER(ADCensusOption), C.c_int, C.c_int]
    L.adc_farm_create.restype = vp
    L.adc_farm_destroy.argtypes = [vp]
    L.adc_farm_destroy.restype = None
    L.adc_farm_submit.argtypes = [vp, u8p, u8p, vp, C.POINTER(C.c_uint64)]
    L.adc_farm_submit.restype = C.c_int
    L.adc_farm_wait.argtypes = [vp, C.c_uint64]
    L.adc_farm_wait.restype = C.c_int
    L.adc_farm_drain.argtypes = [vp]
    L.adc_farm_drain.restype = C.c_int64
    L.adc_debug_counter.argtypes = [vp, C.c_int]
    L.adc_debug_counter.restype = C.c_int64
    L.adc_debug_voting_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.adc_debug_voting_stats.restype = C.c_int
    _lib = L
    return L


def device_count():
    return lib().adc_device_count()


def last_error():
    return lib().adc_last_error().decode()


def host_register(arr):
    """Page-locks a numpy array for DMA straight from / to it (adc_host_register); call host_unregister before it dies."""
    if lib().adc_host_register(arr.ctypes.data, arr.nbytes) != 0:
        raise RuntimeError("adc_host_register failed: " + last_error())


def host_unregister(arr):
    lib().adc_host_unregister(arr.ctypes.data)


def _img(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a


def _maps(map_x, map_y, width, height):
    mx, my = np.ascontiguousarray(map_x, dtype=np.float32), np.ascontiguousarray(map_y, dtype=np.float32)
    assert mx.shape == (height, width) and my.shape == (height, width), (mx.shape, my.shape, (height, width))
    return mx, my


class _RectifyState:
    """What a Python object remembers of the rectification it has set: the raw geometry per side, for the size asserts of its
    entry points (the library keeps the real state)."""

    def __init__(self):
        self.raw = [None, None]

    def set(self, side, raw):
        self.raw[int(side)] = RawFormat(raw.width, raw.height, raw.pitch_bytes, raw.format)

    def clear(self):
        self.raw = [None, None]

    def on(self):
        return self.raw[0] is not None and self.raw[1] is not None

    def sizes(self, plain):
        """bytes the left / right image argument of a match must have"""
        return (self.raw[0].nbytes, self.raw[1].nbytes) if self.on() else (plain, plain)


class PreviousPairFailed(RuntimeError):
    """adc_farm_submit returned ADC_FARM_PREVIOUS_FAILED: the pair that occupied the pipeline before (`failed_ticket`) failed
    while it was collected; the NEW pair is in flight all the same and `ticket` is its ticket."""

    def __init__(self, ticket, failed_ticket, message):
        RuntimeError.__init__(self, message)
        self.ticket, self.failed_ticket = int(ticket), int(failed_ticket)


class PairFarm:
    """Persistent farm of `pipelines` matchers of one geometry on one device (adc_farm_* of the C ABI): submit() enqueues
    a whole Match asynchronously from host buffers, results land in the caller's arrays in submission order."""

    def __init__(self, width, height, option, device=-1, pipelines=3):
        self.width, self.height = int(width), int(height)
        self.pipelines = int(pipelines)
        self._f = lib().adc_farm_create(self.width, self.height, C.byref(option), int(device), int(pipelines))
        if not self._f:
            raise RuntimeError("adc_farm_create failed: " + last_error())
        self._keep = {}
        self._rect = _RectifyState()

    def submit(self, img_left, img_right, disp_left, products=None):
        """products: a Products with HOST addresses (Products.from_arrays) or None; its arrays are delivered with the map, in
        submission order (adc_farm_submit_products), and are kept alive until then."""
        l, r = _img(img_left), _img(img_right)
        assert (l.size, r.size) == self._rect.sizes(self.width * self.height * 3)
        assert disp_left.dtype == np.float32 and disp_left.flags["C_CONTIGUOUS"] and disp_left.size == self.width * self.height
        t = C.c_uint64(0)
        if products is None:
            rc = lib().adc_farm_submit(self._f, l.ctypes.data, r.ctypes.data, disp_left.ctypes.data, C.byref(t))
        else:
            assert products.sizes_ok(self.width * self.height)
            rc = lib().adc_farm_submit_products(self._f, l.ctypes.data, r.ctypes.data, disp_left.ctypes.data, C.byref(products), C.byref(t))
        if rc not in (0, 3):
            raise RuntimeError("adc_farm_submit failed (%d): %s" % (rc, last_error()))
        ticket = int(t.value)
        self._keep[ticket] = (disp_left, products)  # the output arrays must stay alive until the pair is delivered
        self._keep.pop(ticket - self.pipelines, None)  # submit() has just delivered the pair that held this pipeline before
        if rc == 3:  # ADC_FARM_PREVIOUS_FAILED: the new pair IS in flight (ticket), the pipeline's previous pair failed
            raise PreviousPairFailed(ticket, ticket - self.pipelines, "adc_farm_submit: " + last_error())
        return ticket

    def wait(self, ticket):
        if lib().adc_farm_wait(self._f, int(ticket)) != 0:
            raise RuntimeError("adc_farm_wait failed: " + last_error())
        self._keep.pop(int(ticket), None)

    def drain(self):
        n = int(lib().adc_farm_drain(self._f))
        if n < 0:
            raise RuntimeError("adc_farm_drain failed: " + last_error())
        self._keep.clear()
        return n

    def set_speckle_filter(self, max_size, max_diff):
        """The speckle filter of ADCensusStereo.set_speckle_filter on every pipeline (adc_farm_set_speckle_filter); drain() first."""
        if lib().adc_farm_set_speckle_filter(self._f, int(max_size), float(max_diff)) != 0:
            raise RuntimeError("adc_farm_set_speckle_filter failed: " + last_error())

    def set_cloud_voxel_grid(self, leaf, z_min=0.0, z_max=float("inf"), pose=None):
        """The voxel grid of ADCensusStereo.set_cloud_voxel_grid on every pipeline (adc_farm_set_cloud_voxel_grid); leaf=None clears
        it; drain() first."""
        grid = None if leaf is None else VoxelGrid(leaf, z_min, z_max, pose)
        if lib().adc_farm_set_cloud_voxel_grid(self._f, None if grid is None else C.byref(grid)) != 0:
            raise RuntimeError("adc_farm_set_cloud_voxel_grid failed: " + last_error())

    def set_rectify_maps(self, side, raw, map_x, map_y):
        """ADCensusStereo.set_rectify_maps on every pipeline (adc_farm_set_rectify_maps); drain() first."""
        mx, my = _maps(map_x, map_y, self.width, self.height)
        if lib().adc_farm_set_rectify_maps(self._f, int(side), C.byref(raw), mx.ctypes.data, my.ctypes.data) != 0:
            raise RuntimeError("adc_farm_set_rectify_maps failed: " + last_error())
        self._rect.set(side, raw)

    def set_rectify_model(self, side, raw, model):
        """ADCensusStereo.set_rectify_model on every pipeline (adc_farm_set_rectify_model); drain() first."""
        if lib().adc_farm_set_rectify_model(self._f, int(side), C.byref(raw), C.byref(model)) != 0:
            raise RuntimeError("adc_farm_set_rectify_model failed: " + last_error())
        self._rect.set(side, raw)

    def set_input_format(self, side, raw):
        """ADCensusStereo.set_input_format on every pipeline (adc_farm_set_input_format); drain() first."""
        if lib().adc_farm_set_input_format(self._f, int(side), C.byref(raw)) != 0:
            raise RuntimeError("adc_farm_set_input_format failed: " + last_error())
        self._rect.set(side, raw)

    def clear_rectify(self):
        if lib().adc_farm_clear_rectify(self._f) != 0:
            raise RuntimeError("adc_farm_clear_rectify failed: " + last_error())
        self._rect.clear()

    def close(self):
        if self._f:
            lib().adc_farm_destroy(self._f)
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ADCensusStereo:
    """Mirror of class ADCensusStereo (ADCensusStereo.h:14-41).

    Initialize(width, height, option) -> bool ; Match(img_left, img_right, disp_left) -> bool ;
    Reset(width, height, option) -> bool.  Images: uint8 [H][W][3] BGR; disp_left: float32 [H][W],
    caller-allocated, filled in place.
    """

    def __init__(self, device=-1):
        self._h = None
        self._device = device
        self.width = self.height = 0
        self.option = None
        self._rect = _RectifyState()

    # -- lifetime ------------------------------------------------------------------------------
    def Initialize(self, width, height, option):
        self.Release()
        self.width, self.height, self.option = int(width), int(height), option
        h = lib().adc_create(int(width), int(height), C.byref(option), int(self._device))
        self._h = h
        self._rect.clear()  # (a new handle: rectification is off)
        return bool(h)

    def Reset(self, width, height, option):
        self.Release()
        return self.Initialize(width, height, option)

    def Release(self):
        if self._h:
            lib().adc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.Release()
        except Exception:
            pass

    @property
    def is_initialized(self):
        return bool(self._h)

    @property
    def disp_range(self):
        return self.option.max_disparity - self.option.min_disparity

    # -- the drop-in path ----------------------------------------------------------------------
    def Match(self, img_left, img_right, disp_left):
        if not self._h:
            return False  # ADCensusStereo.cpp:71-73
        if img_left is None or img_right is None or disp_left is None:
            return False  # :74-76
        l, r = _img(img_left), _img(img_right)
        assert (l.size, r.size) == self._rect.sizes(self.width * self.height * 3)  # (rectification on: the raw sizes)
        assert disp_left.dtype == np.float32 and disp_left.flags["C_CONTIGUOUS"] and disp_left.size == self.width * self.height
        return lib().adc_match(self._h, l.ctypes.data, r.ctypes.data, disp_left.ctypes.data) == 0

    def match(self, img_left, img_right):
        """Convenience: returns a new float32 [H][W] map; raises on failure."""
        d = np.empty((self.height, self.width), dtype=np.float32)
        if not self.Match(img_left, img_right, d):
            raise RuntimeError("Match failed: " + last_error())
        return d

    # -- additive API --------------------------------------------------------------------------
    def _match_args(self, img_left, img_right, disp_left):
        """what MatchEx / MatchOut / MatchProducts check first: None where Match returns False, else (left, right, pixels)"""
        if not self._h or img_left is None or img_right is None or disp_left is None:
            return None
        l, r = _img(img_left), _img(img_right)
        n = self.width * self.height
        assert (l.size, r.size) == self._rect.sizes(n * 3)
        assert disp_left.dtype == np.float32 and disp_left.flags["C_CONTIGUOUS"] and disp_left.size == n
        return l, r, n

    def MatchEx(self, img_left, img_right, disp_left, provenance=None, confidence=None):
        """Match plus the optional per-pixel maps (adc_match_ex): provenance uint8 [H][W] (code = lr | fill << 2, LR_* / FILL_*),
        confidence float32 [H][W]; either may be None (both None: exactly Match).  False where Match is, and on a handle with paper
        modes set when a map is requested."""
        args = self._match_args(img_left, img_right, disp_left)
        if args is None:
            return False
        l, r, n = args
        for a, dt in ((provenance, np.uint8), (confidence, np.float32)):
            assert a is None or (a.dtype == dt and a.flags["C_CONTIGUOUS"] and a.size == n)
        return lib().adc_match_ex(self._h, l.ctypes.data, r.ctypes.data, disp_left.ctypes.data,
                                  None if provenance is None else provenance.ctypes.data,
                                  None if confidence is None else confidence.ctypes.data) == 0

    def match_ex(self, img_left, img_right):
        """Convenience: returns new (disparity float32, provenance uint8, confidence float32) [H][W] maps; raises on failure."""
        shp = (self.height, self.width)
        d, p, c = np.empty(shp, np.float32), np.empty(shp, np.uint8), np.empty(shp, np.float32)
        if not self.MatchEx(img_left, img_right, d, p, c):
            raise RuntimeError("MatchEx failed: " + last_error())
        return d, p, c

    def match_device_ex(self, d_left, d_right, d_disp, d_provenance=None, d_confidence=None):
        """match_device plus the optional maps into the caller's device buffers (ints or None); asynchronous, call wait()."""
        return lib().adc_match_device_ex(self._h, d_left, d_right, d_disp, d_provenance, d_confidence) == 0

    def MatchOut(self, img_left, img_right, disp_left, calib=None, depth=None, cloud=None, disp8=None):
        """Match plus the outputs computed on the device from the final map (adc_match_out) into the caller's arrays: depth
        float32 [H][W] (needs calib), cloud a POINT_DTYPE array (its length is the capacity), disp8 uint8 [H][W]; any may be None
        (all None: exactly Match).  False where Match is, and when the request is refused; cloud_count() tells how many points are valid."""
        args = self._match_args(img_left, img_right, disp_left)
        if args is None:
            return False
        l, r, n = args
        for a, dt in ((depth, np.float32), (disp8, np.uint8)):
            assert a is None or (a.dtype == dt and a.flags["C_CONTIGUOUS"] and a.size == n)
        assert cloud is None or (cloud.dtype == POINT_DTYPE and cloud.flags["C_CONTIGUOUS"])
        req = _outputs(calib, None if depth is None else depth.ctypes.data, None if cloud is None else cloud.ctypes.data,
                       0 if cloud is None else cloud.size, None, None if disp8 is None else disp8.ctypes.data)
        return lib().adc_match_out(self._h, l.ctypes.data, r.ctypes.data, disp_left.ctypes.data, C.byref(req)) == 0

    def match_out(self, img_left, img_right, calib=None, depth=False, cloud=False, disp8=False):
        """Convenience: returns (disparity, depth, cloud, disp8) as new numpy arrays, None for what was not asked for; the cloud is a
        structured array with the adc_point layout (POINT_DTYPE), cut to the number of valid pixels.  Raises on failure."""
        shp = (self.height, self.width)
        d = np.empty(shp, np.float32)
        z = np.empty(shp, np.float32) if depth else None
        pts = np.empty(shp[0] * shp[1], POINT_DTYPE) if cloud else None
        g = np.empty(shp, np.uint8) if disp8 else None
        if not self.MatchOut(img_left, img_right, d, calib, z, pts, g):
            raise RuntimeError("MatchOut failed: " + last_error())
        if cloud:
            pts = pts[:self.cloud_count()].copy()
        return d, z, pts, g

    def match_device_out(self, d_left, d_right, d_disp, calib=None, d_depth=None, d_cloud=None, cloud_capacity=0, d_cloud_count=None,
                         d_disp8=None):
        """match_device plus the outputs into the caller's device buffers (ints or None; d_cloud_count: a uint32 device word);
        asynchronous, call wait(), then cloud_count()."""
        req = _outputs(calib, d_depth, d_cloud, cloud_capacity, d_cloud_count, d_disp8)
        return lib().adc_match_device_out(self._h, d_left, d_right, d_disp, C.byref(req)) == 0

    def reproject_device(self, d_disp, d_left, calib=None, d_depth=None, d_cloud=None, cloud_capacity=0, d_cloud_count=None, d_disp8=None):
        """The output kernels on any device-resident float32 [H][W] map of this geometry (adc_reproject_device), without a Match;
        asynchronous, call wait()."""
        req = _outputs(calib, d_depth, d_cloud, cloud_capacity, d_cloud_count, d_disp8)
        return lib().adc_reproject_device(self._h, d_disp, d_left, C.byref(req)) == 0

    # -- every product from one Match (adc_*_products) --------------------------------------------
    def MatchProducts(self, img_left, img_right, disp_left, products):
        """Match plus every product the request asks for (adc_match_products; a Products with HOST addresses, e.g. Products.from_arrays),
        synchronous.  None or an empty request: exactly Match.  False where Match is, and when the request is refused."""
        args = self._match_args(img_left, img_right, disp_left)
        if args is None:
            return False
        l, r, n = args
        assert products is None or products.sizes_ok(n)
        return lib().adc_match_products(self._h, l.ctypes.data, r.ctypes.data, disp_left.ctypes.data, None if products is None else C.byref(products)) == 0

    def _product_arrays(self, calib, provenance, confidence, depth, cloud, disp8, disp16_scale, cloud_capacity):
        shp = (self.height, self.width)
        new = lambda on, dt: np.empty(shp, dt) if on else None  # noqa: E731
        cap = shp[0] * shp[1] if cloud_capacity is None else int(cloud_capacity)
        return Products.from_arrays(new(provenance, np.uint8), new(confidence, np.float32), calib, new(depth, np.float32),
                                    np.empty(cap, POINT_DTYPE) if cloud else None, new(disp8, np.uint8), new(disp16_scale is not None, np.uint16),
                                    256.0 if disp16_scale is None else disp16_scale)

    @staticmethod
    def _product_dict(disp, req):
        """what a delivered request holds, as a dict of arrays (only what was asked for); the cloud is cut to the points written"""
        c, prov, conf, depth, cloud, disp8, disp16, count = req._keep
        out = {"disparity": disp}
        for name, a in (("provenance", prov), ("confidence", conf), ("depth", depth), ("disp8", disp8), ("disp16", disp16)):
            if a is not None:
                out[name] = a
        if cloud is not None:
            out["cloud_count"] = int(count[0])
            out["cloud"] = cloud[:min(int(count[0]), cloud.size)]
        return out

    def match_products(self, img_left, img_right, calib=None, provenance=False, confidence=False, depth=False, cloud=False, disp8=False,
                       disp16_scale=None, cloud_capacity=None):
        """Convenience: one synchronous Match, returns a dict of new arrays -- "disparity" and whatever was asked for: "provenance",
        "confidence", "depth" (needs calib), "cloud" (POINT_DTYPE, cut to the points written) with "cloud_count", "disp8", "disp16"
        (disp16_scale: the fixed-point scale, None = not requested).  Raises on failure."""
        d = np.empty((self.height, self.width), np.float32)
        req = self._product_arrays(calib, provenance, confidence, depth, cloud, disp8, disp16_scale, cloud_capacity)
        if not self.MatchProducts(img_left, img_right, d, req):
            raise RuntimeError("MatchProducts failed: " + last_error())
        return self._product_dict(d, req)

    def match_async_products(self, img_left, img_right, disp_left, products):
        """match_async plus the products of the request (HOST addresses; adc_match_async_products): only enqueues, wait() delivers the
        map and every product.  The images may be reused at once; disp_left and the request's arrays are kept alive until wait()."""
        l, r = _img(img_left), _img(img_right)
        assert products is None or products.sizes_ok(self.width * self.height)
        self._keep = (l, r, disp_left, products)
        return lib().adc_match_async_products(self._h, l.ctypes.data, r.ctypes.data, disp_left.ctypes.data,
                                              None if products is None else C.byref(products)) == 0

    def match_device_products(self, d_left, d_right, d_disp, products):
        """match_device plus the products of the request into the caller's DEVICE buffers (Products.from_addresses);
        asynchronous, call wait(), then cloud_count()."""
        return lib().adc_match_device_products(self._h, d_left, d_right, d_disp, None if products is None else C.byref(products)) == 0

    def disp16_device(self, d_disp, scale, d_disp16):
        """The 16-bit fixed-point kernel alone on any device-resident float32 [H][W] map of this geometry (adc_disp16_device);
        d_disp16: uint16 [H][W] device buffer; asynchronous, call wait()."""
        return lib().adc_disp16_device(self._h, d_disp, float(scale), d_disp16) == 0

    def cloud_count(self):
        n = C.c_uint64(0)
        if lib().adc_get_cloud_count(self._h, C.byref(n)) != 0:
            raise RuntimeError("adc_get_cloud_count failed")
        return int(n.value)

    def set_speckle_filter(self, max_size, max_diff):
        """Every later match of this object (all entry points) delivers its map with the 4-connected components (neighbours within
        max_diff) of at most max_size pixels set to +inf (adc_set_speckle_filter); max_size <= 0 switches the filter off.  Raises
        when refused (max_diff negative or not finite, a Match pending) or on a HIP failure."""
        if lib().adc_set_speckle_filter(self._h, int(max_size), float(max_diff)) != 0:
            raise RuntimeError("adc_set_speckle_filter failed: " + last_error())

    def filter_speckles_device(self, d_disp, max_size, max_diff, d_labels=None):
        """The filter's kernels on any device-resident float32 [H][W] map of this geometry, in place (adc_filter_speckles_device);
        d_labels: int32 [H][W] device buffer or None; asynchronous, call wait(), then speckle_stats()."""
        return lib().adc_filter_speckles_device(self._h, d_disp, int(max_size), float(max_diff), d_labels) == 0

    def filter_speckles(self, disp, max_size, max_diff, labels=False):
        """Host convenience: uploads a float32 [H][W] map, filters it on the device, downloads it.  Returns the filtered map, or
        (map, labels int32 [H][W]) with labels=True; speckle_stats() has the counts.  Raises on failure."""
        d = np.ascontiguousarray(disp, dtype=np.float32)
        assert d.shape == (self.height, self.width), (d.shape, (self.height, self.width))
        L = lib()
        pd = L.adc_device_malloc(d.nbytes)
        pl = L.adc_device_malloc(d.nbytes) if labels else None
        try:
            if not pd or (labels and not pl) or L.adc_memcpy_h2d(pd, d.ctypes.data, d.nbytes) != 0:
                raise RuntimeError("filter_speckles: device buffer")
            if not (self.filter_speckles_device(pd, max_size, max_diff, pl) and self.wait()):
                raise RuntimeError("adc_filter_speckles_device failed: " + last_error())
            out = np.empty_like(d)
            lab = np.empty(d.shape, np.int32) if labels else None
            if L.adc_memcpy_d2h(out.ctypes.data, pd, out.nbytes) != 0 or (labels and L.adc_memcpy_d2h(lab.ctypes.data, pl, lab.nbytes) != 0):
                raise RuntimeError("filter_speckles: download")
        finally:
            L.adc_device_free(pd)
            L.adc_device_free(pl)
        return (out, lab) if labels else out

    def speckle_stats(self):
        """(components, removed components, removed pixels) of the last filtered match / filter call that wait() has completed."""
        c, rc, rp = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        if lib().adc_get_speckle_stats(self._h, C.byref(c), C.byref(rc), C.byref(rp)) != 0:
            raise RuntimeError("adc_get_speckle_stats failed")
        return int(c.value), int(rc.value), int(rp.value)

    def set_cloud_voxel_grid(self, leaf, z_min=0.0, z_max=float("inf"), pose=None):
        """Every later cloud of this object (all entry points) holds one point per occupied voxel of edge `leaf` among the points with
        z_min <= Z <= z_max -- mean position and colour, pad = min(points, 255), in the order of the voxels' first pixels; the counts
        count voxels (adc_set_cloud_voxel_grid).  pose: None or (R, t), the camera-frame point's way into the frame of the grid.  A
        cloud then needs a calibration.  Raises when refused (a bad parameter, a Match pending) or on a HIP failure."""
        grid = VoxelGrid(leaf, z_min, z_max, pose)
        if lib().adc_set_cloud_voxel_grid(self._h, C.byref(grid)) != 0:
            raise RuntimeError("adc_set_cloud_voxel_grid failed: " + last_error())

    def clear_cloud_voxel_grid(self):
        """Every later cloud is the plain cloud again (adc_clear_cloud_voxel_grid)."""
        if lib().adc_clear_cloud_voxel_grid(self._h) != 0:
            raise RuntimeError("adc_clear_cloud_voxel_grid failed: " + last_error())

    def voxel_report(self):
        """{"points_valid", "points_kept", "voxels"} of the last voxel cloud that wait() or a synchronous call has completed."""
        rep = VoxelReport()
        if lib().adc_get_voxel_report(self._h, C.byref(rep)) != 0:
            raise RuntimeError("adc_get_voxel_report failed: " + last_error())
        return {"points_valid": int(rep.points_valid), "points_kept": int(rep.points_kept), "voxels": int(rep.voxels)}

    # -- rectification of raw images in front of the match (adc_set_rectify_*) -------------------
    def set_rectify_maps(self, side, raw, map_x, map_y):
        """Declares the raw images of one side (SIDE_LEFT / SIDE_RIGHT) as `raw` (a RawFormat) and their rectification as the float32
        [H][W] maps of source coordinates (as cv::initUndistortRectifyMap gives them).  Once both sides are set, EVERY match entry point
        of this object takes raw images (raw.nbytes bytes each) and matches their rectified versions.  Raises when refused or on a
        HIP failure."""
        mx, my = _maps(map_x, map_y, self.width, self.height)
        if lib().adc_set_rectify_maps(self._h, int(side), C.byref(raw), mx.ctypes.data, my.ctypes.data) != 0:
            raise RuntimeError("adc_set_rectify_maps failed: " + last_error())
        self._rect.set(side, raw)

    def set_rectify_model(self, side, raw, model):
        """The same with the maps computed on the device from a CameraModel (adc_set_rectify_model)."""
        if lib().adc_set_rectify_model(self._h, int(side), C.byref(raw), C.byref(model)) != 0:
            raise RuntimeError("adc_set_rectify_model failed: " + last_error())
        self._rect.set(side, raw)

    def set_input_format(self, side, raw):
        """Conversion only, for frames that are already rectified: declares the frames of one side as `raw` (a RawFormat of the object's
        width and height in any PIX_* layout -- Bayer, YUYV / UYVY, NV12, 16-bit, or one of the 8-bit ones) without maps
        (adc_set_input_format).  It sets the side like set_rectify_maps / set_rectify_model; any mix of the three works."""
        if lib().adc_set_input_format(self._h, int(side), C.byref(raw)) != 0:
            raise RuntimeError("adc_set_input_format failed: " + last_error())
        self._rect.set(side, raw)

    def clear_rectify(self):
        """Rectification off again: the entry points take rectified [H][W][3] BGR images (adc_clear_rectify)."""
        if lib().adc_clear_rectify(self._h) != 0:
            raise RuntimeError("adc_clear_rectify failed: " + last_error())
        self._rect.clear()

    def rectify_maps(self, side):
        """(map_x float32, map_y float32, valid uint8) [H][W] in use for a side (adc_get_rectify_maps); raises when the side is not set."""
        shp = (self.height, self.width)
        mx, my, v = np.empty(shp, np.float32), np.empty(shp, np.float32), np.empty(shp, np.uint8)
        if lib().adc_get_rectify_maps(self._h, int(side), mx.ctypes.data, my.ctypes.data, v.ctypes.data) != 0:
            raise RuntimeError("adc_get_rectify_maps failed: " + last_error())
        return mx, my, v

    def rectify_device(self, side, d_raw, d_bgr_out):
        """The remap alone on device buffers (ints): raw image of the side's geometry -> [H][W][3] BGR (adc_rectify_device);
        asynchronous, call wait()."""
        return lib().adc_rectify_device(self._h, int(side), d_raw, d_bgr_out) == 0

    def rectify(self, raw, side):
        """Host convenience: uploads one raw image of the side's geometry, remaps it on the device, returns uint8 [H][W][3] BGR."""
        a = _img(raw)
        fmt = self._rect.raw[int(side)]
        assert fmt is not None and a.size == fmt.nbytes, (None if fmt is None else fmt.nbytes, a.size)
        out = np.empty((self.height, self.width, 3), np.uint8)
        L = lib()
        pr, po = L.adc_device_malloc(a.nbytes), L.adc_device_malloc(out.nbytes)
        try:
            if not pr or not po or L.adc_memcpy_h2d(pr, a.ctypes.data, a.nbytes) != 0:
                raise RuntimeError("rectify: device buffer")
            if not (self.rectify_device(side, pr, po) and self.wait()):
                raise RuntimeError("adc_rectify_device failed: " + last_error())
            if L.adc_memcpy_d2h(out.ctypes.data, po, out.nbytes) != 0:
                raise RuntimeError("rectify: download")
        finally:
            L.adc_device_free(pr)
            L.adc_device_free(po)
        return out

    # -- evaluation against ground truth (adc_set_ground_truth / adc_evaluate*) ---------------------
    def set_ground_truth(self, left, right=None, nonocc=None, occ_thres=1.0, scale=1.0):
        """Sets the ground truth every later evaluate / evaluate_device of this object scores against.  left / right: a GroundTruth, or a
        2-D uint8 / uint16 / float32 array (then `scale` applies: disparity = value / scale, 0 = unknown in the integer formats);
        right may be None; nonocc: an optional uint8 [H][W] mask (nonzero = non-occluded) used when there is no right view.  Raises
        when refused or on a HIP failure."""
        gl = left if isinstance(left, GroundTruth) else GroundTruth(left, scale)
        gr = right if right is None or isinstance(right, GroundTruth) else GroundTruth(right, scale)
        m = None
        if nonocc is not None:
            m = np.ascontiguousarray(nonocc, dtype=np.uint8)
            assert m.shape == (self.height, self.width), (m.shape, (self.height, self.width))
        for g in (gl, gr):
            a = getattr(g, "_keep", None)
            assert g is None or a is None or a.shape == (self.height, self.width), (a.shape, (self.height, self.width))
        if lib().adc_set_ground_truth(self._h, C.byref(gl), None if gr is None else C.byref(gr), None if m is None else m.ctypes.data,
                                      float(occ_thres)) != 0:
            raise RuntimeError("adc_set_ground_truth failed: " + last_error())

    def clear_ground_truth(self):
        if lib().adc_clear_ground_truth(self._h) != 0:
            raise RuntimeError("adc_clear_ground_truth failed: " + last_error())

    def evaluate_device(self, d_disp, d_provenance=None, d_confidence=None, thresholds=(1.0,), d_err=None, d_class=None):
        """Scores a device-resident float32 [H][W] map (ints: device addresses; provenance uint8, confidence float32, err float32 and
        class uint8 [H][W] or None) against the ground truth set (adc_evaluate_device); asynchronous, call wait(), then eval_report().
        False when refused (no ground truth, a Match pending, bad thresholds, confidence without provenance) or on a HIP failure."""
        params = thresholds if isinstance(thresholds, EvalParams) else EvalParams(thresholds)
        return lib().adc_evaluate_device(self._h, d_disp, d_provenance, d_confidence, C.byref(params), d_err, d_class) == 0

    def evaluate(self, disp, provenance=None, confidence=None, thresholds=(1.0,), err=True, cls=True):
        """Host convenience (adc_evaluate): scores a float32 [H][W] numpy map; returns (EvalReport, err float32 [H][W] or None, class
        uint8 [H][W] or None).  Raises on failure."""
        shp = (self.height, self.width)
        d = np.ascontiguousarray(disp, dtype=np.float32)
        p = None if provenance is None else np.ascontiguousarray(provenance, dtype=np.uint8)
        c = None if confidence is None else np.ascontiguousarray(confidence, dtype=np.float32)
        for a in (d, p, c):
            assert a is None or a.shape == shp, (a.shape, shp)
        e = np.empty(shp, np.float32) if err else None
        k = np.empty(shp, np.uint8) if cls else None
        params = thresholds if isinstance(thresholds, EvalParams) else EvalParams(thresholds)
        rep = EvalReport()
        if lib().adc_evaluate(self._h, d.ctypes.data, None if p is None else p.ctypes.data, None if c is None else c.ctypes.data, C.byref(params),
                              None if e is None else e.ctypes.data, None if k is None else k.ctypes.data, C.byref(rep)) != 0:
            raise RuntimeError("adc_evaluate failed: " + last_error())
        return rep, e, k

    def eval_report(self):
        """The EvalReport of the last evaluation wait() has completed (adc_get_eval_report)."""
        rep = EvalReport()
        if lib().adc_get_eval_report(self._h, C.byref(rep)) != 0:
            raise RuntimeError("adc_get_eval_report failed: " + last_error())
        return rep

    # -- registration of depth into a second camera (adc_set_register_target / adc_register_depth* / adc_align_color*) ------------
    def set_register_target(self, target):
        """Sets the camera every later register_depth / align_color of this object projects into (a RegTarget); the first call
        allocates the z-buffer.  Raises when refused or on a HIP failure."""
        if lib().adc_set_register_target(self._h, None if target is None else C.byref(target)) != 0:
            raise RuntimeError("adc_set_register_target failed: " + last_error())
        self._reg_size = (int(target.height), int(target.width))

    def clear_register_target(self):
        if lib().adc_clear_register_target(self._h) != 0:
            raise RuntimeError("adc_clear_register_target failed: " + last_error())
        self._reg_size = None

    def register_depth_device(self, d_map, calib, kind=REG_FROM_DISPARITY, flags=0, d_depth=None, d_index=None):
        """Registers a device-resident float32 [H][W] disparity or depth map into the target camera (adc_register_depth_device; ints:
        device addresses, depth float32 / index int32 [Ht][Wt] or None); asynchronous, call wait(), then register_report().  False
        when refused (no target, a Match pending, a bad calibration, kind or flag, no output) or on a HIP failure."""
        c = _calib(calib)
        return lib().adc_register_depth_device(self._h, d_map, int(kind), None if c is None else C.byref(c), int(flags), d_depth, d_index) == 0

    def register_depth(self, map_, calib, kind=REG_FROM_DISPARITY, flags=0, depth=True, index=True):
        """Host convenience (adc_register_depth): returns (depth float32 [Ht][Wt] or None, index int32 [Ht][Wt] or None, RegReport).
        Raises on failure."""
        m = np.ascontiguousarray(map_, dtype=np.float32)
        assert m.shape == (self.height, self.width), (m.shape, (self.height, self.width))
        shp = getattr(self, "_reg_size", None) or (0, 0)
        d = np.empty(shp, np.float32) if depth else None
        i = np.empty(shp, np.int32) if index else None
        c = _calib(calib)
        rep = RegReport()
        if lib().adc_register_depth(self._h, m.ctypes.data, int(kind), None if c is None else C.byref(c), int(flags), None if d is None else d.ctypes.data,
                                    None if i is None else i.ctypes.data, C.byref(rep)) != 0:
            raise RuntimeError("adc_register_depth failed: " + last_error())
        return d, i, rep

    def align_color_device(self, d_map, calib, d_target_bgr, d_bgr_out, d_valid=None, kind=REG_FROM_DISPARITY):
        """Colour aligned to depth (adc_align_color_device): every source pixel takes the target image's colour at its projection;
        d_bgr_out uint8 [H][W][3] is what reproject_device takes as d_left.  Asynchronous, call wait().  False when refused or on a
        HIP failure."""
        c = _calib(calib)
        return lib().adc_align_color_device(self._h, d_map, int(kind), None if c is None else C.byref(c), d_target_bgr, d_bgr_out, d_valid) == 0

    def align_color(self, map_, calib, target_bgr, kind=REG_FROM_DISPARITY, valid=True):
        """Host convenience (adc_align_color): returns (bgr uint8 [H][W][3], valid uint8 [H][W] or None).  Raises on failure."""
        m = np.ascontiguousarray(map_, dtype=np.float32)
        t = np.ascontiguousarray(target_bgr, dtype=np.uint8)
        assert m.shape == (self.height, self.width), (m.shape, (self.height, self.width))
        shp = getattr(self, "_reg_size", None)
        assert shp is None or t.shape == shp + (3,), (t.shape, shp)
        out = np.empty((self.height, self.width, 3), np.uint8)
        v = np.empty((self.height, self.width), np.uint8) if valid else None
        c = _calib(calib)
        if lib().adc_align_color(self._h, m.ctypes.data, int(kind), None if c is None else C.byref(c), t.ctypes.data, out.ctypes.data,
                                 None if v is None else v.ctypes.data) != 0:
            raise RuntimeError("adc_align_color failed: " + last_error())
        return out, v

    def register_report(self):
        """The RegReport of the last registration wait() has completed (adc_get_register_report)."""
        rep = RegReport()
        if lib().adc_get_register_report(self._h, C.byref(rep)) != 0:
            raise RuntimeError("adc_get_register_report failed: " + last_error())
        return rep

    # -- surface normals from a disparity map (adc_normals_device / adc_normals / adc_get_normals_report) --------------------------
    def normals_device(self, d_disp, calib, params=None, d_normals=None, d_normals8=None):
        """Camera-facing surface normals of a device-resident float32 [H][W] disparity map (adc_normals_device; ints: device
        addresses, normals float32 [H][W][4] 16-byte aligned / normals8 uint8 [H][W][4] or None; params a NormalsParams or None for
        r = 2, max_diff = 1.0, min_points = 5); asynchronous, call wait(), then normals_report().  False when refused (a Match
        pending, a bad calibration or parameter, no output, a misaligned address) or on a HIP failure."""
        c = _calib(calib)
        return lib().adc_normals_device(self._h, d_disp, None if c is None else C.byref(c), None if params is None else C.byref(params), d_normals,
                                        d_normals8) == 0

    def normals(self, disp, calib, params=None, normals=True, normals8=True):
        """Host convenience (adc_normals): returns (normals float32 [H][W][4] or None, normals8 uint8 [H][W][4] or None,
        NormalsReport).  Raises on failure."""
        m = np.ascontiguousarray(disp, dtype=np.float32)
        assert m.shape == (self.height, self.width), (m.shape, (self.height, self.width))
        n = np.empty((self.height, self.width, 4), np.float32) if normals else None
        n8 = np.empty((self.height, self.width, 4), np.uint8) if normals8 else None
        c = _calib(calib)
        rep = NormalsReport()
        if lib().adc_normals(self._h, m.ctypes.data, None if c is None else C.byref(c), None if params is None else C.byref(params),
                             None if n is None else n.ctypes.data, None if n8 is None else n8.ctypes.data, C.byref(rep)) != 0:
            raise RuntimeError("adc_normals failed: " + last_error())
        return n, n8, rep

    def normals_report(self):
        """The NormalsReport of the last normals call wait() has completed (adc_get_normals_report)."""
        rep = NormalsReport()
        if lib().adc_get_normals_report(self._h, C.byref(rep)) != 0:
            raise RuntimeError("adc_get_normals_report failed: " + last_error())
        return rep

    # -- triangle mesh from a disparity map (adc_mesh_device / adc_mesh / adc_get_mesh_report) -------------------------------------
    def mesh_device(self, d_disp, calib=None, params=None, d_bgr_left=None, d_vertices=None, vertex_capacity=0, d_vertex_index=None, d_triangles=None,
                    triangle_capacity=0, d_counts=None):
        """Triangle mesh of a device-resident float32 [H][W] disparity map (adc_mesh_device; ints: device addresses or None; vertices
        adc_point records, 16-byte aligned; vertex_index int32; triangles uint32 x 3; counts uint32 [2] = vertices, triangles; params
        a MeshParams or None for max_diff = 1.0, step = 1; calib None for no calibration); asynchronous, call wait(), then
        mesh_report().  False when refused (a Match pending, a bad calibration or parameter, no output, a misaligned address) or on a
        HIP failure."""
        c = _calib(calib)
        return lib().adc_mesh_device(self._h, d_disp, d_bgr_left, None if c is None else C.byref(c), None if params is None else C.byref(params), d_vertices,
                                     int(vertex_capacity), d_vertex_index, d_triangles, int(triangle_capacity), d_counts) == 0

    def mesh(self, disp, calib=None, params=None, bgr_left=None):
        """Host convenience (adc_mesh): returns (vertices POINT_DTYPE [n], vertex_index int32 [n], triangles uint32 [m][3], MeshReport);
        sized at the worst case of the lattice and trimmed to the counts.  Raises on failure."""
        m = np.ascontiguousarray(disp, dtype=np.float32)
        assert m.shape == (self.height, self.width), (m.shape, (self.height, self.width))
        img = None
        if bgr_left is not None:
            img = np.ascontiguousarray(bgr_left, dtype=np.uint8)
            assert img.size == 3 * m.size, img.shape
        step = 1 if params is None else int(params.step)
        wl, hl = ((self.width - 1) // step + 1, (self.height - 1) // step + 1) if 1 <= step <= MESH_MAX_STEP else (1, 1)
        vcap, tcap = wl * hl, 2 * (wl - 1) * (hl - 1)
        v = np.zeros(vcap, POINT_DTYPE)
        vi = np.zeros(vcap, np.int32)
        t = np.zeros((max(tcap, 1), 3), np.uint32)
        c = _calib(calib)
        rep = MeshReport()
        if lib().adc_mesh(self._h, m.ctypes.data, None if img is None else img.ctypes.data, None if c is None else C.byref(c),
                          None if params is None else C.byref(params), v.ctypes.data, vcap, vi.ctypes.data, t.ctypes.data, tcap, C.byref(rep)) != 0:
            raise RuntimeError("adc_mesh failed: " + last_error())
        return v[:rep.vertices].copy(), vi[:rep.vertices].copy(), t[:rep.triangles].copy(), rep

    def mesh_report(self):
        """The MeshReport of the last mesh call wait() has completed (adc_get_mesh_report)."""
        rep = MeshReport()
        if lib().adc_get_mesh_report(self._h, C.byref(rep)) != 0:
            raise RuntimeError("adc_get_mesh_report failed: " + last_error())
        return rep

    # -- TSDF volume (adc_tsdf_*): frames fused into a volume on the device, and its surface points --------------------------------
    def tsdf_create(self, params):
        """Allocates and zeroes the volume of a TsdfParams (adc_tsdf_create); a second call replaces it.  False when refused or on a HIP failure."""
        return lib().adc_tsdf_create(self._h, C.byref(params)) == 0

    def tsdf_reset(self):
        return lib().adc_tsdf_reset(self._h) == 0

    def tsdf_destroy(self):
        return lib().adc_tsdf_destroy(self._h) == 0

    def tsdf_integrate_device(self, d_map, frame, d_bgr_left=None):
        """One frame into the volume (adc_tsdf_integrate_device; ints: device addresses; frame a TsdfFrame); asynchronous, call
        wait(), then tsdf_report().  False when refused (no volume, a Match pending, a bad frame, an image without a colour volume,
        a misaligned address) or on a HIP failure."""
        return lib().adc_tsdf_integrate_device(self._h, d_map, d_bgr_left, C.byref(frame)) == 0

    def tsdf_integrate(self, depth_map, frame, bgr_left=None):
        """Host convenience (adc_tsdf_integrate): returns the TsdfReport.  Raises on failure."""
        m = np.ascontiguousarray(depth_map, dtype=np.float32)
        assert m.shape == (self.height, self.width), (m.shape, (self.height, self.width))
        img = None
        if bgr_left is not None:
            img = np.ascontiguousarray(bgr_left, dtype=np.uint8)
            assert img.size == 3 * m.size, img.shape
        rep = TsdfReport()
        if lib().adc_tsdf_integrate(self._h, m.ctypes.data, None if img is None else img.ctypes.data, C.byref(frame), C.byref(rep)) != 0:
            raise RuntimeError("adc_tsdf_integrate failed: " + last_error())
        return rep

    def tsdf_extract_device(self, d_points, capacity, params=None, d_count=None):
        """The surface points of the volume (adc_tsdf_extract_device; d_points adc_point records, 16-byte aligned, or None with
        capacity 0 to count only; d_count one uint32 device word or None; params a TsdfExtractParams or None for min_weight = 1);
        asynchronous, call wait(), then tsdf_report()."""
        return lib().adc_tsdf_extract_device(self._h, None if params is None else C.byref(params), d_points, int(capacity), d_count) == 0

    def tsdf_extract(self, params=None, capacity=None):
        """Host convenience (adc_tsdf_extract): returns (points POINT_DTYPE [min(points, capacity)], TsdfExtractReport).  capacity
        None: a counting call first, then exactly as many records as there are.  Raises on failure."""
        rep = TsdfExtractReport()
        pp = None if params is None else C.byref(params)
        if capacity is None:
            if lib().adc_tsdf_extract(self._h, pp, None, 0, C.byref(rep)) != 0:
                raise RuntimeError("adc_tsdf_extract failed: " + last_error())
            capacity = rep.points
        pts = np.zeros(max(int(capacity), 1), POINT_DTYPE)
        if lib().adc_tsdf_extract(self._h, pp, pts.ctypes.data, int(capacity), C.byref(rep)) != 0:
            raise RuntimeError("adc_tsdf_extract failed: " + last_error())
        return pts[:min(rep.points, int(capacity))].copy(), rep

    def tsdf_report(self):
        """(TsdfReport or None, TsdfExtractReport or None) of the last integrate / extract call wait() has completed (adc_get_tsdf_report)."""
        out = []
        for cls, first in ((TsdfReport, True), (TsdfExtractReport, False)):
            rep = cls()
            rc = lib().adc_get_tsdf_report(self._h, C.byref(rep), None) if first else lib().adc_get_tsdf_report(self._h, None, C.byref(rep))
            out.append(rep if rc == 0 else None)
        return tuple(out)

    # -- stereo-aware fusion (adc_tsdf_weights*, adc_tsdf_fuse*): per-pixel observation weights, gated bilinear map sampling ------
    def tsdf_weights_device(self, d_map, frame, d_weight, params=None, d_provenance=None, d_confidence=None):
        """The observation weights of a map (adc_tsdf_weights_device; ints: device addresses; d_weight uint8 [H][W]; frame a
        TsdfFrame, of which kind and calib are read; params a TsdfWeightParams or None for the defaults); needs no volume;
        asynchronous, call wait(), then tsdf_fuse_report().  False when refused or on a HIP failure."""
        return lib().adc_tsdf_weights_device(self._h, d_map, d_provenance, d_confidence, C.byref(frame), None if params is None else C.byref(params), d_weight) == 0

    def tsdf_weights(self, depth_map, frame, params=None, provenance=None, confidence=None):
        """Host convenience (adc_tsdf_weights): returns (weight uint8 [H][W], TsdfWeightReport).  Raises on failure."""
        m = np.ascontiguousarray(depth_map, dtype=np.float32)
        assert m.shape == (self.height, self.width), (m.shape, (self.height, self.width))
        prov = None if provenance is None else np.ascontiguousarray(provenance, dtype=np.uint8)
        conf = None if confidence is None else np.ascontiguousarray(confidence, dtype=np.float32)
        assert prov is None or prov.shape == m.shape, prov.shape
        assert conf is None or conf.shape == m.shape, conf.shape
        w = np.zeros(m.shape, np.uint8)
        rep = TsdfWeightReport()
        if lib().adc_tsdf_weights(self._h, m.ctypes.data, None if prov is None else prov.ctypes.data, None if conf is None else conf.ctypes.data, C.byref(frame),
                                  None if params is None else C.byref(params), w.ctypes.data, C.byref(rep)) != 0:
            raise RuntimeError("adc_tsdf_weights failed: " + last_error())
        return w, rep

    def tsdf_fuse_device(self, d_map, frame, d_weight=None, params=None, d_bgr_left=None):
        """One weighted frame into the volume (adc_tsdf_fuse_device; ints: device addresses; d_weight uint8 [H][W] or None for 1
        everywhere; params a TsdfFuseParams or None); asynchronous, call wait(), then tsdf_fuse_report().  False when refused (as
        tsdf_integrate_device, or a bad params) or on a HIP failure."""
        return lib().adc_tsdf_fuse_device(self._h, d_map, d_bgr_left, d_weight, C.byref(frame), None if params is None else C.byref(params)) == 0

    def tsdf_fuse(self, depth_map, frame, weight=None, params=None, bgr_left=None):
        """Host convenience (adc_tsdf_fuse): returns the TsdfFuseReport.  Raises on failure."""
        m = np.ascontiguousarray(depth_map, dtype=np.float32)
        assert m.shape == (self.height, self.width), (m.shape, (self.height, self.width))
        img = None
        if bgr_left is not None:
            img = np.ascontiguousarray(bgr_left, dtype=np.uint8)
            assert img.size == 3 * m.size, img.shape
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.uint8)
        assert w is None or w.shape == m.shape, w.shape
        rep = TsdfFuseReport()
        if lib().adc_tsdf_fuse(self._h, m.ctypes.data, None if img is None else img.ctypes.data, None if w is None else w.ctypes.data, C.byref(frame),
                               None if params is None else C.byref(params), C.byref(rep)) != 0:
            raise RuntimeError("adc_tsdf_fuse failed: " + last_error())
        return rep

    def tsdf_fuse_report(self):
        """(TsdfFuseReport or None, TsdfWeightReport or None) of the last fuse / weights call wait() has completed (adc_get_tsdf_fuse_report)."""
        out = []
        for cls, first in ((TsdfFuseReport, True), (TsdfWeightReport, False)):
            rep = cls()
            rc = lib().adc_get_tsdf_fuse_report(self._h, C.byref(rep), None) if first else lib().adc_get_tsdf_fuse_report(self._h, None, C.byref(rep))
            out.append(rep if rc == 0 else None)
        return tuple(out)

    def tsdf_mesh_device(self, d_vertices, vertex_capacity, d_triangles, triangle_capacity, params=None, d_counts=None):
        """The triangle mesh of the volume (adc_tsdf_mesh_device; ints: device addresses; d_vertices adc_point records, 16-byte
        aligned, d_triangles three uint32 per record, either None when that list is not wanted, a capacity of 0 counts only; d_counts
        two uint32 device words or None; params a TsdfExtractParams or None for min_weight = 1); asynchronous, call wait(), then
        tsdf_mesh_report()."""
        return lib().adc_tsdf_mesh_device(self._h, None if params is None else C.byref(params), d_vertices, int(vertex_capacity), d_triangles,
                                          int(triangle_capacity), d_counts) == 0

    def tsdf_mesh(self, params=None, vertices=True, triangles=True):
        """Host convenience (adc_tsdf_mesh): a counting call, then exactly as many records as there are.  Returns (vertices POINT_DTYPE
        [.] or None, triangles uint32 [.][3] or None, TsdfMeshReport).  Raises on failure."""
        rep = TsdfMeshReport()
        pp = None if params is None else C.byref(params)
        if not (vertices or triangles):
            raise ValueError("tsdf_mesh: neither vertices nor triangles requested")
        token = np.zeros(1, POINT_DTYPE)  # (a non-NULL pointer with a capacity of 0 counts only)
        if lib().adc_tsdf_mesh(self._h, pp, token.ctypes.data if vertices else None, 0, token.ctypes.data if triangles else None, 0, C.byref(rep)) != 0:
            raise RuntimeError("adc_tsdf_mesh failed: " + last_error())
        nv, nt = rep.vertices, rep.triangles
        vtx = np.zeros(max(nv, 1), POINT_DTYPE)
        tri = np.zeros((max(nt, 1), 3), np.uint32)
        if lib().adc_tsdf_mesh(self._h, pp, vtx.ctypes.data if vertices else None, nv if vertices else 0, tri.ctypes.data if triangles else None,
                               nt if triangles else 0, C.byref(rep)) != 0:
            raise RuntimeError("adc_tsdf_mesh failed: " + last_error())
        return (vtx[:nv].copy() if vertices else None), (tri[:nt].copy() if triangles else None), rep

    def tsdf_mesh_report(self):
        """The TsdfMeshReport of the last mesh call wait() has completed (adc_get_tsdf_mesh_report), or None."""
        rep = TsdfMeshReport()
        return rep if lib().adc_get_tsdf_mesh_report(self._h, C.byref(rep)) == 0 else None

    def tsdf_raycast_device(self, params, d_depth=None, d_normals=None, d_bgr=None, d_status=None):
        """The volume seen from a camera pose (adc_tsdf_raycast_device; params a TsdfRaycastParams; ints: device addresses of float32
        [height][width], float32 [height][width][4] (16-byte aligned), uint8 [height][width][3] (needs a colour volume) and uint8
        [height][width], each None when not wanted, at least one); asynchronous, call wait(), then tsdf_raycast_report().  False when
        refused or on a HIP failure."""
        return lib().adc_tsdf_raycast_device(self._h, None if params is None else C.byref(params), d_depth, d_normals, d_bgr, d_status) == 0

    def tsdf_raycast(self, params, depth=True, normals=True, bgr=False, status=True):
        """Host convenience (adc_tsdf_raycast): returns (depth float32 [H][W], normals float32 [H][W][4], bgr uint8 [H][W][3], status
        uint8 [H][W], TsdfRaycastReport), None for an output that was not asked for.  Raises on failure."""
        if not (depth or normals or bgr or status):
            raise ValueError("tsdf_raycast: no output requested")
        h, w = max(int(params.height), 0), max(int(params.width), 0)
        d = np.zeros((h, w), np.float32) if depth else None
        n = np.zeros((h, w, 4), np.float32) if normals else None
        c = np.zeros((h, w, 3), np.uint8) if bgr else None
        s = np.zeros((h, w), np.uint8) if status else None
        rep = TsdfRaycastReport()
        if lib().adc_tsdf_raycast(self._h, C.byref(params), *[None if a is None else a.ctypes.data for a in (d, n, c, s)], C.byref(rep)) != 0:
            raise RuntimeError("adc_tsdf_raycast failed: " + last_error())
        return d, n, c, s, rep

    def tsdf_raycast_report(self):
        """The TsdfRaycastReport of the last ray cast wait() has completed (adc_get_tsdf_raycast_report), or None."""
        rep = TsdfRaycastReport()
        return rep if lib().adc_get_tsdf_raycast_report(self._h, C.byref(rep)) == 0 else None

    def track_device(self, d_map, frame, model_view, d_model_depth, d_model_normals, params=None, d_frame_normals=None, d_result=None):
        """The pose of the current frame against the model's predicted maps (adc_track_device; ints: device addresses of the frame's
        float32 [H][W] map, the model's float32 depth and [.][.][4] normals as tsdf_raycast_device wrote them for `model_view`, a
        TsdfRaycastParams; frame a TsdfFrame whose R, t are the initial guess; params a TrackParams or None for the defaults;
        d_frame_normals as normals_device writes them, or None; d_result an 8-byte aligned device address for the record, or None);
        asynchronous, call wait(), then track_result().  False when refused or on a HIP failure."""
        return lib().adc_track_device(self._h, d_map, d_frame_normals, None if frame is None else C.byref(frame), None if model_view is None else C.byref(model_view),
                                      d_model_depth, d_model_normals, None if params is None else C.byref(params), d_result) == 0

    def tsdf_track(self, depth_map, frame, params=None):
        """Host convenience (adc_tsdf_track): ray-casts the volume from the frame's guess and tracks the map against it; returns the
        TrackResult.  Raises on failure."""
        m = np.ascontiguousarray(depth_map, dtype=np.float32)
        assert m.shape == (self.height, self.width), (m.shape, (self.height, self.width))
        res = TrackResult()
        if lib().adc_tsdf_track(self._h, m.ctypes.data, C.byref(frame), None if params is None else C.byref(params), C.byref(res)) != 0:
            raise RuntimeError("adc_tsdf_track failed: " + last_error())
        return res

    def track_result(self):
        """The TrackResult of the last track wait() has completed (adc_get_track_result), or None."""
        res = TrackResult()
        return res if lib().adc_get_track_result(self._h, C.byref(res)) == 0 else None

    # -- moving volume (adc_tsdf_shift*): the window shifts by whole voxels, the surface that leaves is handed out once --------------
    def tsdf_shift_device(self, shift, d_points=None, capacity=0, min_weight=1, d_count=None):
        """Shifts the volume's window by `shift` = (sx, sy, sz) voxels (adc_tsdf_shift_device; a TsdfShiftParams is taken as it is)
        and writes the surface points whose voxels leave (d_points adc_point records, 16-byte aligned, or None with capacity 0;
        d_count one uint32 device word or None); asynchronous, call wait(), then tsdf_shift_report().  tsdf_volume_device() returns
        other addresses after every non-zero shift.  False when refused or on a HIP failure (the volume is then as it was)."""
        sp = shift if isinstance(shift, TsdfShiftParams) else TsdfShiftParams(shift, min_weight)
        return lib().adc_tsdf_shift_device(self._h, C.byref(sp), d_points, int(capacity), d_count) == 0

    def tsdf_shift(self, shift, min_weight=1, capacity=None):
        """Host convenience (adc_tsdf_shift): returns (leaving points POINT_DTYPE [min(points, capacity)], TsdfShiftReport); capacity
        None: all of them.  Raises on failure."""
        sp = shift if isinstance(shift, TsdfShiftParams) else TsdfShiftParams(shift, min_weight)
        rep = TsdfShiftReport()
        if capacity is None:  # (the leaving points are a sub-list of the whole volume's: its count bounds them)
            xrep = TsdfExtractReport()
            xp = TsdfExtractParams(sp.min_weight)
            if lib().adc_tsdf_extract(self._h, C.byref(xp), None, 0, C.byref(xrep)) != 0:
                raise RuntimeError("adc_tsdf_shift failed: " + last_error())
            capacity = xrep.points
        pts = np.zeros(max(int(capacity), 1), POINT_DTYPE)
        if lib().adc_tsdf_shift(self._h, C.byref(sp), pts.ctypes.data, int(capacity), C.byref(rep)) != 0:
            raise RuntimeError("adc_tsdf_shift failed: " + last_error())
        return pts[:min(rep.points, int(capacity))].copy(), rep

    def tsdf_shift_report(self):
        """The TsdfShiftReport of the last shift wait() has completed (adc_get_tsdf_shift_report), or None."""
        rep = TsdfShiftReport()
        return rep if lib().adc_get_tsdf_shift_report(self._h, C.byref(rep)) == 0 else None

    def tsdf_offset(self):
        """((ox, oy, oz) the sum of all shifts in voxels, (x, y, z) the origin given to tsdf_create) (adc_tsdf_get_offset)."""
        off, org = (C.c_int32 * 3)(), (C.c_float * 3)()
        if lib().adc_tsdf_get_offset(self._h, off, org) != 0:
            raise RuntimeError("adc_tsdf_get_offset failed: " + last_error())
        return tuple(off), tuple(org)

    def tsdf_follow_plan(self, R, t, follow=None):
        """tsdf_follow_plan for this handle's volume with its current origin: the shift to hand to tsdf_shift[_device]."""
        _, _, p = self.tsdf_volume_device()
        return tsdf_follow_plan(p, R, t, follow)

    def tsdf_volume_device(self):
        """(device address of the voxel words, of the colour words or None, TsdfParams) for a GPU consumer (adc_tsdf_get_volume_device)."""
        t, c, p = C.c_void_p(), C.c_void_p(), TsdfParams()
        if lib().adc_tsdf_get_volume_device(self._h, C.byref(t), C.byref(c), C.byref(p)) != 0:
            raise RuntimeError("adc_tsdf_get_volume_device failed: " + last_error())
        return t.value, c.value, p

    def tsdf_download(self):
        """Host copy of the whole volume (adc_tsdf_download): (tsdf uint32 [nz][ny][nx], color the same or None)."""
        _, c, p = self.tsdf_volume_device()
        shape = (p.nz, p.ny, p.nx)
        tsdf = np.zeros(shape, np.uint32)
        color = np.zeros(shape, np.uint32) if c else None
        if lib().adc_tsdf_download(self._h, tsdf.ctypes.data, None if color is None else color.ctypes.data) != 0:
            raise RuntimeError("adc_tsdf_download failed: " + last_error())
        return tsdf, color

    def tsdf_upload(self, tsdf, color=None):
        """Replaces the volume's words by host arrays of its shape (adc_tsdf_upload).  Raises on failure."""
        _, _, p = self.tsdf_volume_device()
        t = np.ascontiguousarray(tsdf, dtype=np.uint32)
        assert t.shape == (p.nz, p.ny, p.nx), (t.shape, (p.nz, p.ny, p.nx))
        c = None
        if color is not None:
            c = np.ascontiguousarray(color, dtype=np.uint32)
            assert c.shape == t.shape, c.shape
        if lib().adc_tsdf_upload(self._h, t.ctypes.data, None if c is None else c.ctypes.data) != 0:
            raise RuntimeError("adc_tsdf_upload failed: " + last_error())

    def match_device(self, d_left, d_right, d_disp):
        """Device pointers (ints); asynchronous; call wait().  The two image buffers are BORROWED until wait() returns: do
        not overwrite or free them before (the handle keeps no pointer to them afterwards)."""
        return lib().adc_match_device(self._h, d_left, d_right, d_disp) == 0

    def match_async(self, img_left, img_right, disp_left):
        l, r = _img(img_left), _img(img_right)
        self._keep = (l, r, disp_left)
        return lib().adc_match_async(self._h, l.ctypes.data, r.ctypes.data, disp_left.ctypes.data) == 0

    def wait(self):
        return lib().adc_wait(self._h) == 0

    def set_profiling(self, on=True):
        """False / 0: off; True / 1: stage timers + aggregation launch marks; 2: aggregation launch marks only (adcensus_c_api.h)"""
        lib().adc_set_profiling(self._h, int(on) if not isinstance(on, bool) else (1 if on else 0))

    def set_verbose(self, on=True):
        lib().adc_set_verbose(self._h, 1 if on else 0)

    def stage_ms(self):
        ms = (C.c_float * len(STAGES))()
        lib().adc_get_stage_ms(self._h, ms, len(STAGES))
        return {STAGES[i]: float(ms[i]) for i in range(len(STAGES))}

    def aggregate_pass_ms(self):
        ms, n = C.c_float(0), C.c_int(0)
        lib().adc_get_aggregate_pass_ms(self._h, C.byref(ms), C.byref(n))
        return float(ms.value), int(n.value)

    def aggregate_info(self):
        """(average ms of a regular aggregation launch, launches, algorithmic passes they covered, first pass fused?)"""
        ms, n, p, f = C.c_float(0), C.c_int(0), C.c_int(0), C.c_int(0)
        lib().adc_get_aggregate_info(self._h, C.byref(ms), C.byref(n), C.byref(p), C.byref(f))
        return float(ms.value), int(n.value), int(p.value), bool(f.value)

    def set_paper_modes(self, modes):
        """Opt-in paper features (PAPER_CENSUS5X5 | PAPER_SO_SUM | PAPER_RIGHT_ARMS); 0 = the reference's behaviour."""
        if lib().adc_set_paper_modes(self._h, int(modes)) != 0:
            raise RuntimeError("adc_set_paper_modes failed: " + last_error())

    def aggregate_kernel(self):
        return lib().adc_get_aggregate_kernel(self._h).decode()

    # -- test-only debug surface ---------------------------------------------------------------
    def _buf_spec(self, which):
        h, w, d = self.height, self.width, self.disp_range
        return {
            BUF_GRAY_LEFT: (np.uint8, (h, w)), BUF_GRAY_RIGHT: (np.uint8, (h, w)),
            BUF_CENSUS_LEFT: (np.uint64, (h, w)), BUF_CENSUS_RIGHT: (np.uint64, (h, w)),
            BUF_ARMS: (np.uint8, (h, w, 4)),
            BUF_SUPCOUNT_H: (np.uint16, (h, w)), BUF_SUPCOUNT_V: (np.uint16, (h, w)),
            BUF_VOLUME_A: (np.float32, (h, w, d)),
            BUF_DISP_LEFT: (np.float32, (h, w)), BUF_DISP_RIGHT: (np.float32, (h, w)),
            BUF_OUTLIER_LABEL: (np.uint8, (h, w)),
        }[which]

    def debug_read(self, which):
        dt, shp = self._buf_spec(which)
        out = np.empty(shp, dtype=dt)
        rc = lib().adc_debug_read(self._h, which, out.ctypes.data)
        if rc != 0:
            raise RuntimeError("adc_debug_read(%d) failed: %s" % (which, last_error()))
        return out

    def debug_write(self, which, arr):
        dt, shp = self._buf_spec(which)
        a = np.ascontiguousarray(arr, dtype=dt)
        assert a.shape == tuple(shp), (a.shape, shp)
        rc = lib().adc_debug_write(self._h, which, a.ctypes.data)
        if rc != 0:
            raise RuntimeError("adc_debug_write(%d) failed: %s" % (which, last_error()))

    def debug_read_itp_code(self, which_pass):
        """Test hook: (padded code map of interpolation pass 0 / 1 as u8 [rows][pitch], columns of padding on the left)."""
        pitch, rows, gx = C.c_int(0), C.c_int(0), C.c_int(0)
        if lib().adc_debug_itp_code_geometry(self._h, C.byref(pitch), C.byref(rows), C.byref(gx)) != 0:
            raise RuntimeError("adc_debug_itp_code_geometry failed: " + last_error())
        out = np.empty((rows.value, pitch.value), dtype=np.uint8)
        rc = lib().adc_debug_read_itp_code(self._h, int(which_pass), out.ctypes.data)
        if rc != 0:
            raise RuntimeError("adc_debug_read_itp_code(%d) failed: %s" % (which_pass, last_error()))
        return out, gx.value

    def debug_set_images(self, img_left, img_right):
        l, r = _img(img_left), _img(img_right)
        if lib().adc_debug_set_images(self._h, l.ctypes.data, r.ctypes.data) != 0:
            raise RuntimeError("adc_debug_set_images failed: " + last_error())

    def debug_run(self, stage, arg=0):
        rc = lib().adc_debug_run(self._h, stage, arg)
        if rc != 0:
            raise RuntimeError("adc_debug_run(%d) failed: %s" % (stage, last_error()))

    def debug_set_budget(self, kernels):
        """Test hook: the launch budget of the NEXT Match's voting chain (adc_debug_run ADC_RUN_REGION_VOTING with arg < 0)."""
        rc = lib().adc_debug_run(self._h, RUN_REGION_VOTING, -int(kernels))
        if rc != 0:
            raise RuntimeError("adc_debug_run failed: " + last_error())

    def debug_counter(self, which):
        return int(lib().adc_debug_counter(self._h, which))

    def voting_stats(self):
        r, e = C.c_int64(0), C.c_int64(0)
        lib().adc_debug_voting_stats(self._h, C.byref(r), C.byref(e))
        return int(r.value), int(e.value)
