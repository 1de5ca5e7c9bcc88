#!/usr/bin/env python3
"""Writes the ground-truth fixtures tests/golden/{cone,cloth3,wood2}_gt.npz from the Middlebury disparity images the reference ships
in its Data/ directory (next to the pairs tools/make_golden.py commits): the decoded uint8 arrays `left`, `right` (0 = unknown) and
the integer `scale` (disparity = value / scale).  Data only; PNG decode is lossless.

    python tools/make_gt_golden.py [DATA_DIR]        # default: the Data/ directory tools/make_golden.py reads
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF_DATA, ROOT  # noqa: E402

# name -> (left-view disparities, right-view disparities, scale)
SOURCES = {"cone": ("Cone/disp2.png", "Cone/disp6.png", 4), "cloth3": ("Cloth3/disp1.png", "Cloth3/disp5.png", 2),
           "wood2": ("Wood2/disp1.png", "Wood2/disp5.png", 2)}


def gray(path):
    from PIL import Image
    im = Image.open(path)
    assert im.mode == "L", (path, im.mode)  # 8-bit gray: the same lossless decode make_golden.py uses, without its colour conversion
    return np.ascontiguousarray(np.array(im))


def main(data):
    for name, (l, r, scale) in SOURCES.items():
        left, right = gray(os.path.join(data, l)), gray(os.path.join(data, r))
        assert left.shape == right.shape and left.dtype == np.uint8
        out = os.path.join(ROOT, "tests", "golden", name + "_gt.npz")
        np.savez_compressed(out, left=left, right=right, scale=np.int32(scale))
        print("%s: %dx%d, %d known left, %d bytes" % (out, left.shape[1], left.shape[0], int((left != 0).sum()), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else REF_DATA)
