"""Image pairs for the gather form of the sparse aggregation launches (tests/test_emul_gather.py, tests/test_gpu_gather_agg.py):
noise pairs with planted runs of equal pixels, so that the arms are as long as the runs and nothing else about the image changes."""
import numpy as np

from adcensus_amd import workloads


def run_pair(w, h, seed, horizontal=True, vertical=True, lengths=(6, 7, 8, 9), step=13):
    """Noise pair whose left image carries runs of `lengths` equal pixels: horizontal ones on every `step`-th row and vertical ones on
    every `step`-th column (offset, so that the two families cross only now and then), some of them starting in the first or ending
    in the last pixel of their line.  A run of n equal pixels gives its end pixels an arm of n - 1 and the pixels inside it both arms."""
    left, right = (a.copy() for a in workloads.noise_pair(w, h, seed=seed))
    k = 0
    if horizontal:
        for y in range(2, h, step):
            x = (y * 7) % 5
            while x + 2 * max(lengths) + 2 < w:  # (room for the run that ends with the row, and a pixel between the two)
                n = lengths[k % len(lengths)]
                k += 1
                left[y, x:x + n] = left[y, x]
                x += n + 9 + (k * 5) % 11
            left[y, w - lengths[k % len(lengths)]:w] = left[y, w - 1]  # ... and one that ends with the row
    if vertical:
        for x in range(6, w, step):
            y = (x * 3) % 4
            while y + 2 * max(lengths) + 2 < h:
                n = lengths[k % len(lengths)]
                k += 1
                left[y:y + n, x] = left[y, x]
                y += n + 8 + (k * 3) % 7
            left[h - lengths[k % len(lengths)]:h, x] = left[h - 1, x]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def arm_maxima(arms):
    """(longest horizontal, longest vertical) arm of an oracle `arms` dump [H][W][4] = left, right, up, down."""
    a = np.asarray(arms)
    return int(a[..., 0:2].max()), int(a[..., 2:4].max())
