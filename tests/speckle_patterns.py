"""Hand-built maps for the speckle filter's tests (tests/test_speckle_api.py at small sizes against a brute-force search,
tests/test_gpu_speckle.py against tests/speckle_ref.py up to 1920x1080): the shapes that break naive connected-component labelling.
patterns(w, h) -> {name: (map float32 [H][W], max_size, max_diff)}; every value is exactly representable."""
import numpy as np

F = np.float32
INF = F(np.inf)


def serpentine(w, h):
    """ONE component that visits every row: row y holds the value y, rows are a whole step apart, and one pixel at alternating
    ends (y + 0.5) joins its row to the next one -- the longest possible path.  max_diff 0.5."""
    d = np.repeat(np.arange(h, dtype=F)[:, None], w, 1)
    for y in range(h):
        d[y, w - 1 if y % 2 == 0 else 0] = F(y) + F(0.5)
    return d


def spiral(w, h):
    """A one-pixel path that winds inwards with one invalid pixel between its turns; the value grows by 0.25 per step, so the ends
    are far apart and every step is exactly max_diff = 0.25."""
    d = np.full((h, w), INF, F)
    on = np.zeros((h, w), bool)
    y = x = 0
    dy, dx = 0, 1
    v = F(0)
    d[0, 0], on[0, 0] = v, True
    while True:
        moved = False
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not on[ny, nx] and not (0 <= ay < h and 0 <= ax < w and on[ay, ax]):
                y, x = ny, nx
                v = v + F(0.25)
                d[y, x], on[y, x] = v, True
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return d


def comb(w, h):
    """Teeth (every other column) joined only along the LAST row: the merges arrive late."""
    d = np.full((h, w), INF, F)
    d[:, 0::2] = F(5)
    d[h - 1, :] = F(5)
    return d


def checker(w, h, a, b):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((yy + xx) % 2 == 0, F(a), F(b)).astype(F)


def ramp(w, h, per_row=0):
    """d[y][x] = (x + per_row * y) / 2: every horizontal step (and with per_row = 1 every vertical one) is exactly 0.5"""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx + per_row * yy).astype(F) * F(0.5)).astype(F)


def blocks(w, h):
    """Components of exactly 12 (removed at max_size 12) and 13 pixels (kept) on an invalid background, placed across the
    64-pixel pieces of a row and the 256- / 512-pixel stretches of the raster order, with negative values and one block per kind
    of invalid value next to it."""
    d = np.full((h, w), INF, F)
    k = 0
    for y0 in range(0, h - 4, 5):
        for x0 in list(range(61, w - 5, 64)) + [0, max(0, w - 5)]:
            if x0 + 5 > w or (d[y0:y0 + 4, max(0, x0 - 1):x0 + 6] != INF).any():
                continue
            v = F(-3.5) if k % 3 == 0 else F(k % 7)
            d[y0:y0 + 3, x0:x0 + 4] = v
            if k % 2:
                d[y0 + 3, x0 + (k % 4)] = v  # the thirteenth pixel
            if k % 5 == 0:
                d[y0 + 1, x0 + 4] = [np.nan, -np.inf][k % 2]  # touches the block, joins nothing
            k += 1
    return d


def patterns(w, h):
    rng = np.random.default_rng(w * 7919 + h)
    below = np.nextafter(F(0.5), F(0))
    out = {
        "constant": (np.full((h, w), -12.5, F), 100, 0.0),
        "all_invalid": (np.full((h, w), INF, F), 100, 1.0),
        "checker_valid_invalid": (checker(w, h, 3, np.inf), 1, 1.0),
        "checker_two_disparities": (checker(w, h, 10, 20), 1, 1.0),
        "comb": (comb(w, h), w * h - 1, 0.0),
        "ramp_le_edge": (ramp(w, h), w * h - 1, 0.5),             # one component: nothing removed
        "ramp_below_edge": (ramp(w, h), h, below),                # every column a component of h pixels: all removed
        "ramp_below_edge_kept": (ramp(w, h), h - 1, below),       # ... all kept
        "ramp_offset_rows": (ramp(w, h, 1), 1, below),            # W * H components
        "blocks": (blocks(w, h), 12, 0.0),
    }
    if w >= 2:
        out["serpentine"] = (serpentine(w, h), w * h - 1, 0.5)
        out["serpentine_removed"] = (serpentine(w, h), w * h, 0.5)
    out["spiral"] = (spiral(w, h), 50, 0.25)
    mix = (rng.integers(-8, 9, (h, w)).astype(F) * F(0.5)).astype(F)  # negative values, +-0, holes of every invalid kind
    mix[mix == 0] = np.where(rng.random(int((mix == 0).sum())) < 0.5, F(-0.0), F(0.0))
    r = rng.random((h, w))
    mix[r < 0.15] = INF
    mix[(r >= 0.15) & (r < 0.18)] = np.nan
    mix[(r >= 0.18) & (r < 0.21)] = -np.inf
    out["mixed_invalid_negative"] = (mix, 6, 0.5)
    return out
