"""An independent float64 restatement of DESIGN.md 3.5.4 in numpy, for test_corner.py: the image in [0, 1], central
differences under replicate, the three products smoothed by the true separable Gaussian (sigma = f / 3, weights
normalised in float64, products replicated past the border), the response, the same threshold and local-maximum
rules with a relative margin, and the parabolic sub-pixel offset in float64.  Nothing here is shared with
include/vo_spec.h or tests/corner_ref."""
from __future__ import annotations

import numpy as np

MINEIG, HARRIS = 0, 1


def metric_plane(img: np.ndarray, method: int = MINEIG, f: int = 5) -> np.ndarray:
    p = np.pad(np.asarray(img, np.float64) / 255.0, 1, mode="edge")
    ix = p[1:-1, 2:] - p[1:-1, :-2]
    iy = p[2:, 1:-1] - p[:-2, 1:-1]
    R = (f - 1) // 2
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-k * k / (2.0 * (f / 3.0) ** 2))
    w /= w.sum()

    def smooth(a):
        a = np.pad(a, R, mode="edge")
        a = sum(w[j] * a[:, j:a.shape[1] - 2 * R + j] for j in range(f))
        return sum(w[i] * a[i:a.shape[0] - 2 * R + i, :] for i in range(f))

    a, b, c = smooth(ix * ix), smooth(iy * iy), smooth(ix * iy)
    if method == HARRIS:
        return a * b - c * c - 0.04 * (a + b) ** 2
    return 0.5 * ((a + b) - np.sqrt((a - b) ** 2 + 4.0 * c * c))


def _neighbours(m: np.ndarray):
    """(plane of neighbour values padded with -inf, precedes) for the 8 neighbours."""
    rows, cols = m.shape
    p = np.pad(m, 1, mode="constant", constant_values=-np.inf)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr or dc:
                yield p[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols], (dr < 0 or (dr == 0 and dc < 0))


def corner_mask(m: np.ndarray, min_quality: float, roi=None, margin: float = 0.0) -> np.ndarray:
    """Pixels that are corners by the rules of 3.5.4 with every comparison tightened (margin > 0: clears the
    threshold and beats each neighbour by the relative margin) or loosened (margin < 0) by |margin| of the
    corner's metric."""
    rows, cols = m.shape
    x0, y0, w, h = (0, 0, cols, rows) if roi is None else (roi[0] - 1, roi[1] - 1, roi[2], roi[3])
    inside = np.zeros(m.shape, bool)
    inside[y0:y0 + h, x0:x0 + w] = True
    mmax = m[inside].max()
    if not mmax > 0:
        return np.zeros(m.shape, bool)
    slack = margin * np.abs(m)
    ok = inside & (m - slack > min_quality * mmax)
    for n, before in _neighbours(m):
        ok &= (m - slack > n) if (before or margin != 0.0) else (m >= n)
    return ok


def locations(m: np.ndarray, mask: np.ndarray) -> dict:
    """(r, c) -> (x, y), 1-based, with the float64 parabolic offset (0 beside the border)."""
    rows, cols = m.shape
    out = {}
    for r, c in zip(*np.nonzero(mask)):
        d = [0.0, 0.0]
        for axis, (lo, hi, n) in enumerate((((r, c - 1), (r, c + 1), cols), ((r - 1, c), (r + 1, c), rows))):
            i = (c, r)[axis]
            if 0 < i < n - 1:
                l, z, g = m[lo], m[r, c], m[hi]
                den = (l - z) + (g - z)
                d[axis] = min(max(0.5 * (l - g) / den, -0.5), 0.5) if den < 0 else 0.0
        out[(int(r), int(c))] = (c + 1 + d[0], r + 1 + d[1])
    return out
