"""An independent NumPy restatement of DESIGN.md 3.5.5 (disparitySGM's spec) for tests/test_sgm.py: written from
the text, not from include/vo_spec.h; vectorised over whole rows and the disparity axis, so nothing of the C
reference's per-pixel order survives in it.  Census words by shifted planes, the cost volume by one gather, each
path direction as a sweep over rows (or columns) whose step updates every pixel of the line and every disparity
at once, the selection by argmin / masked minima over the last axis."""
from __future__ import annotations

import numpy as np

ABSENT = 1 << 20          # a neighbour outside 0 .. D - 1: never the minimum


def census(img: np.ndarray) -> np.ndarray:
    """62-bit words: 7 x 9 window under replicate, raster order, centre left out, bit = neighbour < centre"""
    rows, cols = img.shape
    pad = np.pad(img, ((3, 3), (4, 4)), mode="edge")
    w = np.zeros((rows, cols), np.uint64)
    for dy in range(7):
        for dx in range(9):
            if dy == 3 and dx == 4:
                continue
            w = (w << np.uint64(1)) | (pad[dy:dy + rows, dx:dx + cols] < img).astype(np.uint64)
    return w


def popcount64(a: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,))
    return np.unpackbits(b, axis=-1).sum(axis=-1).astype(np.int32)


def cost_volume(left: np.ndarray, right: np.ndarray, dmin: int, D: int) -> np.ndarray:
    """C [rows, cols, D]"""
    cl, cr = census(left), census(right)
    cols = left.shape[1]
    xr = np.clip(np.arange(cols)[:, None] - (dmin + np.arange(D))[None, :], 0, cols - 1)      # [cols, D]
    return popcount64(cl[:, :, None] ^ cr[:, xr])


def _advance(prev: np.ndarray, c: np.ndarray, P1: int, P2: int) -> np.ndarray:
    """prev, c [n, D]: the previous pixels' L and this pixel's costs, for n independent paths"""
    m = prev.min(axis=1, keepdims=True)
    lower = np.concatenate([np.full_like(prev[:, :1], ABSENT), prev[:, :-1]], axis=1) + P1
    upper = np.concatenate([prev[:, 1:], np.full_like(prev[:, :1], ABSENT)], axis=1) + P1
    return c + np.minimum(np.minimum(prev, lower), np.minimum(upper, m + P2)) - m


def path_sum(Cv: np.ndarray, P1: int, P2: int) -> np.ndarray:
    """S [rows, cols, D] over the eight directions"""
    rows, cols, D = Cv.shape
    C = Cv.astype(np.int64)
    S = np.zeros_like(C)
    # along a row, both ways: a sweep over columns, all rows at once
    for order in (range(cols), range(cols - 1, -1, -1)):
        prev = None
        for x in order:
            prev = C[:, x] if prev is None else _advance(prev, C[:, x], P1, P2)
            S[:, x] += prev
    # the six directions that change the row: a sweep over rows, all columns at once; a pixel whose
    # predecessor's column falls outside the image starts a path
    for ys in (range(rows), range(rows - 1, -1, -1)):
        for shift in (0, 1, -1):              # the predecessor's column is x - shift
            prev = None
            for y in ys:
                if prev is None:
                    cur = C[y].copy()
                else:
                    cur = C[y].copy()
                    x = np.arange(cols)
                    inside = (x - shift >= 0) & (x - shift < cols)
                    cur[inside] = _advance(prev[x[inside] - shift], C[y][inside], P1, P2)
                S[y] += cur
                prev = cur
    return S


def select(S: np.ndarray, dmin: int, U: int) -> np.ndarray:
    """disp [rows, cols] float32"""
    rows, cols, D = S.shape
    S = S.astype(np.int64)
    ks = S.argmin(axis=2)                                                   # the first of equals
    V = np.take_along_axis(S, ks[:, :, None], 2)[:, :, 0]
    k = np.arange(D)[None, None, :]
    v = np.where(np.abs(k - ks[:, :, None]) > 1, S, 1 << 40).min(axis=2)
    unreliable = 100 * v < (100 + U) * V
    xr = np.arange(cols)[None, :] - (dmin + ks)
    invalid = (xr < 0) | (xr > cols - 1)
    a = np.take_along_axis(S, np.clip(ks - 1, 0, D - 1)[:, :, None], 2)[:, :, 0]
    b = np.take_along_axis(S, np.clip(ks + 1, 0, D - 1)[:, :, None], 2)[:, :, 0]
    den = 2 * (a - 2 * V + b)
    sub = (ks > 0) & (ks < D - 1) & (den > 0)
    base = (dmin + ks).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        off = (a - b).astype(np.float32) / den.astype(np.float32)
    out = np.where(sub, base + off, base).astype(np.float32)
    out[unreliable | invalid] = np.float32(np.nan)
    return out


def disparity(left, right, dmin: int, D: int, P1: int = 10, P2: int = 120, U: int = 15):
    S = path_sum(cost_volume(np.asarray(left), np.asarray(right), dmin, D), P1, P2)
    return S.astype(np.uint16), select(S, dmin, U)


def reconstruct(disp: np.ndarray, Q) -> np.ndarray:
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    rows, cols = disp.shape
    y, x = np.mgrid[1:rows + 1, 1:cols + 1].astype(np.float64)
    d = disp.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = [((Q[i, 0] * x + Q[i, 1] * y) + Q[i, 2] * d) + Q[i, 3] for i in range(4)]
        out = np.stack([(h[i] / h[3]).astype(np.float32) for i in range(3)], axis=-1)
    out[np.isnan(disp)] = np.float32(np.nan)
    return out
