"""An independent float64 restatement of the tracker's spec, written from its text with numpy:
float bilinear interpolation of the u8 levels, Scharr / 32 derivatives, no fixed point anywhere, and the
same control flow (levels, template tests, stops, skips).  The pyramid is the spec's integer one, evaluated
directly.  Used by tests/test_klt.py to bound what the fixed-point arithmetic costs."""
from __future__ import annotations

import numpy as np

OK, TEMPLATE_OUT, LOST, FLAT = 0, 1, 2, 3
STOP_NONE, STOP_EPS, STOP_OSC, STOP_MAXIT = 0, 1, 2, 3
PAD = 36                      # > 31 + 3: every admissible window, with its Scharr taps, lies inside the padded level
W5 = np.array([1, 4, 6, 4, 1], np.int64)


def pyramid(img: np.ndarray, levels: int) -> list:
    """u8 levels: (rows + 1) / 2 x (cols + 1) / 2, 5 x 5 binomial under reflect-101, (sum + 128) >> 8."""
    out = [np.asarray(img, np.uint8)]
    for _ in range(levels - 1):
        a = out[-1].astype(np.int64)
        rows, cols = a.shape
        p = _reflect_pad(a)
        r1, c1 = (rows + 1) // 2, (cols + 1) // 2
        h = sum(W5[j] * p[:, j:j + 2 * c1:2] for j in range(5))
        v = sum(W5[i] * h[i:i + 2 * r1:2, :] for i in range(5))
        out.append(((v + 128) >> 8).astype(np.uint8))
    return out


def _reflect_pad(a: np.ndarray) -> np.ndarray:
    def idx(n):
        out = []
        for p in range(-2, n + 2):
            while n > 1 and (p < 0 or p >= n):
                p = -p if p < 0 else 2 * n - 2 - p
            out.append(0 if n == 1 else p)
        return np.array(out)
    return a[np.ix_(idx(a.shape[0]), idx(a.shape[1]))]


class _Level:
    def __init__(self, lv: np.ndarray):
        self.rows, self.cols = lv.shape
        p = np.pad(lv.astype(np.float64), PAD + 1, mode="edge")      # replicate: a clamped read
        self.p = p[1:-1, 1:-1]
        self.gx = (3 * (p[:-2, 2:] - p[:-2, :-2]) + 10 * (p[1:-1, 2:] - p[1:-1, :-2]) + 3 * (p[2:, 2:] - p[2:, :-2])) / 32.0
        self.gy = (3 * (p[2:, :-2] - p[:-2, :-2]) + 10 * (p[2:, 1:-1] - p[:-2, 1:-1]) + 3 * (p[2:, 2:] - p[:-2, 2:])) / 32.0


def _out(q, bw, bh, lv):
    ix, iy = np.floor(q[0]), np.floor(q[1])
    return ix < -bw or ix >= lv.cols or iy < -bh or iy >= lv.rows


def _sample(f, q, bw, bh):
    ix, iy = int(np.floor(q[0])), int(np.floor(q[1]))
    a, b = q[0] - ix, q[1] - iy
    w = f[iy + PAD:iy + PAD + bh + 1, ix + PAD:ix + PAD + bw + 1]
    return (1 - a) * (1 - b) * w[:-1, :-1] + a * (1 - b) * w[:-1, 1:] + (1 - a) * b * w[1:, :-1] + a * b * w[1:, 1:]


def track(img0, img1, pts, guess=None, levels=3, block=(31, 31), max_it=30):
    """Forward pass only -> (pts1 [n, 2] float64, status [n], level_codes [n, 6] as tests/klt_ref.py's)."""
    bh, bw = block
    A = [_Level(l) for l in pyramid(img0, levels)]
    B = [_Level(l) for l in pyramid(img1, levels)]
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    h = np.array([(bw - 1) * 0.5, (bh - 1) * 0.5])
    fs = 2.0 ** -10          # the spec's 2^-20 applies to products of two values scaled by 32 each
    out = pts.copy()
    status = np.zeros(len(pts), np.int64)
    codes = np.full((len(pts), 6), 255, np.uint8)
    for i, pt in enumerate(pts):
        pt0 = pt - 1.0
        nxt = None
        st = OK
        for l in range(levels - 1, -1, -1):
            prev = pt0 * 2.0 ** -l
            nxt = ((np.asarray(guess[i], np.float64) - 1.0) if guess is not None else pt0) * 2.0 ** -l if l == levels - 1 else 2.0 * nxt
            a, b = A[l], B[l]
            why, stop = OK, STOP_NONE
            p = prev - h
            if _out(p, bw, bh, a):
                why = TEMPLATE_OUT
            else:
                I, Ix, Iy = _sample(a.p, p, bw, bh), _sample(a.gx, p, bw, bh), _sample(a.gy, p, bw, bh)
                A11, A12, A22 = (Ix * Ix).sum() * fs, (Ix * Iy).sum() * fs, (Iy * Iy).sum() * fs
                D = A11 * A22 - A12 * A12
                min_eig = (A22 + A11 - np.sqrt((A11 - A22) ** 2 + 4 * A12 * A12)) / (2 * bw * bh)
                if min_eig < 1e-4 or D < 1.19209290e-07:
                    why = FLAT
            if why == OK:
                q = nxt - h
                cur = nxt
                pd = None
                for j in range(max_it):
                    if _out(q, bw, bh, b):
                        why = LOST
                        break
                    diff = _sample(b.p, q, bw, bh) - I
                    b1, b2 = (diff * Ix).sum() * fs, (diff * Iy).sum() * fs
                    d = np.array([(A12 * b2 - A22 * b1) / D, (A12 * b1 - A11 * b2) / D])
                    q = q + d
                    cur = q + h
                    if d @ d <= 1e-4:
                        stop = STOP_EPS
                        break
                    if j > 0 and abs(d[0] + pd[0]) < 0.01 and abs(d[1] + pd[1]) < 0.01:
                        cur = cur - 0.5 * d
                        stop = STOP_OSC
                        break
                    pd = d
                if why == OK:
                    if stop == STOP_NONE:
                        stop = STOP_MAXIT
                    nxt = cur
            codes[i, l] = stop if why == OK else 16 + why
            if why != OK and l == 0:
                st = why
        if st == OK and not (0 <= nxt[0] <= img0.shape[1] - 1 and 0 <= nxt[1] <= img0.shape[0] - 1):
            st = LOST
        status[i] = st
        if st == OK:
            out[i] = nxt + 1.0
    return out, status, codes
