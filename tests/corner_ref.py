"""ctypes driver of the CPU reference of vo_detect_corners (tests/corner_ref/corner_ref.c: include/vo_spec.h's
vo_corner_* functions, the ones the kernels call, around the normative loops).  Test infrastructure, built on
demand like tests/klt_ref.py.

`detect(img, ...)` -> record as Context.detect_corners gives it plus the metric plane; `image(key)` generates
the fixtures in numpy (rotated bright squares, a blurred checkerboard, blobs, noise and the small engineered
images of the census); `table()` is the list of rows the CPU and GPU suites share, `results()` their reference
outputs, computed once."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "corner_ref"
LIB = HERE / "build" / "libcorner_ref.so"
MAIN = HERE / "build" / "corner_ref_main"

MINEIG, HARRIS = 0, 1
OK, ERR_CAPACITY = 0, -5
SIZES = {"a": (40, 56), "b": (37, 53), "c": (64, 64)}
MAX_KEYPOINTS = 512                       # of the suites' contexts: the device list holds 4 x as many
DEFAULTS = dict(method=MINEIG, f=5, min_quality=0.01, strongest=0, roi=None, max_keypoints=MAX_KEYPOINTS)
WEIGHTS = {
    3: [1123, 1850, 1123],
    5: [547, 939, 1124, 939, 547],
    7: [352, 558, 735, 806, 735, 558, 352],
    9: [258, 381, 502, 593, 628, 593, 502, 381, 258],
    11: [203, 283, 368, 443, 495, 512, 495, 443, 368, 283, 203],
    13: [167, 223, 284, 342, 391, 423, 436, 423, 391, 342, 284, 223, 167],
    15: [141, 183, 229, 274, 315, 348, 369, 378, 369, 348, 315, 274, 229, 183, 141],
}

_lib = None


def build(target: str = "all") -> None:
    subprocess.run(["make", "-s", "-C", str(HERE), target], check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(str(LIB))
        P = C.POINTER
        L.corner_ref_weights.argtypes = [C.c_int, P(C.c_int)]
        L.corner_ref_weights.restype = None
        L.corner_ref_offset.argtypes = [C.c_float, C.c_float, C.c_float]
        L.corner_ref_offset.restype = C.c_float
        L.corner_ref_metric.argtypes = [P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_float)]
        L.corner_ref_detect.argtypes = [P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, P(C.c_int), C.c_int,
                                        P(C.c_float), P(C.c_float), P(C.c_float), C.c_int, P(C.c_int)]
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def weights(f: int) -> list:
    q = (C.c_int * 15)()
    lib().corner_ref_weights(f, q)
    return list(q[:f])


def offset(l: float, z: float, g: float) -> float:
    """vo_corner_offset on three f32 metrics."""
    return float(lib().corner_ref_offset(l, z, g))


def detect(img, method=MINEIG, f=5, min_quality=0.01, strongest=0, roi=None, max_keypoints=MAX_KEYPOINTS, capacity=None) -> dict:
    """-> dict(status OK | ERR_CAPACITY, count (the true count on overflow), loc [n, 2] f32, metric [n] f32, plane
    [rows, cols] f32)."""
    img = np.ascontiguousarray(img, np.uint8)
    rows, cols = img.shape
    cap = 4 * max_keypoints if capacity is None else capacity
    loc = np.zeros((max(cap, 1), 2), np.float32)
    met = np.zeros(max(cap, 1), np.float32)
    plane = np.zeros((rows, cols), np.float32)
    n = C.c_int(0)
    r = (C.c_int * 4)(*roi) if roi is not None else None
    rc = lib().corner_ref_detect(_p(img, C.c_uint8), rows, cols, int(method), int(f), float(min_quality), int(strongest), r,
                                 4 * max_keypoints, _p(plane, C.c_float), _p(loc, C.c_float), _p(met, C.c_float), cap, C.byref(n))
    assert rc in (0, 1), rc
    k = n.value if rc == 0 else 0
    return dict(status=OK if rc == 0 else ERR_CAPACITY, count=n.value, loc=loc[:k].copy(), metric=met[:k].copy(), plane=plane)


def write_problem(path, img, method=MINEIG, f=5, min_quality=0.01, strongest=0, roi=None, max_keypoints=MAX_KEYPOINTS) -> None:
    """The file tests/corner_ref/corner_ref_main.c reads."""
    rows, cols = img.shape
    with open(path, "wb") as fh:
        fh.write(np.array([rows, cols, method, f, strongest, 4 * max_keypoints, 4 * max_keypoints, roi is not None] +
                          list(roi if roi is not None else (0, 0, 0, 0)), np.int32).tobytes())
        fh.write(np.array([min_quality], np.float32).tobytes())
        fh.write(np.ascontiguousarray(img, np.uint8).tobytes())


def main_lines(rec: dict) -> list:
    """A detect() record as corner_ref_main prints it."""
    out = ["%d %d" % (0 if rec["status"] == OK else 1, rec["count"])]
    for xy, m in zip(rec["loc"].view(np.uint32), rec["metric"].view(np.uint32)):
        out.append("%08x %08x %08x" % (xy[0], xy[1], m))
    return out


# --------------------------------------------------------------------------- generated images
def _blur(a: np.ndarray, sigma: float) -> np.ndarray:
    """Periodic Gaussian blur of a float64 image by its transfer function."""
    fy, fx = np.fft.fftfreq(a.shape[0])[:, None], np.fft.fftfreq(a.shape[1])[None, :]
    return np.fft.ifft2(np.fft.fft2(a) * np.exp(-2.0 * (np.pi * sigma) ** 2 * (fx * fx + fy * fy))).real


def _u8(a: np.ndarray) -> np.ndarray:
    out = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def render_squares(rows: int, cols: int, squares, ss: int = 8, lo: float = 40.0, hi: float = 200.0) -> np.ndarray:
    """Bright squares (centre x, y in 0-based pixel coordinates, half side, angle in radians) on a dark ground, by
    ss x ss supersampling: float64 grey levels.  The four corners of square k are corners_of(squares[k])."""
    y, x = (np.arange(rows * ss) + 0.5) / ss - 0.5, (np.arange(cols * ss) + 0.5) / ss - 0.5
    X, Y = np.meshgrid(x, y)
    cover = np.zeros_like(X)
    for cx, cy, half, ang in squares:
        u = (X - cx) * np.cos(ang) + (Y - cy) * np.sin(ang)
        v = -(X - cx) * np.sin(ang) + (Y - cy) * np.cos(ang)
        cover = np.maximum(cover, ((np.abs(u) <= half) & (np.abs(v) <= half)).astype(np.float64))
    return lo + (hi - lo) * cover.reshape(rows, ss, cols, ss).mean((1, 3))


def corners_of(square) -> np.ndarray:
    """The L-corners of a rendered square, [4, 2] (x, y), 1-based as Location is."""
    cx, cy, half, ang = square
    out = []
    for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        out.append((cx + half * (su * np.cos(ang) - sv * np.sin(ang)) + 1.0, cy + half * (su * np.sin(ang) + sv * np.cos(ang)) + 1.0))
    return np.array(out)


SQUARES = {
    "a": [(14.3, 12.6, 6.0, 0.3), (38.7, 24.2, 7.5, 1.0), (15.5, 30.0, 4.0, 0.0)],
    "b": [(13.2, 11.4, 5.5, 0.7), (36.1, 22.8, 7.0, 0.2)],
    "c": [(16.4, 15.7, 7.0, 0.5), (45.2, 18.3, 6.0, 1.2), (20.6, 45.1, 8.0, 0.15), (46.0, 46.0, 5.0, 0.0)],
}
CHECKER_PERIOD, CHECKER_ORIGIN = 9.0, (4.3, 5.6)


def checker_float(rows: int, cols: int) -> np.ndarray:
    """A checkerboard of period 9 px whose X-corners lie at CHECKER_ORIGIN + 9 (i, j) (0-based x, y), supersampled
    and blurred by sigma 1: float64 grey levels."""
    ss = 8
    y, x = (np.arange(rows * ss) + 0.5) / ss - 0.5, (np.arange(cols * ss) + 0.5) / ss - 0.5
    X, Y = np.meshgrid(x, y)
    board = (np.floor((X - CHECKER_ORIGIN[0]) / CHECKER_PERIOD) + np.floor((Y - CHECKER_ORIGIN[1]) / CHECKER_PERIOD)) % 2
    return _blur(50.0 + 150.0 * board.reshape(rows, ss, cols, ss).mean((1, 3)), 1.0)


def x_corners(rows: int, cols: int, margin: float = 6.0) -> np.ndarray:
    """The checkerboard's X-corners at least `margin` from the border, [n, 2] (x, y), 1-based."""
    out = []
    for j in range(-1, rows):
        for i in range(-1, cols):
            x, y = CHECKER_ORIGIN[0] + CHECKER_PERIOD * i, CHECKER_ORIGIN[1] + CHECKER_PERIOD * j
            if margin <= x <= cols - 1 - margin and margin <= y <= rows - 1 - margin:
                out.append((x + 1.0, y + 1.0))
    return np.array(out)


def _dots(rows: int, cols: int, pixels, ground: int = 30, value: int = 220) -> np.ndarray:
    a = np.full((rows, cols), ground, np.float64)
    for r, c in pixels:
        a[r, c] = value
    return a


@functools.lru_cache(maxsize=None)
def image(key: str) -> np.ndarray:
    """Fixture images by key "<size>:<kind>", uint8, read-only."""
    size, kind = key.split(":")
    rows, cols = SIZES[size]
    rng = np.random.default_rng(sum(map(ord, key)))
    if kind == "squares":
        return _u8(_blur(render_squares(rows, cols, SQUARES[size]), 0.7))
    if kind == "checker":
        return _u8(checker_float(rows, cols))
    if kind == "blobs":
        a = np.full((rows, cols), 60.0)
        yy, xx = np.mgrid[:rows, :cols]
        for _ in range(12):
            cy, cx, s, amp = rng.uniform(4, rows - 5), rng.uniform(4, cols - 5), rng.uniform(1.2, 2.5), rng.uniform(60, 180)
            a += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        return _u8(a)
    if kind == "noise":
        return _u8(128.0 + 40.0 * _blur(rng.standard_normal((rows, cols)), 1.5) / 0.19)
    if kind == "white":                   # many corners: the list overflow
        return _u8(rng.integers(0, 256, (rows, cols)).astype(np.float64))
    if kind == "flat":
        return _u8(np.full((rows, cols), 77.0))
    if kind == "edge":                    # a straight vertical edge: one eigenvalue is 0 everywhere
        a = np.full((rows, cols), 40.0)
        a[:, cols // 2:] = 200.0
        return _u8(a)
    if kind == "pairs":
        # mirror-symmetric dots: a 2-wide x 3-tall block (equal pair in a row), 3 x 2 (in a column), two pixels on
        # an anti-diagonal (equal diagonal pair), a 2 x 2 block (a 2 x 2 plateau)
        px = [(8 + i, 10 + j) for i in range(3) for j in range(2)] + [(8 + i, 30 + j) for i in range(2) for j in range(3)]
        px += [(26, 12), (25, 13)] + [(26 + i, 32 + j) for i in range(2) for j in range(2)]
        return _u8(_dots(rows, cols, px))
    if kind == "border":
        # single bright pixels on each side and in each corner of the image
        px = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (0, cols // 2), (rows - 1, cols // 2), (rows // 2, 0),
              (rows // 2, cols - 1), (rows // 2, cols // 2)]
        return _u8(_dots(rows, cols, px))
    if kind == "quad":
        # an axis-aligned square, mirror-symmetric in both axes about pixel centres: its four corners have one metric
        a = np.full((rows, cols), 40.0)
        a[12:rows - 12, 14:cols - 14] = 210.0
        a[rows // 2 - 2:rows // 2 + 3, cols // 2 - 2:cols // 2 + 3] = 90.0    # and a weaker square inside
        return _u8(a)
    raise KeyError(key)


def lattice(rows: int, cols: int, tile_w: int = 64, tile_h: int = 16) -> np.ndarray:
    """Single bright pixels of varying grey, every 5 rows and every 7 columns with the columns shifted from row to
    row, so that over an image of a few tiles they fall on every residue of the kernel's tile width and height
    (the test that uses it asserts that for the detected corners)."""
    a = np.full((rows, cols), 25.0)
    k = 0
    for r in range(1, rows - 1, 5):
        for c in range(1 + (3 * k) % 7, cols - 1, 7):
            a[r, c] = 120.0 + (37 * (r + c)) % 120
        k += 1
    return _u8(a)


# --------------------------------------------------------------------------- the table
def _row(name, key, **kw):
    return dict(name=name, image=key, params=dict(DEFAULTS, **kw))


@functools.lru_cache(maxsize=None)
def table() -> list:
    t = []
    for size in SIZES:
        for kind in ("squares", "checker", "blobs", "noise"):
            t.append(_row(f"{kind}_{size}", f"{size}:{kind}"))
    t += [
        _row("squares_a_harris", "a:squares", method=HARRIS),
        _row("checker_b_harris_f3", "b:checker", method=HARRIS, f=3),
        _row("noise_c_f3", "c:noise", f=3),
        _row("noise_c_f15", "c:noise", f=15),
        _row("noise_b_harris_f15", "b:noise", method=HARRIS, f=15),
        _row("blobs_a_f9", "a:blobs", f=9),
        _row("checker_c_f9", "c:checker", f=9),
        _row("squares_c_f15", "c:squares", f=15),
        _row("noise_a_f15", "a:noise", f=15),
        _row("noise_b_f9", "b:noise", f=9),
        _row("blobs_c_harris_f15", "c:blobs", method=HARRIS, f=15),
        _row("pairs_a", "a:pairs"),
        _row("pairs_a_harris", "a:pairs", method=HARRIS),
        _row("pairs_b_f3", "b:pairs", f=3),
        _row("border_a", "a:border"),
        _row("border_b_f3", "b:border", f=3),
        _row("border_c_harris_f15", "c:border", method=HARRIS, f=15),
        _row("flat_a", "a:flat"),
        _row("flat_b_harris", "b:flat", method=HARRIS),
        _row("edge_a_harris", "a:edge", method=HARRIS),
        _row("edge_a_mineig", "a:edge"),
        _row("noise_a_q0", "a:noise", min_quality=0.0),
        _row("noise_a_q1", "a:noise", min_quality=1.0),
        _row("noise_b_q50", "b:noise", min_quality=0.5),
        _row("noise_a_roi_1x1", "a:noise", roi="peak1x1"),
        _row("noise_a_roi_boundary", "a:noise", roi="peak_on_boundary"),
        _row("noise_a_roi_excl", "a:noise", roi="excludes_peak", min_quality=0.3),
        _row("squares_c_roi_harris", "c:squares", method=HARRIS, roi=(9, 5, 40, 33)),
        _row("quad_a_strongest_tie", "a:quad", strongest=2),
        _row("quad_a_strongest_3", "a:quad", strongest=3),
        _row("quad_a_strongest_all", "a:quad", strongest=500),
        _row("noise_c_strongest_10", "c:noise", strongest=10, f=3, min_quality=0.0),
        _row("white_c_overflow", "c:white", f=3, min_quality=0.0, max_keypoints=16),
        _row("white_c_overflow_strongest", "c:white", f=3, min_quality=0.0, max_keypoints=16, strongest=5),
        _row("noise_a_k16_overflow_by_one", "a:noise", max_keypoints=16, min_quality=0.2),
        _row("noise_a_k16", "a:noise", max_keypoints=16, min_quality=0.5),
    ]
    for r in t:
        r["params"]["roi"] = _named_roi(r["image"], r["params"])
    return t


def _named_roi(key: str, p: dict):
    """ROIs named after the metric plane's global maximum (x y w h, 1-based)."""
    roi = p["roi"]
    if not isinstance(roi, str):
        return roi
    plane = detect(image(key), p["method"], p["f"])["plane"]
    rows, cols = plane.shape
    pr, pc = np.unravel_index(np.argmax(plane), plane.shape)
    if roi == "peak1x1":
        return (int(pc) + 1, int(pr) + 1, 1, 1)
    if roi == "peak_on_boundary":         # the maximum on the ROI's first column and last row
        return (int(pc) + 1, max(int(pr) - 9, 0) + 1, min(12, cols - int(pc)), int(pr) - max(int(pr) - 9, 0) + 1)
    if roi == "excludes_peak":            # the half of the image that does not hold the maximum
        return (1, 1, cols // 2, rows) if pc >= cols // 2 else (cols // 2 + 1, 1, cols - cols // 2, rows)
    raise KeyError(roi)


@functools.lru_cache(maxsize=None)
def results() -> list:
    return [detect(image(r["image"]), **r["params"]) for r in table()]
