"""ctypes driver of the CPU reference of vo_track_points (tests/klt_ref/klt_ref.c: include/vo_spec.h's
vo_klt_* functions, the ones the kernels call, around the normative loops).  Test infrastructure, built
on demand like tests/fund_ref.py.

`pyramid(img, levels)` -> the list of u8 levels; `track(img0, img1, pts, ...)` -> record as
Context.track_points plus the forward pass' per-level codes.  `texture` / `shifted` generate the
images (band-limited noise, a copy shifted by Fourier phase with added noise), `table()` the rows the
CPU and GPU suites share, `results()` their reference outputs, computed once."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "klt_ref"
LIB = HERE / "build" / "libklt_ref.so"
MAIN = HERE / "build" / "klt_ref_main"

OK, TEMPLATE_OUT, LOST, FLAT, BIDIR = 0, 1, 2, 3, 4
STOP_NONE, STOP_EPS, STOP_OSC, STOP_MAXIT = 0, 1, 2, 3
MAX_LEVELS = 6
LV_NOT_RUN = 255
INFO_DTYPE = np.dtype([("status", "u1"), ("stop", "u1"), ("iterations", "u1"), ("levels_skipped", "u1"), ("bidir_error", "<f4")])
DEFAULTS = dict(levels=3, block=(31, 31), max_it=30, max_bidir=float("inf"))

_lib = None


def build(target: str = "all") -> None:
    subprocess.run(["make", "-s", "-C", str(HERE), target], check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(str(LIB))
        P = C.POINTER
        L.klt_ref_layout.argtypes = [C.c_int, C.c_int, C.c_int, P(C.c_long)]
        L.klt_ref_layout.restype = C.c_long
        L.klt_ref_pyramid.argtypes = [P(C.c_uint8), C.c_int, C.c_int, C.c_int, P(C.c_uint8)]
        L.klt_ref_pyramid.restype = None
        L.klt_ref_track.argtypes = [P(C.c_uint8), P(C.c_uint8), C.c_int, C.c_int, P(C.c_float), P(C.c_float), C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_float, P(C.c_float), P(C.c_uint8), P(C.c_float), C.c_void_p, P(C.c_uint8)]
        L.klt_ref_track.restype = None
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def level_dims(rows: int, cols: int, levels: int):
    out = []
    for _ in range(levels):
        out.append((rows, cols))
        rows, cols = (rows + 1) // 2, (cols + 1) // 2
    return out


def _pyr_flat(img: np.ndarray, levels: int) -> np.ndarray:
    img = np.ascontiguousarray(img, np.uint8)
    rows, cols = img.shape
    total = lib().klt_ref_layout(rows, cols, levels, None)
    out = np.zeros(total, np.uint8)
    lib().klt_ref_pyramid(_p(img, C.c_uint8), rows, cols, levels, _p(out, C.c_uint8))
    return out


def pyramid(img: np.ndarray, levels: int) -> list:
    flat = _pyr_flat(img, levels)
    out, o = [], 0
    for r, c in level_dims(*img.shape, levels):
        out.append(flat[o:o + r * c].reshape(r, c).copy())
        o += r * c
    return out


def track(img0, img1, pts, guess=None, levels=3, block=(31, 31), max_it=30, max_bidir=float("inf")) -> dict:
    """-> dict(pts1 [n, 2] f32, valid [n] bool, scores [n] f32, info [n] INFO_DTYPE, level_codes [n, 6] u8:
    the forward pass' record per level -- a STOP_* code for a level that iterated to a stop, 16 + status
    for one that ended otherwise, 255 for a level the call does not have)."""
    img0, img1 = np.ascontiguousarray(img0, np.uint8), np.ascontiguousarray(img1, np.uint8)
    assert img0.shape == img1.shape and img0.ndim == 2
    rows, cols = img0.shape
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    g = None if guess is None else np.ascontiguousarray(guess, np.float32).reshape(-1, 2)
    n = len(pts)
    p0, p1 = _pyr_flat(img0, levels), _pyr_flat(img1, levels)
    out = np.zeros((max(n, 1), 2), np.float32)
    valid = np.zeros(max(n, 1), np.uint8)
    scores = np.zeros(max(n, 1), np.float32)
    info = np.zeros(max(n, 1), INFO_DTYPE)
    codes = np.zeros((max(n, 1), MAX_LEVELS), np.uint8)
    lib().klt_ref_track(_p(p0, C.c_uint8), _p(p1, C.c_uint8), rows, cols, _p(pts, C.c_float), _p(g, C.c_float) if g is not None else None,
                        n, int(levels), int(block[0]), int(block[1]), int(max_it), float(max_bidir), _p(out, C.c_float),
                        _p(valid, C.c_uint8), _p(scores, C.c_float), info.ctypes.data, _p(codes, C.c_uint8))
    return dict(pts1=out[:n], valid=valid[:n].astype(bool), scores=scores[:n], info=info[:n], level_codes=codes[:n])


def write_problem(path, img0, img1, pts, guess=None, levels=3, block=(31, 31), max_it=30, max_bidir=float("inf")) -> None:
    """The file tests/klt_ref/klt_ref_main.c reads."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    rows, cols = img0.shape
    with open(path, "wb") as f:
        f.write(np.array([rows, cols, len(pts), levels, block[0], block[1], max_it, guess is not None], np.int32).tobytes())
        f.write(np.array([max_bidir], np.float32).tobytes())
        f.write(np.ascontiguousarray(img0, np.uint8).tobytes())
        f.write(np.ascontiguousarray(img1, np.uint8).tobytes())
        f.write(pts.tobytes())
        if guess is not None:
            f.write(np.ascontiguousarray(guess, np.float32).reshape(-1, 2).tobytes())


def main_lines(rec: dict) -> list:
    """A track() record as klt_ref_main prints it."""
    out = []
    for i in range(len(rec["pts1"])):
        w = rec["pts1"][i].view(np.uint32)
        inf = rec["info"][i]
        out.append("%08x %08x %d %08x %d %d %d %d %08x" % (w[0], w[1], int(rec["valid"][i]), rec["scores"][i:i + 1].view(np.uint32)[0],
                                                           inf["status"], inf["stop"], inf["iterations"], inf["levels_skipped"],
                                                           rec["info"]["bidir_error"][i:i + 1].view(np.uint32)[0]))
    return out


# --------------------------------------------------------------------------- generated images
@functools.lru_cache(maxsize=None)
def field(rows: int, cols: int, seed: int) -> np.ndarray:
    """Band-limited noise: white noise through a Gaussian of sigma 1.5 px (periodic), sd 40 about 128; float64."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((rows, cols))
    fy, fx = np.fft.fftfreq(rows)[:, None], np.fft.fftfreq(cols)[None, :]
    g = np.exp(-2.0 * (np.pi * 1.5) ** 2 * (fx * fx + fy * fy))
    f = np.fft.ifft2(np.fft.fft2(w) * g).real
    f.setflags(write=False)
    return f


def render(f: np.ndarray, dx: float = 0.0, dy: float = 0.0, noise_sd: float = 0.0, seed: int = 0) -> np.ndarray:
    """The field moved by (dx, dy) px (content at x appears at x + dx) by Fourier phase, scaled to sd 40 about
    128, plus white noise of noise_sd grey levels, rounded and clipped to u8."""
    rows, cols = f.shape
    fy, fx = np.fft.fftfreq(rows)[:, None], np.fft.fftfreq(cols)[None, :]
    s = np.fft.ifft2(np.fft.fft2(f) * np.exp(-2j * np.pi * (fx * dx + fy * dy))).real
    img = 128.0 + 40.0 * s / f.std()
    if noise_sd:
        img = img + np.random.default_rng(seed).standard_normal(f.shape) * noise_sd
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def interior_points(rows: int, cols: int, n: int, seed: int, margin: float = 24.0) -> np.ndarray:
    """n random 1-based points at least `margin` px from every side (float positions, a few on integers)."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(margin + 1, cols - margin, n), rng.uniform(margin + 1, rows - margin, n)], 1).astype(np.float32)
    p[::7] = np.rint(p[::7])                    # integer coordinates: w00 = 16384
    return p


def side_points(rows: int, cols: int, block) -> np.ndarray:
    """Points whose windows are clipped by each of the four sides, corners included, and points outside the
    image, far enough on each side for the template corner to be out."""
    bh, bw = block
    xs = [1.0, 2.5, cols / 2.0 + 0.25, cols - 1.5, float(cols)]
    ys = [1.0, 2.25, rows / 2.0 + 0.5, rows - 1.25, float(rows)]
    p = [(x, y) for x in xs for y in ys if not (x == xs[2] and y == ys[2])]
    far_x, far_y = bw + 2.0, bh + 2.0
    p += [(-far_x, rows / 2.0), (cols + far_x, rows / 2.0), (cols / 2.0, -far_y), (cols / 2.0, rows + far_y),
          (-0.5, rows / 2.0), (cols + 1.5, rows / 2.0), (cols / 2.0, 0.25), (cols / 2.0, rows + 1.75)]
    return np.array(p, np.float32)


SHIFT = (3.25, -2.5)
SIZES = {"a": (97, 121), "b": (64, 64)}


@functools.lru_cache(maxsize=None)
def images(key: str):
    """key -> (img0, img1): 'a' / 'b' the two sizes; ':same' identical, ':const' constant, ':s<sd>' the copy
    shifted by SHIFT with noise sd, ':far' the copy shifted by (30, 0)."""
    size, kind = key.split(":")
    rows, cols = SIZES[size]
    f = field(rows, cols, 11 if size == "a" else 12)
    img0 = render(f)
    if kind == "same":
        img1 = img0.copy()
    elif kind == "const":
        img0 = np.full((rows, cols), 93, np.uint8)
        img1 = img0.copy()
    elif kind == "far":
        img1 = render(f, 30.0, 0.0)
    else:
        img1 = render(f, SHIFT[0], SHIFT[1], float(kind[1:]), seed=100 + int(kind[1:]))
    for a in (img0, img1):
        a.setflags(write=False)
    return img0, img1


@functools.lru_cache(maxsize=None)
def table() -> tuple:
    """Rows dict(name, images, pts, guess, params, shift, compare): `shift` the true motion (None where the
    row has none), `compare` whether the row enters the comparison with the float64 restatement (interior
    points, windows >= 11, noise <= 8)."""
    rows = []

    def add(name, key, pts, guess=None, shift=None, compare=False, **params):
        pts = np.ascontiguousarray(pts, np.float32)
        assert len(pts) <= 200
        pts.setflags(write=False)
        rows.append(dict(name=name, images=key, pts=pts, guess=guess, params=dict(DEFAULTS, **params), shift=shift, compare=compare))

    ra, ca = SIZES["a"]
    rb, cb = SIZES["b"]
    ia = interior_points(ra, ca, 80, 1)
    ib = interior_points(rb, cb, 40, 2)
    add("same_a_31_L3", "a:same", np.concatenate([ia, side_points(ra, ca, (31, 31))[:24]]), shift=(0.0, 0.0))
    add("same_b_5_L1", "b:same", interior_points(rb, cb, 40, 3, 4.0), shift=(0.0, 0.0), levels=1, block=(5, 5))
    add("shift_a_31_L3", "a:s0", ia, shift=SHIFT, compare=True)
    add("shift_a_31_L3_n8", "a:s8", ia, shift=SHIFT, compare=True)
    add("shift_a_11_L3", "a:s0", ia, shift=SHIFT, compare=True, block=(11, 11))
    add("shift_a_11_L3_n8", "a:s8", ia, shift=SHIFT, compare=True, block=(11, 11))
    add("shift_a_7x21_L3", "a:s0", ia, shift=SHIFT, block=(7, 21))
    add("shift_a_21x7_L3", "a:s0", ia, shift=SHIFT, block=(21, 7))
    add("shift_b_31_L3", "b:s0", ib, shift=SHIFT, compare=True)
    add("shift_a_31_L1", "a:s0", ia, shift=SHIFT, compare=True, levels=1)
    add("shift_a_31_L6", "a:s0", ia, shift=SHIFT, compare=True, levels=6)
    add("shift_a_15_L6", "a:s8", ia, shift=SHIFT, compare=True, levels=6, block=(15, 15))
    add("shift_a_31_it1", "a:s0", ia, shift=SHIFT, max_it=1)
    add("sides_a_31_L3", "a:s0", side_points(ra, ca, (31, 31)), shift=SHIFT)
    add("sides_a_31_L1", "a:s0", side_points(ra, ca, (31, 31)), shift=SHIFT, levels=1)
    add("sides_a_5_L3", "a:s0", side_points(ra, ca, (5, 5)), shift=SHIFT, block=(5, 5))
    add("sides_a_7x21_L6", "a:s8", side_points(ra, ca, (7, 21)), shift=SHIFT, block=(7, 21), levels=6)
    add("sides_b_31_L3", "b:s0", side_points(rb, cb, (31, 31)), shift=SHIFT)
    add("noisy_a_5_L3", "a:s25", interior_points(ra, ca, 200, 4, 6.0), shift=SHIFT, block=(5, 5))
    add("noisy_a_5_L1_n8", "a:s8", interior_points(ra, ca, 200, 5, 6.0), shift=SHIFT, block=(5, 5), levels=1)
    add("const_b_31_L3", "b:const", ib, shift=None)
    add("const_b_5_L1", "b:const", side_points(rb, cb, (5, 5)), shift=None, levels=1, block=(5, 5))
    far = interior_points(ra, ca, 60, 6, 24.0)
    far = far[far[:, 0] < ca - 24.0 - 30.0]
    add("far_a_11_L1", "a:far", far, shift=(30.0, 0.0), levels=1, block=(11, 11))
    add("far_a_11_L1_guess", "a:far", far, guess=(far + np.float32([30.0, 0.0])).astype(np.float32), shift=(30.0, 0.0), levels=1,
        block=(11, 11))
    add("bidir_a_31_L3", "a:s0", ia, shift=SHIFT, max_bidir=0.5)
    add("bidir_a_5_L3_n25", "a:s25", interior_points(ra, ca, 200, 4, 6.0), shift=SHIFT, block=(5, 5), max_bidir=0.1)
    add("bidir_sides_a_11", "a:s8", side_points(ra, ca, (11, 11)), shift=SHIFT, block=(11, 11), max_bidir=1.0)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def results() -> tuple:
    """The reference's record for every table row (computed once; treat as read-only)."""
    out = []
    for row in table():
        img0, img1 = images(row["images"])
        rec = track(img0, img1, row["pts"], row["guess"], **row["params"])
        for v in rec.values():
            v.setflags(write=False)
        out.append(rec)
    return tuple(out)
