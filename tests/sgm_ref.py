"""CPU reference of vo_disparity_sgm / vo_reconstruct_scene for the tests: the ctypes binding of tests/sgm_ref
(include/vo_spec.h's vo_sgm_* / vo_reconstruct_* functions built for the host), the image generators, the case
table and the names of the branch counters the reference returns.  tests/sgm_np_ref.py is the independent
restatement the reference is held to; the device is held to the reference by bytes."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "sgm_ref"
LIB = HERE / "build" / "libsgm_ref.so"
MAIN = HERE / "build" / "sgm_ref_main"

DEFAULTS = dict(P1=10, P2=120, U=15)
NAN_BITS = 0x7FC00000

# the counters of sgm_ref.c
C_FIRST, C_ARG, C_NO_LOWER, C_NO_UPPER, C_TIE, C_K_FIRST, C_K_LAST, C_DEN_ZERO = 0, 8, 40, 41, 42, 43, 44, 45
C_PLUS_HALF, C_MINUS_HALF, C_INVALID_LEFT, C_INVALID_RIGHT, C_UNRELIABLE, C_V_ZERO, C_RETURNED, C_SUBPIXEL = 46, 47, 48, 49, 50, 51, 52, 53
N_COUNTERS = 56

_lib = None


def build(target: str = "all") -> None:
    subprocess.run(["make", "-s", "-C", str(HERE), target], check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(str(LIB))
        P = C.POINTER
        L.sgm_ref_disparity.argtypes = [P(C.c_uint8), P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        P(C.c_uint16), P(C.c_float), P(C.c_int64)]
        L.sgm_ref_reconstruct.argtypes = [P(C.c_float), C.c_int, C.c_int, C.c_int, P(C.c_double), P(C.c_float)]
        L.sgm_ref_reconstruct.restype = None
        L.sgm_ref_reprojection.argtypes = [P(C.c_double), P(C.c_double), P(C.c_double)]
        L.sgm_ref_select.argtypes = [P(C.c_uint16), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.sgm_ref_select.restype = C.c_float
        L.sgm_ref_step.argtypes = [C.c_int] * 7
        L.sgm_ref_census.argtypes = [P(C.c_uint8), C.c_int, C.c_int, P(C.c_uint64)]
        L.sgm_ref_census.restype = None
        assert L.sgm_ref_n_counters() == N_COUNTERS
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def disparity(left, right, dmin: int, D: int, P1: int = 10, P2: int = 120, U: int = 15) -> dict:
    """-> dict(S [rows, cols, D] uint16, disp [rows, cols] float32, counters [N_COUNTERS] int64)"""
    left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
    rows, cols = left.shape
    S = np.zeros((rows, cols, D), np.uint16)
    disp = np.zeros((rows, cols), np.float32)
    n = np.zeros(N_COUNTERS, np.int64)
    rc = lib().sgm_ref_disparity(_p(left, C.c_uint8), _p(right, C.c_uint8), rows, cols, dmin, D, P1, P2, U, _p(S, C.c_uint16),
                                 _p(disp, C.c_float), _p(n, C.c_int64))
    assert rc == 0
    return dict(S=S, disp=disp, counters=n)


def census(img) -> np.ndarray:
    img = np.ascontiguousarray(img, np.uint8)
    out = np.zeros(img.shape, np.uint64)
    lib().sgm_ref_census(_p(img, C.c_uint8), img.shape[0], img.shape[1], _p(out, C.c_uint64))
    return out


def select(S, dmin: int, x: int, cols: int, U: int) -> np.float32:
    S = np.ascontiguousarray(S, np.uint16)
    return np.float32(lib().sgm_ref_select(_p(S, C.c_uint16), S.size, dmin, x, cols, U))


def step(c, lk, lm, lp, m, P1, P2) -> int:
    return lib().sgm_ref_step(c, lk, lm, lp, m, P1, P2)


def reconstruct(disp, Q) -> np.ndarray:
    """disp [rows, cols] float32, C- or Fortran-ordered -> xyz [rows, cols, 3] in the same order"""
    disp = np.asarray(disp, np.float32)
    col_major = int(disp.flags.f_contiguous and not disp.flags.c_contiguous)
    if not col_major:
        disp = np.ascontiguousarray(disp)
    rows, cols = disp.shape
    q = np.ascontiguousarray(np.asarray(Q, np.float64).reshape(-1))
    out = np.zeros((rows, cols, 3), np.float32, order="F" if col_major else "C")
    lib().sgm_ref_reconstruct(_p(disp, C.c_float), rows, cols, col_major, _p(q, C.c_double), _p(out, C.c_float))
    return out


def reprojection(P1, P2):
    a = np.ascontiguousarray(np.asarray(P1, np.float64).reshape(-1))
    b = np.ascontiguousarray(np.asarray(P2, np.float64).reshape(-1))
    Q = np.zeros(16, np.float64)
    rc = lib().sgm_ref_reprojection(_p(a, C.c_double), _p(b, C.c_double), _p(Q, C.c_double))
    return rc, Q.reshape(4, 4)


# ---- images ----
KINDS = ("texture", "flat", "stripes", "step")


def _texture(rng, rows: int, width: int) -> np.ndarray:
    """random texture with structure at 1, 2 and 4 pixels"""
    t = rng.integers(0, 96, (rows, width)).astype(np.int32)
    t += np.repeat(np.repeat(rng.integers(0, 80, ((rows + 1) // 2, (width + 1) // 2)), 2, 0), 2, 1)[:rows, :width]
    t += np.repeat(np.repeat(rng.integers(0, 80, ((rows + 3) // 4, (width + 3) // 4)), 4, 0), 4, 1)[:rows, :width]
    return t.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pair(kind: str, rows: int, cols: int, dmin: int, D: int, seed: int = 0):
    """-> (left, right) uint8 [rows, cols]: left(y, x) = right(y, x - d) where the scene has disparity d"""
    rng = np.random.default_rng(1000 * seed + 7 * rows + 13 * cols + D + dmin + KINDS.index(kind))
    if kind == "texture":                       # one plane at disparity d0 inside the range
        d0 = dmin + D // 3
        T = _texture(rng, rows, cols + abs(d0))
        left, right = (T[:, :cols], T[:, d0:d0 + cols]) if d0 >= 0 else (T[:, -d0:-d0 + cols], T[:, :cols])
    elif kind == "flat":
        left = right = np.full((rows, cols), 128, np.uint8)
    elif kind == "stripes":                     # period 8, with independent noise of 0 .. 3 in either image
        base = np.where((np.arange(cols) // 4) % 2 == 0, 60, 200)[None, :].repeat(rows, 0)
        left = (base + rng.integers(0, 4, (rows, cols))).astype(np.uint8)
        right = (base + rng.integers(0, 4, (rows, cols))).astype(np.uint8)
    elif kind == "step":                        # a near rectangle in front of a far plane: an occlusion beside it
        db, df = dmin + D // 4, dmin + (3 * D) // 4
        pad = max(abs(db), abs(df)) + 1
        Tb, Tf = _texture(rng, rows, cols + 2 * pad), _texture(rng, rows, cols + 2 * pad)
        x = np.arange(cols)
        left = Tb[:, pad + x].copy()                                  # the far plane in left coordinates
        right = Tb[:, pad + np.clip(x + db, -pad, cols + pad - 1)].copy()   # right(x') = left(x' + db)
        y0, y1, x0, x1 = rows // 4, rows - rows // 4, cols // 3, cols - cols // 4
        left[y0:y1, x0:x1] = Tf[y0:y1, pad + x0:pad + x1]
        rx0, rx1 = max(x0 - df, 0), min(x1 - df, cols)
        if rx1 > rx0:
            right[y0:y1, rx0:rx1] = Tf[y0:y1, pad + rx0 + df:pad + rx1 + df]
    else:
        raise KeyError(kind)
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


# ---- the case table: rows x cols, D, dmin (what each reaches is in tests/test_gpu_sgm.py) ----
SHAPES = [(16, 16, 8, 0), (16, 20, 64, 0), (37, 53, 16, -4), (53, 37, 32, 0), (24, 150, 64, 0), (20, 200, 128, 3), (17, 65, 24, 0)]
VARIANTS = [dict(P1=0, P2=0), dict(P1=255, P2=255), dict(U=0), dict(U=100)]
VARIANT_SHAPE = (37, 53, 16, -4)


def table() -> list:
    """every shape on the four images at the defaults, then one shape at the parameter corners"""
    out = []
    for rows, cols, D, dmin in SHAPES:
        for kind in KINDS:
            out.append(dict(name=f"{rows}x{cols}_D{D}_{dmin}_{kind}", rows=rows, cols=cols, D=D, dmin=dmin, kind=kind, **DEFAULTS))
    rows, cols, D, dmin = VARIANT_SHAPE
    for v in VARIANTS:
        for kind in KINDS:
            p = dict(DEFAULTS, **v)
            tag = "_".join(f"{k}{val}" for k, val in v.items())
            out.append(dict(name=f"{rows}x{cols}_D{D}_{dmin}_{kind}_{tag}", rows=rows, cols=cols, D=D, dmin=dmin, kind=kind, **p))
    return out


TABLE = table()


@functools.lru_cache(maxsize=None)
def result(i: int) -> dict:
    """the reference's result of table row i, computed once and shared"""
    c = TABLE[i]
    left, right = pair(c["kind"], c["rows"], c["cols"], c["dmin"], c["D"])
    r = disparity(left, right, c["dmin"], c["D"], c["P1"], c["P2"], c["U"])
    for a in r.values():
        a.setflags(write=False)
    return r


# ---- the stand-alone sanitizer program's problem file and output ----
def write_problem(path, left, right, dmin, D, P1, P2, U) -> None:
    rows, cols = left.shape
    with open(path, "wb") as f:
        f.write(np.array([rows, cols, dmin, D, P1, P2, U], np.int32).tobytes())
        f.write(np.ascontiguousarray(left).tobytes())
        f.write(np.ascontiguousarray(right).tobytes())


def fnv1a(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def main_lines(r: dict) -> list:
    """what sgm_ref_main prints for a result: the hash of S's bytes, the counters, the hash of the map's bytes"""
    return [f"S {fnv1a(r['S'].tobytes()):016x}", "n " + " ".join(str(int(v)) for v in r["counters"]),
            f"disp {fnv1a(r['disp'].tobytes()):016x}"]
