"""ctypes driver of the CPU reference of triangulate's reprojectionErrors / validIndex
(tests/tri_quality_ref/tri_quality_ref.c: include/vo_spec.h's vo_tri_quality, the function the
kernel calls, over arrays).  Test infrastructure, built on demand like tests/describe_ref.py.

`quality(x1, x2, X, P1, P2)` -> (err float32 [n], valid bool [n]) for X as vo_triangulate returns it.
`quality_longdouble` is the same formula in numpy.longdouble, written from include/vo.h, and
`same_class` / PROBE_* are what the CPU and GPU tests share."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "tri_quality_ref"
LIB = HERE / "build" / "libtri_quality_ref.so"

_lib = None

# the four probe pairs under the KITTI calibration: negative disparity (behind the cameras, yet a
# perfect reprojection), zero disparity, half a pixel of row offset, zero disparity off-centre
PROBE_X1 = np.array([[600, 180], [600, 180], [600, 180], [100, 50]], np.float32)
PROBE_X2 = np.array([[610, 180], [600, 180], [590, 180.5], [100, 50]], np.float32)


def build() -> None:
    subprocess.run(["make", "-s", "-C", str(HERE)], check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(str(LIB))
        P = C.POINTER
        L.tri_quality_ref.argtypes = [P(C.c_float), P(C.c_float), P(C.c_double), C.c_int, P(C.c_double), P(C.c_double),
                                      P(C.c_float), P(C.c_uint8)]
        L.tri_quality_ref.restype = None
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def quality(x1, x2, X, P1, P2):
    x1 = np.ascontiguousarray(x1, np.float32).reshape(-1, 2)
    x2 = np.ascontiguousarray(x2, np.float32).reshape(-1, 2)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    P1 = np.ascontiguousarray(P1, np.float64).reshape(12)
    P2 = np.ascontiguousarray(P2, np.float64).reshape(12)
    n = x1.shape[0]
    assert x2.shape[0] == n and X.shape[0] == n
    err = np.zeros(n, np.float32)
    valid = np.zeros(n, np.uint8)
    lib().tri_quality_ref(_p(x1, C.c_float), _p(x2, C.c_float), _p(X, C.c_double), n, _p(P1, C.c_double), _p(P2, C.c_double),
                          _p(err, C.c_float), _p(valid, C.c_uint8))
    return err, valid.astype(bool)


def quality_longdouble(x1, x2, X, P1, P2):
    """The formula of include/vo.h in numpy.longdouble -> (err longdouble [n], valid bool [n])."""
    LD = np.longdouble
    X = np.asarray(X, np.float64).reshape(-1, 3).astype(LD)
    e = []
    ok = np.ones(len(X), bool)
    with np.errstate(all="ignore"):
        for x, P in ((x1, P1), (x2, P2)):
            x = np.asarray(x, np.float32).reshape(-1, 2).astype(LD)
            P = np.asarray(P, np.float64).reshape(3, 4).astype(LD)
            h = X @ P[:, :3].T + P[:, 3]
            du, dv = h[:, 0] / h[:, 2] - x[:, 0], h[:, 1] / h[:, 2] - x[:, 1]
            e.append(np.sqrt(du * du + dv * dv))
            ok &= h[:, 2] > 0
        return (e[0] + e[1]) * LD(0.5), ok


def same_class(got, ref) -> None:
    """Finite values by bytes, the others by kind (nan, +inf, -inf): NaN sign and payload are not
    part of the spec."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    assert got[fin].tobytes() == ref[fin].tobytes()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref))
