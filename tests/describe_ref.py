"""ctypes driver of the CPU reference of vo_describe (tests/describe_ref/describe_ref.c: the oracle's
own build_pyramid / descriptor, reached by including oracle/sift_ref.c, behind the inverse keypoint
mapping of include/vo.h).  Test infrastructure, built on demand like tests/mexshim.py.

`describe(img, points, params)` -> [n, 128] uint8; `radius(scl)` is descriptor()'s uncapped window
radius of an octave-relative scale."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import oracle

HERE = Path(__file__).resolve().parent / "describe_ref"
LIB = HERE / "build" / "libdescribe_ref.so"

_lib = None


def build() -> None:
    subprocess.run(["make", "-s", "-C", str(HERE)], check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(str(LIB))
        P = C.POINTER
        L.describe_ref.argtypes = [P(C.c_uint8), C.c_int, C.c_int, C.c_int, P(oracle.SiftParams), P(oracle.Keypoint), C.c_int,
                                   P(C.c_uint8)]
        L.describe_ref.restype = C.c_int
        L.describe_ref_radius.argtypes = [C.c_float]
        L.describe_ref_radius.restype = C.c_int
        _lib = L
    return _lib


def describe(img: np.ndarray, points: np.ndarray, params=None) -> np.ndarray:
    img = np.ascontiguousarray(img, np.uint8)
    pts = np.ascontiguousarray(points)
    assert pts.dtype == oracle.KP_DTYPE and pts.ndim == 1
    p = params or oracle.sift_params()
    desc = np.zeros((len(pts), 128), np.uint8)
    n = lib().describe_ref(img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape[0], img.shape[1], img.shape[1], C.byref(p),
                           pts.ctypes.data_as(C.POINTER(oracle.Keypoint)), len(pts), desc.ctypes.data_as(C.POINTER(C.c_uint8)))
    if n == -1:
        raise ValueError("describe_ref: unsupported SIFT parameters")
    if n < 0:
        raise ValueError(f"describe_ref: point {-n - 2} names an octave or level outside the pyramid")
    return desc


def radius(scl: float) -> int:
    return int(lib().describe_ref_radius(float(np.float32(scl))))
