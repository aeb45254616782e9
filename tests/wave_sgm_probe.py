"""ctypes driver of the device probe of csrc/wave.h's 64-lane shifts (tests/wave_sgm_probe/wave_sgm_probe.hip: thin
kernels, one call per thread, every thread's return value stored) and the NumPy restatements the device is
compared with.  Test infrastructure, built on demand like tests/wave_probe.py."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "wave_sgm_probe"
LIB = HERE / "build" / "libwave_sgm_probe.so"
FN = {"shift_up": 0, "shift_down": 1, "min_and_neighbours": 2}
TY = {np.dtype(np.uint32): 0, np.dtype(np.float32): 1}

_lib = None


def build() -> None:
    subprocess.run(["make", "-s", "-C", str(HERE)], check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        try:                                   # one HIP runtime per process: torch's, as vo.load_library binds libvo
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(str(LIB))
        L.wave_sgm_probe_run.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5
        L.wave_sgm_probe_run.restype = C.c_int
        _lib = L
    return _lib


def run(fn: str, x: np.ndarray, fill, nwaves: int):
    """x [nblocks][nwaves * 64] uint32 or float32 -> the output array(s), shaped like x"""
    x = np.ascontiguousarray(x)
    nblocks, width = x.shape
    assert width == nwaves * 64
    f = np.array([fill], x.dtype)
    outs = [np.empty_like(x) for _ in range(3 if fn == "min_and_neighbours" else 1)]
    ptr = [o.ctypes.data for o in outs] + [None, None]
    rc = lib().wave_sgm_probe_run(FN[fn], TY[x.dtype], nwaves, nblocks, x.ctypes.data, f.ctypes.data, ptr[0], ptr[1], ptr[2])
    assert rc == 0, rc
    return outs if len(outs) > 1 else outs[0]


# ---- NumPy restatements: x [..., nwaves * 64], each wave of 64 on its own ----
def shift_up(x: np.ndarray, fill) -> np.ndarray:
    w = x.reshape(x.shape[:-1] + (-1, 64))
    out = np.empty_like(w)
    out[..., 1:] = w[..., :-1]
    out[..., 0] = fill
    return out.reshape(x.shape)


def shift_down(x: np.ndarray, fill) -> np.ndarray:
    w = x.reshape(x.shape[:-1] + (-1, 64))
    out = np.empty_like(w)
    out[..., :-1] = w[..., 1:]
    out[..., 63] = fill
    return out.reshape(x.shape)


def wave_min(x: np.ndarray) -> np.ndarray:
    w = x.reshape(x.shape[:-1] + (-1, 64))
    return np.broadcast_to(w.min(axis=-1, keepdims=True), w.shape).reshape(x.shape)
