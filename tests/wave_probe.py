"""ctypes driver of the device probe of the wave and block collectives (tests/wave_probe/wave_probe.hip: thin
kernels around csrc/wave.h and csrc/match_merge.h, one call per thread, every thread's return value stored)
and the NumPy restatements the device is compared with.  Test infrastructure, built on demand like
tests/corner_ref.py; `VO_WAVE_PROBE_LIB` names another build of the probe (a copy of the headers under test).

Arrays are [nblocks][rounds][NWAVES * 64]: a block runs its `rounds` slices in turn inside one launch.  Every
restatement works in the value's own dtype, so an integer sum wraps as the device's does and a float sum
rounds where the device's does; tests/test_wave_ref.py holds them to independent references.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "wave_probe"
LIB = HERE / "build" / "libwave_probe.so"

FN = {name: k for k, name in enumerate((
    "wave_sum", "wave_sum_xor", "wave_sum_xor_n", "wave_max", "wave_min", "wave_incl_scan", "wave_rank",
    "block_excl_scan", "block_sum", "block_exscan_1024", "block_exscan_256", "top2c_merge_lanes", "top2s_merge_wave",
    "match_place"))}
TY = {np.dtype(np.int32): 0, np.dtype(np.uint32): 1, np.dtype(np.float32): 2, np.dtype(np.int64): 3, np.dtype(np.float64): 4}
XOR_N = {np.dtype(np.int32): 3, np.dtype(np.float64): 28}       # the two wave_sum_xor<N> the probe instantiates
I32, U32, F32 = np.dtype(np.int32), np.dtype(np.uint32), np.dtype(np.float32)

_lib = None


def build() -> None:
    subprocess.run(["make", "-s", "-C", str(HERE)], check=True)


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("VO_WAVE_PROBE_LIB")
        if not path:
            build()
            path = str(LIB)
        L = C.CDLL(path)
        L.wave_probe_run.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.wave_probe_run.restype = C.c_int
        _lib = L
    return _lib


def _out_dtypes(fn: str, dt: np.dtype):
    return {"wave_rank": (I32, I32), "block_excl_scan": (U32, U32), "block_exscan_1024": (U32, U32),
            "block_exscan_256": (U32,), "top2c_merge_lanes": (F32, I32, F32), "top2s_merge_wave": (F32, I32, F32),
            "match_place": (U32, U32)}.get(fn, (dt,))


def run(fn: str, *ins: np.ndarray, nwaves: int):
    """One launch of collective `fn`: ins[k] is [nblocks][rounds][nwaves * 64] (wave_sum_xor_n: a last axis of N).
    Returns the output arrays, shaped like ins[0]."""
    ins = [np.ascontiguousarray(a) for a in ins]
    x = ins[0]
    nblocks, rounds, width = x.shape[:3]
    assert width == nwaves * 64 and all(a.shape == x.shape for a in ins)
    assert x.ndim == (4 if fn == "wave_sum_xor_n" else 3)
    outs = [np.empty(x.shape, dt) for dt in _out_dtypes(fn, x.dtype)]
    host = (C.c_void_p * 6)()
    size = (C.c_size_t * 6)()
    for k, a in enumerate(ins):
        host[k], size[k] = a.ctypes.data, a.nbytes
    for k, a in enumerate(outs):
        host[3 + k], size[3 + k] = a.ctypes.data, a.nbytes
    err = lib().wave_probe_run(FN[fn], TY[x.dtype], nwaves, nblocks, rounds, host, size)
    if err:
        raise RuntimeError(f"wave_probe_run({fn}, {x.dtype}, nwaves={nwaves}) returned {err}")
    return outs


# ---------------------------------------------------------------- the restatements
OFFS = (32, 16, 8, 4, 2, 1)


def tree_sum(x: np.ndarray) -> np.ndarray:
    """[..., 64] -> [...]: p[l] = p[l] + p[l + off] for off = 32 .. 1 in x's dtype; the result is p[0]."""
    q = np.array(x, copy=True)
    with np.errstate(all="ignore"):
        for off in OFFS:
            q[..., :off] = q[..., :off] + q[..., off:2 * off]
    return q[..., 0].copy()


def seq_sum(x: np.ndarray) -> np.ndarray:
    """[..., 64] -> [...]: left to right, in x's dtype (what the tree must differ from on the float families)."""
    s = x[..., 0].copy()
    with np.errstate(all="ignore"):
        for l in range(1, x.shape[-1]):
            s = s + x[..., l]
    return s


def rev_tree_sum(x: np.ndarray) -> np.ndarray:
    """The tree with its levels reversed (off = 1 .. 32: neighbours first), in x's dtype."""
    q = np.array(x, copy=True)
    with np.errstate(all="ignore"):
        while q.shape[-1] > 1:
            q = q[..., 0::2] + q[..., 1::2]
    return q[..., 0].copy()


def per_wave(x: np.ndarray) -> np.ndarray:
    """[..., nwaves * 64] -> [..., nwaves, 64]"""
    return x.reshape(x.shape[:-1] + (x.shape[-1] // 64, 64))


def every_lane(r: np.ndarray, like: np.ndarray) -> np.ndarray:
    """one value per wave [..., nwaves] -> the same value in each of its lanes, shaped like `like`"""
    return np.repeat(r, 64, axis=-1).reshape(like.shape)


def wave_sum(x: np.ndarray) -> np.ndarray:
    return every_lane(tree_sum(per_wave(x)), x)


def wave_sum_n(x: np.ndarray) -> np.ndarray:
    """[..., nwaves * 64, N]: N trees side by side"""
    w = np.moveaxis(x.reshape(x.shape[:-2] + (x.shape[-2] // 64, 64, x.shape[-1])), -1, -2)    # [..., nwaves, N, 64]
    r = tree_sum(w)                                                                             # [..., nwaves, N]
    return np.repeat(r[..., None, :], 64, axis=-2).reshape(x.shape)


def wave_max(x: np.ndarray) -> np.ndarray:
    """fmaxf's rule for floats: a NaN lane does not count; NaN only if every lane is NaN"""
    with np.errstate(all="ignore"):
        return every_lane(np.fmax.reduce(per_wave(x), axis=-1), x)


def wave_min(x: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return every_lane(np.fmin.reduce(per_wave(x), axis=-1), x)


def wave_incl_scan(x: np.ndarray) -> np.ndarray:
    return np.cumsum(per_wave(x).view(np.uint32), axis=-1, dtype=np.uint32).view(x.dtype).reshape(x.shape)


def wave_rank(pred: np.ndarray):
    """popcount below the lane, and the wave's count in every lane"""
    p = per_wave(pred != 0).astype(np.int32)
    c = np.cumsum(p, axis=-1, dtype=np.int32)
    return (c - p).reshape(pred.shape), every_lane(c[..., -1], pred)


def block_excl_scan(x: np.ndarray):
    """uint32 [..., B] -> (exclusive prefix sums in thread order, the block's total in every thread), mod 2^32"""
    c = np.cumsum(x, axis=-1, dtype=np.uint32)
    return c - x, np.broadcast_to(c[..., -1:], x.shape).copy()


def block_sum(x: np.ndarray) -> np.ndarray:
    """the per-wave tree, then the waves' totals added left to right, in x's dtype"""
    t = tree_sum(per_wave(x))
    s = t[..., 0].copy()
    with np.errstate(all="ignore"):
        for w in range(1, t.shape[-1]):
            s = s + t[..., w]
    return np.broadcast_to(s[..., None], x.shape).copy()


def block_seq_sum(x: np.ndarray) -> np.ndarray:
    return seq_sum(x)


def block_rev_sum(x: np.ndarray) -> np.ndarray:
    """block_sum with the reversed tree inside the waves"""
    t = rev_tree_sum(per_wave(x))
    return seq_sum(t)


def top2c_union(cands):
    """cands: (best, idx, second) triples of the cosine ranking.  Lexicographic best on (value descending,
    index ascending) and the second largest value of the union multiset, by sorting."""
    b, i, _ = sorted(cands, key=lambda c: (-c[0], c[1]))[0]
    vals = sorted((v for c in cands for v in (c[0], c[2])), reverse=True)
    return b, i, vals[1]


def top2s_union(cands):
    """The SSD ranking: lexicographic best on (value, index) ascending over the triples that hold a column
    (idx >= 0), (inf, -1) if none does, and the second smallest value of the union multiset."""
    vals = sorted(v for c in cands for v in (c[0], c[2]))
    held = sorted((c for c in cands if c[1] >= 0), key=lambda c: (c[0], c[1]))
    b, i = (held[0][0], held[0][1]) if held else (float("inf"), -1)
    return b, i, vals[1]


def top2c_merge_lanes(b: np.ndarray, i: np.ndarray, s: np.ndarray):
    """lane l joined with lane l ^ 32, for every lane"""
    wb, wi, ws = per_wave(b), per_wave(i), per_wave(s)
    ob, oi, os_ = np.empty_like(wb), np.empty_like(wi), np.empty_like(ws)
    for w in np.ndindex(wb.shape[:-1]):
        for l in range(64):
            m = l ^ 32
            ob[w][l], oi[w][l], os_[w][l] = top2c_union([(float(wb[w][l]), int(wi[w][l]), float(ws[w][l])),
                                                         (float(wb[w][m]), int(wi[w][m]), float(ws[w][m]))])
    return ob.reshape(b.shape), oi.reshape(i.shape), os_.reshape(s.shape)


def top2s_merge_wave(b: np.ndarray, i: np.ndarray, s: np.ndarray):
    """the wave's 64 triples joined; the same result in every lane"""
    wb, wi, ws = per_wave(b), per_wave(i), per_wave(s)
    ob, oi, os_ = np.empty_like(wb), np.empty_like(wi), np.empty_like(ws)
    for w in np.ndindex(wb.shape[:-1]):
        ob[w][:], oi[w][:], os_[w][:] = top2s_union([(float(wb[w][l]), int(wi[w][l]), float(ws[w][l])) for l in range(64)])
    return ob.reshape(b.shape), oi.reshape(i.shape), os_.reshape(s.shape)


def match_place(ok: np.ndarray):
    """[nblocks][rounds][256] flags -> (position of every thread, base after the round in every thread): a
    round's accepted rows in thread order after the rows of the rounds before it"""
    p = (ok != 0).astype(np.uint32)
    pos, base_out = np.empty(ok.shape, np.uint32), np.empty(ok.shape, np.uint32)
    base = np.zeros((ok.shape[0], 1), np.uint32)
    for r in range(ok.shape[1]):
        c = np.cumsum(p[:, r], axis=-1, dtype=np.uint32)
        pos[:, r] = base + c - p[:, r]
        base = base + c[:, -1:]
        base_out[:, r] = base
    return pos, base_out


# ---------------------------------------------------------------- input families shared by the CPU and GPU suites
# Seeds at which every sum of the family differs in bits from the left-to-right sum and from the reversed tree
# (tests/test_wave_ref.py asserts it), so that a device sum in another order cannot pass.
WAVE_SEED = {np.dtype(np.float32): 88, np.dtype(np.float64): 28}
BLOCK_NWAVES = (1, 2, 3, 4, 16)
BLOCK_SEED = {(np.dtype(np.float32), nw): s for nw, s in zip(BLOCK_NWAVES, (3, 11, 18, 11, 5))}
BLOCK_SEED.update({(np.dtype(np.float64), nw): s for nw, s in zip(BLOCK_NWAVES, (9, 8, 11, 3, 3))})
XOR28_SEED = 0      # wave_sum_xor<28>: 28 sums per wave; at least half of each wave's differ from either other order


def mixed(dtype, shape, seed: int) -> np.ndarray:
    """mixed-sign values over six decades: the order of the additions shows in the last bits"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(dtype)


def wave_family(dtype) -> np.ndarray:
    """[2][1][256]: eight waves"""
    return mixed(dtype, (2, 1, 256), WAVE_SEED[np.dtype(dtype)])


def block_family(dtype, nwaves: int) -> np.ndarray:
    """[2][2][nwaves * 64]: two blocks, two calls each"""
    return mixed(dtype, (2, 2, nwaves * 64), BLOCK_SEED[(np.dtype(dtype), nwaves)])


def xor28_family() -> np.ndarray:
    """[2][1][256][28] float64"""
    return mixed(np.float64, (2, 1, 256, 28), XOR28_SEED)


def rank_masks(seed: int = 5) -> np.ndarray:
    """[n][64] 0/1: no lane, all lanes, alternating (both phases), one row of 16 only (each row), random masks, then
    one lane k for every k"""
    rng = np.random.default_rng(seed)
    lane = np.arange(64)
    rows = [np.zeros(64, bool), np.ones(64, bool), lane % 2 == 0, lane % 2 == 1]
    rows += [lane // 16 == r for r in range(4)]
    rows += [rng.random(64) < 0.5, rng.random(64) < 0.1, rng.random(64) < 0.9, rng.random(64) < 0.5]
    rows += [lane == k for k in range(64)]
    return np.array(rows).astype(np.int32)
