"""numpy restatement of the u8 matchFeatures spec with options, and the input
generators of the option tests (test_match_options.py, test_gpu_match_options.py).

Score matrix: sv(i, j) = 2 - 2 c(i, j), c(i, j) = ((float)dot(i, j) * inv|F1_i|) * inv|F2_j| in
float32, the two multiplies in exactly this order.  Forward step per F1 row: best and second-best
sv (a multiset; ties -> lowest j), accepted if best <= 0.04f * MatchThreshold and
best / second <= MaxRatio.  Unique (the toolbox's findUniqueIndices): back(j) = argmin_i sv(i, j)
over ALL F1 rows, first index on ties; an accepted (i, j) is kept iff back(j) == i.
matchMetric = sv of the kept pair.

`swapped_back=True` scores the backward pass as the forward kernel would with its two sides
exchanged, ((float)dot * inv|F2_j|) * inv|F1_i| -- NOT the spec; it exists to show that the operand
order decides near-ties (the crowded-column case).
"""
from __future__ import annotations

import functools

import numpy as np

F32 = np.float32

SHAPES = [(33, 129), (129, 33), (300, 257), (4100, 200), (200, 4100), (4100, 4100)]
DEGENERATE = [(1, 1), (2, 1), (0, 5), (5, 0)]
OPTIONS = [(1.0, 0.6), (5.0, 0.8), (25.0, 1.0)]          # (MatchThreshold, MaxRatio)


def _inv_norm(F: np.ndarray) -> np.ndarray:
    sq = (F.astype(np.int64) ** 2).sum(1)
    with np.errstate(divide="ignore"):
        inv = F32(1.0) / np.sqrt(sq.astype(F32))
    return np.where(sq > 0, inv, F32(0.0)).astype(F32)


def _dots(F1: np.ndarray, F2: np.ndarray) -> np.ndarray:
    """Exact integer dot products as int64.  Computed by a float64 matrix product: every partial
    sum is an integer below 128 * 255^2 < 2^53, so the product is exact in any summation order."""
    return np.rint(F1.astype(np.float64) @ F2.astype(np.float64).T).astype(np.int64)


def scores(F1: np.ndarray, F2: np.ndarray, swapped: bool = False) -> np.ndarray:
    """sv [n1, n2] float32 in spec operand order (swapped: the other order)."""
    d = _dots(F1, F2).astype(F32)                          # < 2^24: exact
    i1, i2 = _inv_norm(F1)[:, None], _inv_norm(F2)[None, :]
    c = (d * i2) * i1 if swapped else (d * i1) * i2
    return (F32(2.0) - F32(2.0) * c).astype(F32)


def forward(sv: np.ndarray, match_threshold: float, max_ratio: float):
    """-> (accepted mask [n1], best column [n1], best sv [n1])"""
    n1, n2 = sv.shape
    if n1 == 0 or n2 == 0:
        return np.zeros(n1, bool), np.zeros(n1, np.int64), np.zeros(n1, F32)
    j = np.argmin(sv, axis=1)                              # first index on ties
    best = sv[np.arange(n1), j]
    second = np.partition(sv, 1, axis=1)[:, 1] if n2 > 1 else np.full(n1, np.inf, F32)
    T = F32(match_threshold) * F32(0.04)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (best <= T) & ((best / second) <= F32(max_ratio))
    return ok, j, best


def match(F1: np.ndarray, F2: np.ndarray, match_threshold: float = 1.0, max_ratio: float = 0.6, unique: bool = False,
          swapped_back: bool = False):
    """-> (pairs [P, 2] uint32 1-based ascending in F1, metric [P] float32)"""
    F1 = np.asarray(F1, np.uint8).reshape(-1, 128)
    F2 = np.asarray(F2, np.uint8).reshape(-1, 128)
    sv = scores(F1, F2)
    ok, j, best = forward(sv, match_threshold, max_ratio)
    if unique and sv.size:
        back = np.argmin(scores(F1, F2, swapped=True) if swapped_back else sv, axis=0)
        ok = ok & (back[j] == np.arange(len(j)))
    i = np.nonzero(ok)[0]
    return np.stack([i + 1, j[i] + 1], 1).astype(np.uint32).reshape(-1, 2), best[i].astype(F32)


def index_decided_columns(F1: np.ndarray, F2: np.ndarray, match_threshold: float = 1.0, max_ratio: float = 0.6) -> int:
    """Columns that hold an accepted pair and whose minimum sv is reached by more than one F1 row."""
    sv = scores(np.asarray(F1, np.uint8), np.asarray(F2, np.uint8))
    ok, j, _ = forward(sv, match_threshold, max_ratio)
    cols = np.unique(j[ok])
    return int(((sv[:, cols] == sv[:, cols].min(axis=0)).sum(axis=0) > 1).sum()) if len(cols) else 0


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def _noisy(rows: np.ndarray, rng) -> np.ndarray:
    return np.clip(rows.astype(np.int64) + rng.integers(-3, 4, rows.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def features(n1: int, n2: int, seed: int = 7):
    """Random u8 rows; two thirds of the F1 rows are +-3-noise copies of rows of the first half of
    F2 (several F1 rows share an F2 row), and the last quarter of those copies repeats the first
    quarter exactly (column ties that the lowest F1 index decides)."""
    rng = np.random.default_rng([seed, n1, n2])
    F1 = rng.integers(0, 256, (n1, 128), dtype=np.uint8)
    F2 = rng.integers(0, 256, (n2, 128), dtype=np.uint8)
    nc = 2 * n1 // 3 if n2 // 2 else 0
    if nc:
        F1[:nc] = _noisy(F2[rng.integers(0, n2 // 2, nc)], rng)
        q = nc // 4
        F1[nc - q:nc] = F1[:q]
    F1.setflags(write=False)
    F2.setflags(write=False)
    return F1, F2


@functools.lru_cache(maxsize=None)
def reference(n1: int, n2: int, match_threshold: float = 1.0, max_ratio: float = 0.6, unique: bool = False):
    F1, F2 = features(n1, n2)
    return match(F1, F2, match_threshold, max_ratio, unique)


# Chosen on the CPU by searching seeds upward from 0 for one where the column's two best copies lie
# within an ulp of each other, so the two operand orders rank them differently (about 1 seed in
# 300 does): spec order keeps (301, 18), the swapped order (374, 18).
CROWDED_SEED = 366


@functools.lru_cache(maxsize=None)
def crowded(seed: int | None = None):
    """One F2 row with 512 near-copies among 600 F1 rows (40 F2 rows): the copies' c values crowd
    into few distinct floats, so the column's winner depends on the order of the two multiplies."""
    rng = np.random.default_rng(CROWDED_SEED if seed is None else seed)
    F2 = rng.integers(0, 256, (40, 128), dtype=np.uint8)
    F1 = rng.integers(0, 256, (600, 128), dtype=np.uint8)
    rows = rng.permutation(600)[:512]
    F1[rows] = _noisy(np.repeat(F2[17:18], 512, 0), rng)
    return F1, F2


def chunk_tie_rows():
    """n1 = 4100 (two backward chunks of 4096): F1 rows 10 and 4099 are the same noisy copy of F2
    row 5; everything else is random.  Unique keeps exactly (11, 6) (1-based)."""
    rng = np.random.default_rng(41)
    F1 = rng.integers(0, 256, (4100, 128), dtype=np.uint8)
    F2 = rng.integers(0, 256, (64, 128), dtype=np.uint8)
    F1[10] = _noisy(F2[5:6], rng)[0]
    F1[4099] = F1[10]
    return F1, F2


def chunk_tie_cols():
    """The mirror: n2 = 4100 (two forward chunks); F1 rows 3 and 40 are distinct noisy copies of F2
    row 4098 in the second chunk."""
    rng = np.random.default_rng(42)
    F1 = rng.integers(0, 256, (64, 128), dtype=np.uint8)
    F2 = rng.integers(0, 256, (4100, 128), dtype=np.uint8)
    F1[3] = _noisy(F2[4098:4099], rng)[0]
    F1[40] = _noisy(F2[4098:4099], rng)[0]
    return F1, F2


def general_features(n1: int, n2: int, seed: int = 11):
    """General single features (not u8-valued): half of the F1 rows are noisy copies of F2 rows,
    a few F1 rows repeat another F1 row exactly (column ties); noise is added to every copy, so
    no F1 row equals an F2 row (no 0 / 0 in the ratio test)."""
    rng = np.random.default_rng([seed, n1, n2])
    F1 = rng.normal(size=(n1, 128)).astype(F32)
    F2 = rng.normal(size=(n2, 128)).astype(F32)
    nc = n1 // 2
    F1[:nc] = F2[rng.integers(0, max(n2 // 2, 1), nc)] + rng.normal(scale=0.05, size=(nc, 128)).astype(F32)
    q = nc // 4
    F1[nc - q:nc] = F1[:q]
    assert not (F1[:, None, :8] == F2[None, :, :8]).all(2).any()
    return F1, F2
