"""numpy restatement of matchFeaturesInRadius ("In radius"; include/vo.h:
vo_match_radius), the ctypes driver of the CPU build of its two spec functions
(tests/match_radius_ref/: include/vo_spec.h's vo_radius_gate / vo_radius_box_lb, the text the
kernel compiles), and the input generators with their census (tests/test_match_radius.py asserts
it on the reference alone, so tests/test_gpu_match_radius.py cannot pass vacuously).

Scores are match_ref.scores' sv(i, j).  Candidates of row i: C_i = {j : d2(i, j) <= r2_i},
dx = x2_j - cx_i, dy = y2_j - cy_i, d2 = dx * dx + dy * dy, r2_i = r_i * r_i in float32, one rounding
per operation.  Outside C_i the score is +inf; the forward step, the thresholds and Unique are then
match_ref's own on the gated matrix: no candidate -> best = +inf fails the threshold; one
candidate -> second = +inf, ratio 0; back(j) = argmin_i of the gated column.
"""
from __future__ import annotations

import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

import match_ref as mr

F32 = np.float32
HERE = Path(__file__).resolve().parent / "match_radius_ref"
LIB = HERE / "build" / "libmatch_radius_ref.so"

SHAPES = [(33, 129), (129, 33), (300, 257), (4100, 200), (200, 4100), (2100, 2100)]
LAYOUTS = ["scalar", "perrow", "sorted"]
WIDTH, HEIGHT = 1242, 375

_lib = None


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def _radius_rows(radius, n1: int) -> np.ndarray:
    r = np.asarray(radius, F32).reshape(-1)
    assert r.size in (1, n1)
    return np.broadcast_to(r, (n1,)) if r.size == 1 else r


def gate(points2, centers, radius) -> np.ndarray:
    """-> bool [n1, n2]: column j is a candidate of row i."""
    p2 = np.asarray(points2, F32).reshape(-1, 2)
    c = np.asarray(centers, F32).reshape(-1, 2)
    r = _radius_rows(radius, len(c))
    with np.errstate(over="ignore"):
        dx = p2[None, :, 0] - c[:, None, 0]
        dy = p2[None, :, 1] - c[:, None, 1]
        d2 = dx * dx + dy * dy
        r2 = r * r
    assert d2.dtype == F32 and r2.dtype == F32
    return d2 <= r2[:, None]


def box_lb(boxes, points) -> np.ndarray:
    """vo_radius_box_lb: boxes [nb, 4] = (xmin, xmax, ymin, ymax), points [n, 2] -> lb float32 [n, nb]."""
    b = np.asarray(boxes, F32).reshape(-1, 4)
    p = np.asarray(points, F32).reshape(-1, 2)
    zero = F32(0.0)
    with np.errstate(over="ignore"):
        bx = np.maximum(np.maximum(b[None, :, 0] - p[:, None, 0], p[:, None, 0] - b[None, :, 1]), zero)
        by = np.maximum(np.maximum(b[None, :, 2] - p[:, None, 1], p[:, None, 1] - b[None, :, 3]), zero)
        lb = bx * bx + by * by
    assert lb.dtype == F32
    return lb


def tile_boxes(points) -> np.ndarray:
    """Bounding boxes [ceil(n / 32), 4] = (xmin, xmax, ymin, ymax) of the aligned 32-row tiles."""
    p = np.asarray(points, F32).reshape(-1, 2)
    out = [(t[:, 0].min(), t[:, 0].max(), t[:, 1].min(), t[:, 1].max()) for t in (p[k:k + 32] for k in range(0, len(p), 32))]
    return np.array(out, F32).reshape(-1, 4)


def gated_scores(F1, F2, points2, centers, radius) -> np.ndarray:
    sv = mr.scores(np.asarray(F1, np.uint8).reshape(-1, 128), np.asarray(F2, np.uint8).reshape(-1, 128))
    return np.where(gate(points2, centers, radius), sv, F32(np.inf)).astype(F32)


def match_gated(g: np.ndarray, match_threshold: float = 1.0, max_ratio: float = 0.6, unique: bool = False):
    """match_ref's forward step and Unique on a gated score matrix -> (pairs, metric)."""
    ok, j, best = mr.forward(g, match_threshold, max_ratio)
    if unique and g.size:
        ok = ok & (np.argmin(g, axis=0)[j] == np.arange(len(j)))
    i = np.nonzero(ok)[0]
    return np.stack([i + 1, j[i] + 1], 1).astype(np.uint32).reshape(-1, 2), best[i].astype(F32)


def match(F1, F2, points2, centers, radius, match_threshold: float = 1.0, max_ratio: float = 0.6, unique: bool = False):
    """-> (pairs [P, 2] uint32 1-based ascending in F1, metric [P] float32)"""
    return match_gated(gated_scores(F1, F2, points2, centers, radius), match_threshold, max_ratio, unique)


# ---------------------------------------------------------------------------
# the CPU build of the spec functions
# ---------------------------------------------------------------------------
def build() -> None:
    subprocess.run(["make", "-s", "-C", str(HERE)], check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(str(LIB))
        P = C.POINTER
        L.radius_gate_ref.argtypes = [P(C.c_float), C.c_int, P(C.c_float), C.c_int, P(C.c_float), C.c_int, P(C.c_uint8)]
        L.radius_gate_ref.restype = None
        L.radius_box_ref.argtypes = [P(C.c_float), C.c_int, P(C.c_float), C.c_int, P(C.c_float)]
        L.radius_box_ref.restype = None
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def gate_c(points2, centers, radius) -> np.ndarray:
    p2 = np.ascontiguousarray(points2, F32).reshape(-1, 2)
    c = np.ascontiguousarray(centers, F32).reshape(-1, 2)
    r = np.ascontiguousarray(radius, F32).reshape(-1)
    out = np.zeros((len(c), len(p2)), np.uint8)
    lib().radius_gate_ref(_p(p2, C.c_float), len(p2), _p(c, C.c_float), len(c), _p(r, C.c_float), len(r), _p(out, C.c_uint8))
    return out.astype(bool)


def box_lb_c(boxes, points) -> np.ndarray:
    b = np.ascontiguousarray(boxes, F32).reshape(-1, 4)
    p = np.ascontiguousarray(points, F32).reshape(-1, 2)
    out = np.zeros((len(p), len(b)), F32)
    lib().radius_box_ref(_p(b, C.c_float), len(b), _p(p, C.c_float), len(p), _p(out, C.c_float))
    return out


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
# seeds chosen on the CPU, searching upward from 0 for the first at which the case's census holds
SEEDS: dict = {(33, 129, "scalar"): 2, (33, 129, "sorted"): 1, (200, 4100, "scalar"): 2, (200, 4100, "sorted"): 1}   # others: 0


@functools.lru_cache(maxsize=None)
def case(n1: int, n2: int, layout: str, seed: int | None = None):
    """-> (F1, F2, points2, centers, radius): coordinates on a quarter-pixel grid in 1242 x 375.
    Two thirds of the F1 rows are +-3-noise copies of F2 rows of F2's first half; a copy's centre is
    its source's point plus s k (+-3, +-4) or s k (+-4, +-3), k in 1..4, its radius 5 k (layout
    "scalar": k = 4, one radius 20), s in {0.5, 1, 1.25}: inside, exactly on the circle
    (d2 = 25 k^2 = r2 in float32) and outside.  A quarter of the copies get a decoy in F2's upper
    half, 200.25 px from the source: a second near-copy of the source, or (every other one) an exact
    copy of the F1 row itself -- the row's best descriptor in all of F2, outside its circle.
    With n2 >= 64 the points of F2 rows 0..31 (one tile of the unsorted layouts) cluster in a 32 px
    square, so that the row blocks far from it skip that tile.
    "sorted": F2 and points2 reordered by (y, x), the order SIFT emits within a layer."""
    assert layout in LAYOUTS
    rng = np.random.default_rng([SEEDS.get((n1, n2, layout), 0) if seed is None else seed, n1, n2, LAYOUTS.index(layout)])
    F1 = rng.integers(0, 256, (n1, 128), dtype=np.uint8)
    F2 = rng.integers(0, 256, (n2, 128), dtype=np.uint8)
    grid = lambda n: np.stack([rng.integers(0, 4 * WIDTH, n), rng.integers(0, 4 * HEIGHT, n)], 1).astype(F32) * F32(0.25)
    P2, Cn = grid(n2), grid(n1)
    if n2 >= 64:                                           # a tile the row blocks without a centre near it skip
        P2[:32] = grid(1) * F32(0.9) // F32(0.25) * F32(0.25) + rng.integers(0, 128, (32, 2)).astype(F32) * F32(0.25)
    k = rng.integers(1, 5, n1) if layout != "scalar" else np.full(n1, 4)
    nc = 2 * n1 // 3 if n2 // 2 else 0
    if nc:
        src = rng.integers(0, n2 // 2, nc)
        F1[:nc] = mr._noisy(F2[src], rng)
        s = np.array([0.5, 1.0, 1.25])[rng.integers(0, 3, nc)]
        leg = np.where(rng.integers(0, 2, nc)[:, None] == 0, [[3.0, 4.0]], [[4.0, 3.0]]) * rng.choice([-1.0, 1.0], (nc, 2))
        Cn[:nc] = (P2[src].astype(np.float64) + (s * k[:nc])[:, None] * leg).astype(F32)
        nd = min(nc // 4, (n2 - n2 // 2) // 2)
        rows = rng.permutation(nc)[:nd]
        cols = n2 // 2 + rng.permutation(n2 - n2 // 2)[:nd]
        F2[cols] = mr._noisy(F2[src[rows]], rng)
        F2[cols[::2]] = F1[rows[::2]]
        side = np.where(P2[src[rows], 0] < WIDTH / 2, 200.25, -200.25)
        P2[cols] = P2[src[rows]] + np.stack([side, np.zeros(nd)], 1).astype(F32)
    radius = np.array([20.0], F32) if layout == "scalar" else (5 * k).astype(F32)
    if layout == "sorted":
        order = np.lexsort((P2[:, 0], P2[:, 1]))
        F2, P2 = F2[order], P2[order]
    for a in (F1, F2, P2, Cn, radius):
        a.setflags(write=False)
    return F1, F2, P2, Cn, radius


@functools.lru_cache(maxsize=8)
def gated(n1: int, n2: int, layout: str, seed: int | None = None) -> np.ndarray:
    g = gated_scores(*case(n1, n2, layout, seed))
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def reference(n1: int, n2: int, layout: str, match_threshold: float = 1.0, max_ratio: float = 0.6, unique: bool = False):
    return match_gated(gated(n1, n2, layout), match_threshold, max_ratio, unique)


def prereject(points2, centers, radius) -> np.ndarray:
    """bool [ceil(n1 / 32), ceil(n2 / 32)]: the forward pass skips (32-row block, tile): no row of
    the block has box_lb(tile's box, its centre) <= its r2."""
    c = np.asarray(centers, F32).reshape(-1, 2)
    r = _radius_rows(radius, len(c))
    with np.errstate(over="ignore"):
        may = box_lb(tile_boxes(points2), c) <= (r * r)[:, None]
    return np.array([~may[b:b + 32].any(0) for b in range(0, len(c), 32)]).reshape(-1, may.shape[1])


def census_required(n1: int, n2: int, layout: str) -> list:
    """The classes a case of this size must contain (each count >= 1).  0 / 1 / 2 / >= 3 candidates
    need a point density that the four larger shapes have; a pair that plain matchFeatures rejects
    needs a near-copy decoy whose row is inside its circle, which the 5 decoys of (33, 129) do not
    reliably give; the pre-reject needs two column tiles."""
    need = ["on_circle", "single", "unique_removed", "best_outside"]
    if n1 * n2 >= 300 * 257:
        need += ["cand0", "cand1", "cand2", "cand3"]
    if (n1, n2) != (33, 129):
        need.append("not_plain")
    if layout == "sorted":
        need.append("empty_fraction")
    if n2 >= 64:
        need += ["pre_skipped", "pre_kept"]
    return need


def census(n1: int, n2: int, layout: str, seed: int | None = None) -> dict:
    """Counts of the classes the generator is built to contain, at the default options."""
    F1, F2, P2, Cn, radius = case(n1, n2, layout, seed)
    g = gated(n1, n2, layout, seed) if seed is None else gated_scores(F1, F2, P2, Cn, radius)
    inside = np.isfinite(g)
    ncand = inside.sum(1)
    pairs, _ = match_gated(g)
    pu, _ = match_gated(g, unique=True)
    i, j = pairs[:, 0].astype(np.int64) - 1, pairs[:, 1].astype(np.int64) - 1
    r = _radius_rows(radius, n1)
    d2 = ((P2[j, 0] - Cn[i, 0]) ** 2 + (P2[j, 1] - Cn[i, 1]) ** 2).astype(F32)
    plain = {tuple(p) for p in mr.match(F1, F2)[0].tolist()}
    sv = mr.scores(F1, F2)
    gbest = np.argmin(sv, axis=1)
    empty = np.array([[not inside[a:a + 32, b:b + 32].any() for b in range(0, n2, 32)] for a in range(0, n1, 32)])
    pre = prereject(P2, Cn, radius)
    assert not (pre & ~empty).any(), "the pre-reject skipped a tile that holds a candidate"
    return {
        "cand0": int((ncand == 0).sum()), "cand1": int((ncand == 1).sum()), "cand2": int((ncand == 2).sum()),
        "cand3": int((ncand >= 3).sum()),
        "on_circle": int((d2 == (r * r)[i]).sum()),
        "single": int((ncand[i] == 1).sum()),
        "not_plain": sum(tuple(p) not in plain for p in pairs.tolist()),
        "unique_removed": len(pairs) - len(pu),
        "best_outside": int(((gbest[i] != j) & ~inside[i, gbest[i]] & (sv[i, gbest[i]] < sv[i, j])).sum()),
        "empty_fraction": float(empty.mean()),
        "pre_skipped": int(pre.sum()), "pre_kept": int((~pre).sum()),
        "pairs": len(pairs),
    }
