"""ctypes driver of the CPU reference of vo_est_fundamental (tests/fund_ref/fund_ref.c: include/vo_spec.h's
vo_fund_* functions, the ones the kernel calls, around the normative loops).  Test infrastructure,
built on demand like tests/pose_refine_ref.py.

`estimate(x1, x2, ...)` -> record as Context.est_fundamental plus the best slot's own F and the census.
`case(...)` is the generator the CPU and GPU suites share (KITTI-00 K, a general and a rectified-stereo
motion, given noise and outlier fraction, points rounded to single), `table()` the census table both
replay, and `norm8_svd` / `sampson_ld` an independent evaluation written from the definitions
(numpy.linalg.svd for both decompositions, longdouble for the sums)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "fund_ref"
LIB = HERE / "build" / "libfund_ref.so"

OK, TOO_FEW, NO_CONSENSUS = 0, -3, -4
NORM8, MSAC = 0, 1
NO_BOUND = 0x7FFFFFFF
DEFAULTS = dict(method=MSAC, num_trials=500, distance_threshold=0.01, confidence=99.0, seed=0x5EED)
CENSUS = ("trials", "bound", "best", "slots", "reattempt", "no_sample", "no_model", "nan_dist", "no_bound", "sweeps9", "sweeps3",
          "improved", "ties", "refit_model")

_lib = None


def build() -> None:
    subprocess.run(["make", "-s", "-C", str(HERE)], check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(str(LIB))
        P = C.POINTER
        L.fund_ref.argtypes = [P(C.c_float), P(C.c_float), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                               P(C.c_double), P(C.c_uint8), P(C.c_int32), P(C.c_double), P(C.c_int32)]
        L.fund_ref_norm8.argtypes = [P(C.c_float), P(C.c_float), C.c_int, P(C.c_uint8), P(C.c_double), P(C.c_int32)]
        L.fund_ref_sample_fit.argtypes = [P(C.c_float), P(C.c_float), P(C.c_uint32), P(C.c_double), P(C.c_int32)]
        L.fund_ref_sampson.argtypes = [P(C.c_double), P(C.c_float), P(C.c_float), C.c_int, P(C.c_double)]
        L.fund_ref_sampson.restype = None
        L.fund_ref_sample.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint32), P(C.c_int32)]
        L.fund_ref_trials_needed.argtypes = [C.c_int, C.c_int, C.c_double]
        L.fund_ref_jacobi.argtypes = [P(C.c_double), P(C.c_double), C.c_int, P(C.c_int32)]
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _pts(x):
    return np.ascontiguousarray(x, np.float32).reshape(-1, 2)


def estimate(x1, x2, key: int = 0, **params) -> dict:
    """-> dict(status, F [3, 3], inliers [n] bool, n_inliers, best_F [3, 3], census dict)."""
    x1, x2 = _pts(x1), _pts(x2)
    assert len(x1) == len(x2)
    p = dict(DEFAULTS, **params)
    n = len(x1)
    F, Fb = np.zeros(9), np.zeros(9)
    mask = np.zeros(max(n, 1), np.uint8)
    nin = np.zeros(1, np.int32)
    cen = np.zeros(len(CENSUS), np.int32)
    st = lib().fund_ref(_p(x1, C.c_float), _p(x2, C.c_float), n, int(p["method"]), int(p["num_trials"]),
                        float(p["distance_threshold"]), float(p["confidence"]), int(p["seed"]), int(key) & 0xFFFFFFFF,
                        _p(F, C.c_double), _p(mask, C.c_uint8), _p(nin, C.c_int32), _p(Fb, C.c_double), _p(cen, C.c_int32))
    return dict(status=int(st), F=F.reshape(3, 3), inliers=mask[:n].astype(bool), n_inliers=int(nin[0]), best_F=Fb.reshape(3, 3),
                census=dict(zip(CENSUS, (int(v) for v in cen))))


def norm8(x1, x2, mask=None):
    """The masked fit -> (ok, F [3, 3], (sweeps at 9x9, sweeps at 3x3))."""
    x1, x2 = _pts(x1), _pts(x2)
    F = np.zeros(9)
    sw = np.zeros(2, np.int32)
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    ok = lib().fund_ref_norm8(_p(x1, C.c_float), _p(x2, C.c_float), len(x1), _p(m, C.c_uint8) if m is not None else None,
                              _p(F, C.c_double), _p(sw, C.c_int32))
    return bool(ok), F.reshape(3, 3), (int(sw[0]), int(sw[1]))


def sample_fit(x1, x2, idx):
    """A sample's sequential fit over the 8 rows idx -> (ok, F, sweeps)."""
    x1, x2 = _pts(x1), _pts(x2)
    idx = np.ascontiguousarray(idx, np.uint32)
    assert idx.shape == (8,)
    F = np.zeros(9)
    sw = np.zeros(2, np.int32)
    ok = lib().fund_ref_sample_fit(_p(x1, C.c_float), _p(x2, C.c_float), _p(idx, C.c_uint32), _p(F, C.c_double), _p(sw, C.c_int32))
    return bool(ok), F.reshape(3, 3), (int(sw[0]), int(sw[1]))


def sampson(F, x1, x2) -> np.ndarray:
    x1, x2 = _pts(x1), _pts(x2)
    F = np.ascontiguousarray(F, np.float64).reshape(9)
    d = np.zeros(len(x1))
    lib().fund_ref_sampson(_p(F, C.c_double), _p(x1, C.c_float), _p(x2, C.c_float), len(x1), _p(d, C.c_double))
    return d


def sample(seed: int, key: int, slot: int, n: int):
    idx = np.zeros(8, np.uint32)
    att = np.zeros(1, np.int32)
    ok = lib().fund_ref_sample(seed, key, slot, n, _p(idx, C.c_uint32), _p(att, C.c_int32))
    return bool(ok), idx, int(att[0])


def trials_needed(n_in: int, n: int, conf: float) -> int:
    return int(lib().fund_ref_trials_needed(n_in, n, conf))


def jacobi(A: np.ndarray):
    """Symmetric A [n, n] -> (eigenvalues on the diagonal, V, index of the smallest, sweeps)."""
    A = np.asarray(A, np.float64)
    n = len(A)
    tri = np.ascontiguousarray(A[np.triu_indices(n)])
    V = np.zeros(n * n)
    sw = np.zeros(1, np.int32)
    j = lib().fund_ref_jacobi(_p(tri, C.c_double), _p(V, C.c_double), n, _p(sw, C.c_int32))
    full = np.zeros((n, n))
    full[np.triu_indices(n)] = tri
    return np.diag(full).copy(), V.reshape(n, n), int(j), int(sw[0])


# --------------------------------------------------------------------------- generator
K00 = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])
ROWS, COLS = 375, 1242


def _rodrigues(axis, ang):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)


MOTIONS = {
    # camera 2: Xc2 = R Xc1 + t
    "general": (_rodrigues([0.2, 1.0, 0.1], np.deg2rad(2.0)), np.array([0.15, -0.05, -0.9])),
    "stereo": (np.eye(3), np.array([-0.537, 0.0, 0.0])),
}


def true_F(motion: str) -> np.ndarray:
    """F of the motion for 1-based pixels, unit Frobenius norm, F[2, 2] >= 0."""
    R, t = MOTIONS[motion]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K00)
    S = np.array([[1.0, 0, -1.0], [0, 1.0, -1.0], [0, 0, 1.0]])      # 1-based -> 0-based pixels
    F = S.T @ Ki.T @ tx @ R @ Ki @ S
    F = F / np.linalg.norm(F)
    return -F if F[2, 2] < 0 else F


def case(n: int, motion: str = "general", noise: float = 0.1, outliers: float = 0.0, seed: int = 0):
    """n correspondences of points 4 .. 40 m in front of camera 1, seen by both cameras inside the
    KITTI frame; Gaussian pixel noise; the first round(outliers * n) rows of a fixed permutation get a
    uniformly random second point.  1-based pixels rounded to single -> (x1, x2 [n, 2] float32,
    is_outlier [n] bool)."""
    rng = np.random.default_rng([0xF0D, n, int(noise * 1000), int(outliers * 1000), seed, sorted(MOTIONS).index(motion)])
    R, t = MOTIONS[motion]
    x1 = np.zeros((n, 2))
    x2 = np.zeros((n, 2))
    k = 0
    while k < n:
        u = rng.uniform([20, 20], [COLS - 20, ROWS - 20])
        z = rng.uniform(4.0, 40.0)
        X = z * (np.linalg.inv(K00) @ np.array([u[0], u[1], 1.0]))
        Y = R @ X + t
        if Y[2] < 1.0:
            continue
        v = (K00 @ Y)[:2] / Y[2]
        if not (0 <= v[0] < COLS and 0 <= v[1] < ROWS):
            continue
        x1[k], x2[k] = u, v
        k += 1
    x1 += rng.normal(scale=noise, size=x1.shape) if noise else 0.0
    x2 += rng.normal(scale=noise, size=x2.shape) if noise else 0.0
    bad = np.zeros(n, bool)
    m = int(round(outliers * n))
    if m:
        rows = rng.permutation(n)[:m]
        bad[rows] = True
        x2[rows] = rng.uniform([0, 0], [COLS, ROWS], size=(m, 2))
    return (x1 + 1.0).astype(np.float32), (x2 + 1.0).astype(np.float32), bad


def coincident_case(n: int = 40, seed: int = 3):
    """A general-motion case whose first n // 2 rows are one and the same correspondence: most samples
    hold coincident points (a rank-deficient design matrix), some hold nothing else."""
    x1, x2, _ = case(n, "general", 0.1, 0.0, seed)
    x1[: n // 2] = x1[0]
    x2[: n // 2] = x2[0]
    return x1, x2


def all_same_case(n: int = 12):
    """Every row the same correspondence: no scale, so no sample and no fit has a model."""
    x1 = np.tile(np.float32([100.5, 50.25]), (n, 1))
    x2 = np.tile(np.float32([90.0, 50.5]), (n, 1))
    return x1, x2


def _mixed(n: int, n_good: int, seed: int):
    """n rows of which exactly the first n_good fit the general motion without noise; the rest are
    far off (random second points)."""
    x1, x2, _ = case(n, "general", 0.0, 0.0, seed)
    rng = np.random.default_rng([0xBAD, n, n_good, seed])
    x2[n_good:] = rng.uniform([1, 1], [COLS, ROWS], size=(n - n_good, 2)).astype(np.float32)
    return x1, x2


# The census table both suites replay: (name, x1, x2, params, key).  n covers 0, 7, 8, 9, 63, 64, 65, 129,
# 300; num_trials 1, 10, 64, 65, 500 (the chunk edges); both methods.
def table():
    T = []

    def add(name, x1, x2, key=0, **params):
        T.append((name, x1, x2, dict(DEFAULTS, **params), key))

    e = np.zeros((0, 2), np.float32)
    add("n0", e, e)
    add("n0_norm8", e, e, method=NORM8)
    for n in (7, 8, 9, 63, 64, 65, 129, 300):
        x1, x2, _ = case(n, "general" if n % 2 else "stereo", 0.1, 0.0, n)
        add(f"norm8_n{n}", x1, x2, method=NORM8)
        if n in (8, 9):         # with noise the rank-2 fit of 8 points leaves some of them outside the threshold:
            add(f"msac_n{n}_noisy", x1, x2, key=n, distance_threshold=0.1)      # no consensus, equal-sample slots tie
            x1, x2, _ = case(n, "general" if n % 2 else "stereo", 0.0, 0.0, n)
        add(f"msac_n{n}", x1, x2, key=n, distance_threshold=0.1)
    # n = 8, general motion, 0.5 px noise, tight threshold: the rank-2 fit leaves points outside, so the loop goes on
    # over the ~4 % of slots that are valid -- all of them the same 8 rows in another order: equal or nearly equal scores
    x1, x2, _ = case(8, "general", 0.5, 0.0, 88)
    add("msac_n8_tie", x1, x2, key=5, distance_threshold=1e-4, num_trials=500)
    for nt in (1, 10, 64, 65, 500):
        for out in (0.0, 0.3, 0.6):
            x1, x2, _ = case(300, "general", 0.1, out, nt)
            add(f"msac_n300_t{nt}_o{int(out * 100)}", x1, x2, key=nt, num_trials=nt, distance_threshold=0.1)
    for out in (0.2, 0.4, 0.5):
        x1, x2, _ = case(40, "stereo", 0.1, out, 7)
        add(f"msac_n40_o{int(out * 100)}", x1, x2, key=40, distance_threshold=0.1)
    for n_good in (63, 64, 65):                                   # the refit with and without a final partial
        x1, x2 = _mixed(129, n_good, n_good)
        add(f"refit_{n_good}", x1, x2, key=n_good, distance_threshold=0.01, num_trials=2000)
    x1, x2 = coincident_case()
    add("coincident", x1, x2, key=1, distance_threshold=0.1, num_trials=200)
    x1, x2 = all_same_case()
    add("all_same", x1, x2, key=2)
    add("all_same_norm8", x1, x2, method=NORM8)
    x1, x2 = _mixed(300, 2, 9)                                     # two consistent rows of 300: w < 0.01, no bound
    add("no_bound", x1, x2, key=3, distance_threshold=1e-6, num_trials=65)
    x1, x2 = _mixed(40, 6, 11)                                     # fewer than 8 inliers whatever is sampled
    add("few_inliers", x1, x2, key=4, distance_threshold=1e-9, num_trials=64)
    return T


# --------------------------------------------------------------------------- independent evaluation
LD = np.longdouble


def _normalise_ld(x):
    c = x.mean(0)
    d = np.sqrt(((x - c) ** 2).sum(1)).mean()
    s = np.sqrt(LD(2)) / d
    T = np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]], LD)
    return (x - c) * s, T


def norm8_svd(x1, x2, mask=None) -> np.ndarray:
    """The normalised 8-point algorithm from its textbook definition: longdouble normalisation and
    design matrix, numpy.linalg.svd for the null vector of A and for the rank-2 projection."""
    x1, x2 = np.asarray(x1, LD).reshape(-1, 2), np.asarray(x2, LD).reshape(-1, 2)
    if mask is not None:
        x1, x2 = x1[np.asarray(mask, bool)], x2[np.asarray(mask, bool)]
    a, T1 = _normalise_ld(x1)
    b, T2 = _normalise_ld(x2)
    A = np.stack([b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0], b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1], a[:, 0], a[:, 1],
                  np.ones(len(a), LD)], 1)
    M = (A.T @ A).astype(np.float64)                                  # the sums in longdouble, the decomposition in double
    _, _, Vt = np.linalg.svd(M)
    Fh = Vt[-1].reshape(3, 3)
    U, S, Vt3 = np.linalg.svd(Fh)
    Fr = (U * np.array([S[0], S[1], 0.0])) @ Vt3
    F = (T2.T @ Fr.astype(LD) @ T1).astype(np.float64)
    F = F / np.linalg.norm(F)
    return -F if F[2, 2] < 0 else F


def sampson_ld(F, x1, x2) -> np.ndarray:
    F = np.asarray(F, LD).reshape(3, 3)
    h1 = np.concatenate([np.asarray(x1, LD).reshape(-1, 2), np.ones((len(x1), 1), LD)], 1)
    h2 = np.concatenate([np.asarray(x2, LD).reshape(-1, 2), np.ones((len(x2), 1), LD)], 1)
    l = h1 @ F.T
    m = h2 @ F
    r = (h2 * l).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (r * r / (l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2)).astype(np.float64)
