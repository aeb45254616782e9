"""ctypes driver of the CPU reference of vo_refine_pose (tests/pose_refine_ref/pose_refine_ref.c:
include/vo_spec.h's vo_refine_* functions, the ones the kernel calls, around a pass that sums in the
normative order).  Test infrastructure, built on demand like tests/tri_quality_ref.py.

`refine(img, world, T, K, use=None, **params)` -> (T_out [4, 4], stats record) as Context.refine_pose.
`minimise_longdouble` is an independent evaluation written from the definitions (numpy.longdouble,
Rodrigues exponential, plain Gauss-Newton run to a fixed point), and PLANTED_* / `start_pose` /
`to_T` / `from_T` are what the CPU and GPU tests share."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import geom_ref as G

HERE = Path(__file__).resolve().parent / "pose_refine_ref"
LIB = HERE / "build" / "libpose_refine_ref.so"

CONVERGED, MAX_ITER, DAMPING, DEGENERATE, TOO_FEW = 0, 1, 2, -1, -3
STATS_DTYPE = np.dtype([("status", "<i4"), ("n_used", "<i4"), ("passes", "<i4"), ("accepted", "<i4"),
                        ("cost_initial", "<f8"), ("cost_final", "<f8")])
DEFAULTS = dict(max_iterations=20, relative_tolerance=1e-9, absolute_tolerance=0.0, lambda0=1e-3)

# the pose geom_ref.pose_problem plants (extrinsics, Xc = R X + t)
PLANTED_R = G.rodrigues([0.0, 1.0, 0.0], np.deg2rad(0.4))
PLANTED_T = np.array([0.02, -0.01, -0.95])

_lib = None


def build() -> None:
    subprocess.run(["make", "-s", "-C", str(HERE)], check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(str(LIB))
        P = C.POINTER
        L.pose_refine_ref.argtypes = [P(C.c_double), P(C.c_double), C.c_int, P(C.c_uint8), P(C.c_double), P(C.c_double), C.c_int,
                                      C.c_double, C.c_double, C.c_double, P(C.c_double), P(C.c_int32), P(C.c_double)]
        L.pose_refine_ref.restype = None
        L.pose_refine_pass.argtypes = [P(C.c_double), P(C.c_double), C.c_int, P(C.c_uint8), P(C.c_double), P(C.c_double),
                                       P(C.c_double), P(C.c_int32)]
        L.pose_refine_pass.restype = None
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _inputs(img, world, T, K, use):
    img = np.ascontiguousarray(img, np.float64).reshape(-1, 2)
    world = np.ascontiguousarray(world, np.float64).reshape(-1, 3)
    assert len(img) == len(world)
    T = np.ascontiguousarray(T, np.float64).reshape(16)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    if use is not None:
        use = np.ascontiguousarray(np.asarray(use) != 0, np.uint8).reshape(-1)
        assert len(use) == len(img)
    return img, world, T, K, use


def refine(img, world, T, K, use=None, **params):
    img, world, T, K, use = _inputs(img, world, T, K, use)
    p = dict(DEFAULTS, **params)
    out = np.zeros(16)
    stat = np.zeros(4, np.int32)
    cost = np.zeros(2)
    lib().pose_refine_ref(_p(img, C.c_double), _p(world, C.c_double), len(img), _p(use, C.c_uint8) if use is not None else None,
                          _p(K, C.c_double), _p(T, C.c_double), int(p["max_iterations"]), float(p["relative_tolerance"]),
                          float(p["absolute_tolerance"]), float(p["lambda0"]), _p(out, C.c_double), _p(stat, C.c_int32),
                          _p(cost, C.c_double))
    st = np.zeros((), STATS_DTYPE)
    st["status"], st["n_used"], st["passes"], st["accepted"] = (int(v) for v in stat)
    st["cost_initial"], st["cost_final"] = cost
    return out.reshape(4, 4), st


def sums(img, world, T, K, use=None):
    """One pass at T -> (28 sums: H's upper triangle row-major, g, cost; n_used)."""
    img, world, T, K, use = _inputs(img, world, T, K, use)
    s = np.zeros(28)
    n = np.zeros(1, np.int32)
    lib().pose_refine_pass(_p(img, C.c_double), _p(world, C.c_double), len(img), _p(use, C.c_uint8) if use is not None else None,
                           _p(K, C.c_double), _p(T, C.c_double), _p(s, C.c_double), _p(n, C.c_int32))
    return s, int(n[0])


# --------------------------------------------------------------------------- poses
def to_T(R, t) -> np.ndarray:
    """Extrinsics (Xc = R X + t) -> the camera pose in the world, rigidtform3d.A."""
    T = np.eye(4)
    T[:3, :3] = np.asarray(R).T
    T[:3, 3] = -np.asarray(R).T @ np.asarray(t)
    return T


def from_T(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    R = T[:3, :3].T
    return R, -R @ T[:3, 3]


def start_pose(rng, deg: float, dist: float, R=PLANTED_R, t=PLANTED_T) -> np.ndarray:
    """The planted pose turned by `deg` degrees about a random axis and moved by `dist` metres -> T."""
    ax = rng.normal(size=3)
    d = rng.normal(size=3)
    return to_T(G.rodrigues(ax, np.deg2rad(deg)) @ R, t + dist * d / np.linalg.norm(d))


def behind_case(seed: int):
    """40 noisy points, one of them 0.05 m in front of the planted camera, and a start 1 m behind the
    planted pose: the first step overshoots and carries that point behind the camera plane
    -> (uv, Xw, K, T0)."""
    rng = np.random.default_rng([0xF, seed])
    uv, Xw, K = G.pose_problem(rng, 40, 0.0, noise=0.2)
    Xw[0] = PLANTED_R.T @ (np.array([0.01, 0.005, 0.05]) - PLANTED_T)
    uv[0] = G.project(K, PLANTED_R, PLANTED_T, Xw[:1])[0]
    return uv, Xw, K, to_T(PLANTED_R, PLANTED_T + np.array([0.0, 0.0, 1.0]))


def far_case(seed: int = 1):
    """129 noisy points and a start 15 degrees / 4 m off: with lambda0 = 1e-9 the first, nearly
    undamped steps are rejected -> (uv, Xw, K, T0)."""
    rng = np.random.default_rng([0xE, 15, seed])
    uv, Xw, K = G.pose_problem(rng, 129, 0.0, noise=0.2)
    return uv, Xw, K, start_pose(rng, 15.0, 4.0)


SKEWED_K = np.array([[700.0, 1.5, 600.0], [0.0, 705.0, 190.0], [0.0, 0.0, 1.0]])


def pose_err_T(T, R0=PLANTED_R, t0=PLANTED_T) -> float:
    R, t = from_T(T)
    return G.pose_err(R, t, R0, t0)


# --------------------------------------------------------------------------- independent minimiser
LD = np.longdouble


def _exp_ld(w):
    th = np.sqrt(w @ w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], LD)
    if th < LD(1e-30):
        return np.eye(3, dtype=LD) + Kx
    return np.eye(3, dtype=LD) + (np.sin(th) / th) * Kx + ((1 - np.cos(th)) / (th * th)) * (Kx @ Kx)


def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in longdouble (numpy.linalg has no longdouble)."""
    A, b = A.copy(), b.copy()
    n = len(b)
    for i in range(n):
        p = i + int(np.argmax(np.abs(A[i:, i])))
        A[[i, p]], b[[i, p]] = A[[p, i]], b[[p, i]]
        for r in range(i + 1, n):
            f = A[r, i] / A[i, i]
            A[r, i:] -= f * A[i, i:]
            b[r] -= f * b[i]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


def residuals_ld(R, t, K, X, uv):
    Xc = X @ R.T + t
    xn, yn = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r = np.stack([K[0, 0] * xn + K[0, 1] * yn + K[0, 2] - uv[:, 0], K[1, 1] * yn + K[1, 2] - uv[:, 1]], 1)
    return r, Xc


def cost_ld(T, img, world, K, use=None) -> float:
    """Sum of squared pixel residuals of the used points at T, in longdouble."""
    R, t = from_T(T)
    m = np.ones(len(img), bool) if use is None else np.asarray(use, bool)
    r, _ = residuals_ld(R.astype(LD), t.astype(LD), np.asarray(K, LD).reshape(3, 3), np.asarray(world, LD)[m], np.asarray(img, LD)[m])
    return float((r * r).sum())


def minimise_longdouble(img, world, T0, K, use=None, iters: int = 60):
    """Plain Gauss-Newton on the used points from T0, in longdouble, until the step no longer moves
    the pose -> (R, t float64, cost float).  The step is the left perturbation exp(w) applied to
    (R, t); the Jacobian is written from the chain rule d(pixel)/d(Xc) * d(Xc)/d(w, v), with
    d(Xc)/dw = -[Xc]x."""
    R, t = (a.astype(LD) for a in from_T(T0))
    K = np.asarray(K, LD).reshape(3, 3)
    m = np.ones(len(img), bool) if use is None else np.asarray(use, bool)
    X, uv = np.asarray(world, LD).reshape(-1, 3)[m], np.asarray(img, LD).reshape(-1, 2)[m]
    for _ in range(iters):
        r, Xc = residuals_ld(R, t, K, X, uv)
        z = Xc[:, 2]
        n = len(X)
        dp = np.zeros((n, 2, 3), LD)                      # d(pixel) / d(Xc)
        dp[:, 0, 0] = K[0, 0] / z
        dp[:, 0, 1] = K[0, 1] / z
        dp[:, 0, 2] = -(K[0, 0] * Xc[:, 0] + K[0, 1] * Xc[:, 1]) / (z * z)
        dp[:, 1, 1] = K[1, 1] / z
        dp[:, 1, 2] = -K[1, 1] * Xc[:, 1] / (z * z)
        sk = np.zeros((n, 3, 3), LD)                      # -[Xc]x
        sk[:, 0, 1], sk[:, 0, 2] = Xc[:, 2], -Xc[:, 1]
        sk[:, 1, 0], sk[:, 1, 2] = -Xc[:, 2], Xc[:, 0]
        sk[:, 2, 0], sk[:, 2, 1] = Xc[:, 1], -Xc[:, 0]
        J = np.concatenate([np.einsum("nij,njk->nik", dp, sk), dp], 2).reshape(2 * n, 6)
        d = _solve_ld(J.T @ J, -(J.T @ r.reshape(-1)))
        dR = _exp_ld(d[:3])
        R, t = dR @ R, dR @ t + d[3:]
        if np.abs(d).max() < LD(1e-18):
            break
    r, _ = residuals_ld(R, t, K, X, uv)
    return R.astype(np.float64), t.astype(np.float64), float((r * r).sum())
