"""float64 numpy references of the geometry stages, written from the
definitions, and the input generators shared by test_geometry_ref.py (CPU: the oracle against
these references) and test_gpu_geometry_edges.py (GPU: libvo.so against the oracle).

tri_svd        linear DLT triangulation: numpy.linalg.svd of the 4x4 system.
p3p_roots      Grunert's P3P: the quartic's closed-form coefficients (Haralick, Lee, Ottenberg,
               Noelle 1994, eq. 9), numpy.roots, Kabsch/SVD alignment.
msac_replay    estworldpose: the Philox sampler restated in Python, the oracle's P3P per slot,
               scores / inlier counts / adaptive termination / mask in numpy float64.
landmarks_np   VO.m:145-160 + CreateLandmarksFromFeatures.m on top of a triangulation.

Nothing here calls into libvo.so; `oracle` is passed in where a function needs the oracle's
Philox, P3P or triangulation.
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
KITTI_K = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])
KITTI_P1 = np.c_[KITTI_K, np.zeros(3)]
KITTI_P2 = np.c_[KITTI_K, [-386.1448, 0.0, 0.0]]


# --------------------------------------------------------------------------- rotations
def rodrigues(axis, angle: float) -> np.ndarray:
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx


def project(K, R, t, Xw) -> np.ndarray:
    """Pixels of world points under x = K (R X + t) (K upper triangular, skew allowed)."""
    Xc = np.asarray(Xw) @ np.asarray(R).T + t
    xn, yn = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    return np.stack([K[0, 0] * xn + K[0, 1] * yn + K[0, 2], K[1, 1] * yn + K[1, 2]], 1)


# --------------------------------------------------------------------------- triangulate
def tri_svd(x1, x2, P1, P2):
    """-> (X [n, 3], wn [n]): the null vector v of the DLT system by numpy's SVD, X = v[:3] / v[3],
    wn = |v[3]| / |v| (small: the point is near infinity and X is ill-determined).  The inputs
    are taken as given (single pixel positions are exact in float64)."""
    x1 = np.asarray(x1, np.float64).reshape(-1, 2)
    x2 = np.asarray(x2, np.float64).reshape(-1, 2)
    P1, P2 = np.asarray(P1, np.float64).reshape(3, 4), np.asarray(P2, np.float64).reshape(3, 4)
    n = x1.shape[0]
    A = np.empty((n, 4, 4))
    A[:, 0] = x1[:, :1] * P1[2] - P1[0]
    A[:, 1] = x1[:, 1:] * P1[2] - P1[1]
    A[:, 2] = x2[:, :1] * P2[2] - P2[0]
    A[:, 3] = x2[:, 1:] * P2[2] - P2[1]
    if n == 0:
        return np.zeros((0, 3)), np.zeros(0)
    v = np.linalg.svd(A)[2][:, 3, :]
    return v[:, :3] / v[:, 3:], np.abs(v[:, 3]) / np.linalg.norm(v, axis=1)


def tri_ulp_ratio(got, ref) -> np.ndarray:
    """Per row: max |got - ref| in units of the single-precision half-ulp bound of the row's
    largest reference coordinate, 2^-24 max|ref row|."""
    return np.abs(got - ref).max(1) / (2.0 ** -24 * np.abs(ref).max(1))


def tri_fixtures():
    """name -> (x1, x2, P1, P2) single pixel positions: (a) 2000 KITTI-calibrated points, disparity
    0.5 .. 120 px (depth 3 .. 770 m), 0.3 px row noise; (b) the 1-based pixel offset of the MATLAB
    path (projections + 1); (c) a general second camera: rotated 0.2 rad about a skew axis, baseline
    with all three components -- not rectified."""
    rng = np.random.default_rng(0x7121)
    out = {}
    n = 2000
    u = rng.uniform(130, 1240, n)
    v = rng.uniform(0, 375, n)
    d = np.exp(rng.uniform(np.log(0.5), np.log(120.0), n))
    x1 = np.stack([u, v], 1).astype(F32)
    x2 = np.stack([u - d, v + rng.normal(0, 0.3, n)], 1).astype(F32)
    out["kitti_low_disparity"] = (x1, x2, KITTI_P1, KITTI_P2)
    m = 500
    X = np.stack([rng.uniform(-20, 20, m), rng.uniform(-3, 3, m), rng.uniform(4, 90, m)], 1)
    I3, z3 = np.eye(3), np.zeros(3)
    tb = np.linalg.solve(KITTI_K, KITTI_P2[:, 3])
    out["one_based"] = ((project(KITTI_K, I3, z3, X) + 1.0).astype(F32), (project(KITTI_K, I3, tb, X) + 1.0).astype(F32),
                        KITTI_P1, KITTI_P2)
    R2 = rodrigues([0.3, 1.0, -0.2], 0.2)
    t2 = np.array([-0.6, 0.05, 0.1])
    K2 = np.array([[700.0, 1.5, 600.0], [0.0, 705.0, 190.0], [0.0, 0.0, 1.0]])
    P2g = K2 @ np.c_[R2, t2]
    out["general_P2"] = (project(KITTI_K, I3, z3, X).astype(F32), project(K2, R2, t2, X).astype(F32), KITTI_P1, P2g)
    return out


# --------------------------------------------------------------------------- P3P
def grunert_quartic(img3, world3, K):
    """-> (A [5] ascending coefficients of Grunert's quartic in v = s3 / s1, aux).  Closed form of
    Haralick et al. 1994 eq. 9, with a, b, c the sides opposite world points 1, 2, 3 and alpha,
    beta, gamma the angles between the bearing pairs (2,3), (1,3), (1,2)."""
    img3 = np.asarray(img3, np.float64).reshape(3, 2)
    w = np.asarray(world3, np.float64).reshape(3, 3)
    K = np.asarray(K, np.float64).reshape(3, 3)
    j = np.linalg.solve(K, np.c_[img3, np.ones(3)].T).T
    j = j / np.linalg.norm(j, axis=1, keepdims=True)
    a2 = float(np.sum((w[1] - w[2]) ** 2))
    b2 = float(np.sum((w[0] - w[2]) ** 2))
    c2 = float(np.sum((w[0] - w[1]) ** 2))
    ca, cb, cg = float(j[1] @ j[2]), float(j[0] @ j[2]), float(j[0] @ j[1])
    if not (a2 > 0 and b2 > 0 and c2 > 0):
        return None, None
    q = (a2 - c2) / b2                 # (a^2 - c^2) / b^2
    p = (a2 + c2) / b2
    A4 = (q - 1.0) ** 2 - 4.0 * c2 / b2 * ca * ca
    A3 = 4.0 * (q * (1.0 - q) * cb - (1.0 - p) * ca * cg + 2.0 * c2 / b2 * ca * ca * cb)
    A2 = 2.0 * (q * q - 1.0 + 2.0 * q * q * cb * cb + 2.0 * (b2 - c2) / b2 * ca * ca - 4.0 * p * ca * cb * cg
                + 2.0 * (b2 - a2) / b2 * cg * cg)
    A1 = 4.0 * (-q * (1.0 + q) * cb + 2.0 * a2 / b2 * cg * cg * cb - (1.0 - p) * ca * cg)
    A0 = (1.0 + q) ** 2 - 4.0 * a2 / b2 * cg * cg
    return np.array([A0, A1, A2, A3, A4]), dict(j=j, a2=a2, b2=b2, c2=c2, ca=ca, cb=cb, cg=cg, q=q)


def quartic_by_substitution(aux) -> np.ndarray:
    """The same quartic from the law of cosines: u = N(v) / D(v) put into
    1 + u^2 - 2 u cos(gamma) = (c^2 / b^2) (1 + v^2 - 2 v cos(beta)), times D^2 (ascending)."""
    from numpy.polynomial import polynomial as Pl
    q, ca, cb, cg = aux["q"], aux["ca"], aux["cb"], aux["cg"]
    N = np.array([1.0 + q, -2.0 * q * cb, q - 1.0])
    D = np.array([2.0 * cg, -2.0 * ca])
    Q = np.array([1.0, -2.0 * cb, 1.0])
    DD = Pl.polymul(D, D)
    out = Pl.polyadd(Pl.polyadd(DD, Pl.polymul(N, N)), -2.0 * cg * Pl.polymul(N, D))
    return Pl.polysub(out, aux["c2"] / aux["b2"] * Pl.polymul(Q, DD))


def kabsch(Pw, Pc):
    """R, t with Pc ~ R Pw + t (least squares, proper rotation)."""
    mw, mc = Pw.mean(0), Pc.mean(0)
    H = (Pw - mw).T @ (Pc - mc)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, mc - R @ mw


def p3p_roots(img3, world3, K, sep: float = 1e-6):
    """-> (Rs [k, 3, 3], ts [k, 3], close): the poses of the admissible roots (v real and > 0,
    u = N(v) / D(v) > 0) of Grunert's quartic, ascending in v.  `close` is True when the count is
    ill-determined: two roots of the quartic (complex ones included) within `sep` relative of each
    other, or an admissible-root test (v > 0, u > 0, D(v) != 0) within `sep` of its boundary."""
    A, aux = grunert_quartic(img3, world3, K)
    if A is None:
        return np.zeros((0, 3, 3)), np.zeros((0, 3)), False
    amax = np.abs(A).max()
    hi = A[::-1].copy()
    while len(hi) > 1 and abs(hi[0]) <= 1e-14 * amax:      # the vanishing leading terms (cubic family)
        hi = hi[1:]
    r = np.roots(hi)
    close = False
    for i in range(len(r)):
        for k in range(i + 1, len(r)):
            if abs(r[i] - r[k]) <= sep * max(abs(r[i]), abs(r[k]), 1e-300):
                close = True
    q, ca, cb, cg, b2 = aux["q"], aux["ca"], aux["cb"], aux["cg"], aux["b2"]
    j, w = aux["j"], np.asarray(world3, np.float64).reshape(3, 3)
    Rs, ts = [], []
    for v in sorted(x.real for x in r if x.imag == 0.0):
        Dv = 2.0 * cg - 2.0 * ca * v
        Nv = (1.0 + q) - 2.0 * q * cb * v + (q - 1.0) * v * v
        if abs(v) <= sep or abs(Dv) <= sep * (abs(2.0 * cg) + abs(2.0 * ca * v)) or abs(Nv) <= sep * abs(Dv):
            close = True
        if not v > 0 or Dv == 0.0:
            continue
        u = Nv / Dv
        Qv = 1.0 - 2.0 * cb * v + v * v
        if not u > 0 or not Qv > 0:
            continue
        s1 = math.sqrt(b2 / Qv)
        Pc = np.stack([s1 * j[0], u * s1 * j[1], v * s1 * j[2]])
        R, t = kabsch(w, Pc)
        Rs.append(R)
        ts.append(t)
    return np.array(Rs).reshape(-1, 3, 3), np.array(ts).reshape(-1, 3), close


def _pose_case(rng, Xc, max_angle):
    """World points and pose (R, t) whose camera-frame points are Xc."""
    R = rodrigues(rng.normal(size=3), rng.uniform(0.05, max_angle))
    t = rng.normal(scale=2.0, size=3)
    return (Xc - t) @ R, R, t          # Xw = R^T (Xc - t)


def cam_points(rng, n, zlo, zhi):
    z = rng.uniform(zlo, zhi, n)
    u, v = rng.uniform(50, 1190, n), rng.uniform(20, 355, n)
    return np.stack([(u - KITTI_K[0, 2]) / KITTI_K[0, 0] * z, (v - KITTI_K[1, 2]) / KITTI_K[1, 1] * z, z], 1)


def cubic_triples(count: int, seed: int = 0xC0B1C, trim: float = 1e-15):
    """Triples whose quartic has a vanishing leading coefficient (Kq - 1)^2 - 4 (c^2/b^2) cos^2(alpha):
    it is zero exactly when the angle of the world triangle at w0 equals the angle between bearings
    1 and 2.  w1, w2 in front of the camera; w0 = the camera centre turned about the axis w1 w2 by
    2.6 .. 3.6 rad (it keeps its distances to w1 and w2, hence its angle over the chord), depth > 2.
    Kept: |A4| / max|A| <= trim in grunert_quartic.  -> list of (uv [3,2], Xw [3,3], R, t)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(200 * count):
        if len(out) == count:
            break
        w12 = cam_points(rng, 2, 4.0, 30.0)
        ax = w12[1] - w12[0]
        Rr = rodrigues(ax, rng.uniform(2.6, 3.6))
        w0 = w12[0] + Rr @ (np.zeros(3) - w12[0])
        if not w0[2] > 2.0:
            continue
        Xc = np.vstack([w0, w12])
        uv0 = project(KITTI_K, np.eye(3), np.zeros(3), Xc)
        if uv0.min() < -2000 or uv0.max() > 3000:
            continue
        Xw, R, t = _pose_case(rng, Xc, 2.5)
        uv = project(KITTI_K, R, t, Xw)
        A, _ = grunert_quartic(uv, Xw, KITTI_K)
        if abs(A[4]) <= trim * np.abs(A).max():
            out.append((uv, Xw, R, t))
    assert len(out) == count, "cubic_triples: the generator ran dry"
    return out


REF_REPROJ_PX = 1e-8


def well_posed(uv, Xw) -> bool:
    """A fixture triangle is kept when the float64 reference's own solutions all reproject the
    three points within REF_REPROJ_PX.  Grunert's elimination u = N(v) / D(v) loses digits where
    D(v) and N(v) vanish together (all four roots crowd near v = 1: views from near the
    triangle's axis); there numpy.roots + Kabsch is itself off by 1e-6 .. 1e-5 px, and says
    nothing about a bound of 1e-6 px on anyone else."""
    Rs, ts, _ = p3p_roots(uv, Xw, KITTI_K)
    return len(Rs) > 0 and max(reproj_px(KITTI_K, R, t, Xw, uv) for R, t in zip(Rs, ts)) <= REF_REPROJ_PX


def p3p_families():
    """-> (name -> list of (uv [3,2], Xw [3,3], R, t), n_dropped): noise free, K = KITTI_K; n_dropped
    counts the drawn triangles that well_posed() turned away."""
    rng = np.random.default_rng(0x9393)
    fam = {"large_rotation": [], "isosceles": [], "right_angle": [], "depth_50_to_1": []}
    dropped = [0]

    def add(name, case):
        if well_posed(case[0], case[1]):
            fam[name].append(case)
        else:
            dropped[0] += 1

    while len(fam["large_rotation"]) < 40:
        Xw, R, t = _pose_case(rng, cam_points(rng, 3, 5.0, 40.0), 2.5)
        add("large_rotation", (project(KITTI_K, R, t, Xw), Xw, R, t))
    while len(fam["depth_50_to_1"]) < 30:
        Xc = cam_points(rng, 3, 1.0, 2.0)
        Xc[rng.integers(0, 3)] *= rng.uniform(50.0, 60.0)           # one point 50 x deeper along its ray
        Xw, R, t = _pose_case(rng, Xc, 2.5)
        add("depth_50_to_1", (project(KITTI_K, R, t, Xw), Xw, R, t))

    def place(Xw):
        """A pose that sees the given world triangle from 8 .. 25 units, rotation <= 2.5 rad."""
        for _ in range(100):
            R = rodrigues(rng.normal(size=3), rng.uniform(0.05, 2.5))
            cen = cam_points(rng, 1, 8.0, 25.0)[0]
            t = cen - R @ Xw.mean(0)
            uv = project(KITTI_K, R, t, Xw)
            if ((Xw @ R.T + t)[:, 2] > 2.0).all() and uv.min() > -500 and uv.max() < 2000:
                return uv, Xw, R, t
        raise AssertionError("p3p_families: no pose found")

    g = lambda: rng.integers(-96, 97, 3) / 32.0                      # exact in binary: differences are exact
    while len(fam["isosceles"]) < 30:
        # |w1 - w2| == |w1 - w0| bit for bit: the two legs are the same components reordered/negated
        w1, d = g(), g()
        e = np.array([d[1], d[0], -d[2]])
        if np.linalg.norm(np.cross(d, e)) < 1.0:
            continue
        Xw = np.stack([w1 + d, w1, w1 + e])
        assert np.sum((Xw[1] - Xw[2]) ** 2) == np.sum((Xw[0] - Xw[1]) ** 2)
        add("isosceles", place(Xw))
    k = 0
    while len(fam["right_angle"]) < 30:
        # legs (p, q, 0) and (-q, p, r): orthogonal exactly, at vertex 0, 1, 2 in turn
        p, q, r = (int(x) / 16.0 for x in rng.integers(8, 64, 3))
        corner = g()
        legs = [corner + np.array([p, q, 0.0]), corner + np.array([-q, p, r])]
        Xw = np.stack(legs[: k % 3] + [corner] + legs[k % 3:])
        k += 1
        add("right_angle", place(Xw))
    fam["cubic"] = cubic_triples(12)
    return fam, dropped[0]


def reproj_px(K, R, t, Xw, uv) -> float:
    """Worst pixel distance of Xw under (R, t) from uv (inf behind the camera)."""
    Xc = Xw @ R.T + t
    if not (Xc[:, 2] > 0).all():
        return math.inf
    return float(np.linalg.norm(project(K, R, t, Xw) - uv, axis=1).max())


def pose_err(R, t, R0, t0) -> float:
    return float(np.abs(R - R0).max() + np.abs(t - t0).max())


# --------------------------------------------------------------------------- MSAC
def msac_sample(oracle, seed: int, frame_key: int, s: int, n: int):
    """The four distinct point indices of hypothesis slot s (None: none found in 16 attempts):
    Philox4x32-10 with counter (s, attempt, frame_key, 0x5EED) and key (seed, 0x9E3779B9), each
    word r mapped to (r * n) >> 32."""
    for att in range(16):
        r = oracle.philox((s, att, frame_key & 0xFFFFFFFF, 0x5EED), (seed, 0x9E3779B9))
        idx = [(int(x) * n) >> 32 for x in r]
        if len(set(idx)) == 4:
            return idx
    return None


def reproj_err2(R, t, K, X, uv) -> np.ndarray:
    """Squared pixel error per point, inf at or behind the camera plane."""
    Xc = X @ R.T + t
    z = Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        xn, yn = Xc[:, 0] / z, Xc[:, 1] / z
        e = (K[0, 0] * xn + K[0, 1] * yn + K[0, 2] - uv[:, 0]) ** 2 + (K[1, 1] * yn + K[1, 2] - uv[:, 1]) ** 2
    return np.where(z > 0, e, np.inf)


def trials_needed(n_in: int, n: int, conf: float) -> int:
    w4 = (n_in / n) ** 4
    if not w4 > 1e-300:
        return 0x7FFFFFFF
    if w4 >= 1.0 or not math.log(1.0 - w4) < 0:          # every point an inlier / 1 - w^4 rounds to 1
        return 1
    N = math.ceil(math.log(1.0 - conf) / math.log(1.0 - w4))
    return int(min(max(N, 1), 0x7FFFFFFF))


def msac_replay(oracle, img, world, K, max_num_trials=1000, confidence=99.0, max_reprojection_error=1.0,
                seed=0x5EED, frame_key=0):
    """-> dict(status, T, mask, n_inliers, best, slots, thr_gap, score_gap): M-estimator sample
    consensus as estworldpose runs it.  Slot s = sample, the oracle's P3P on the first three
    points, the solution with the smallest error at the fourth; score = sum of min(e, thr);
    a better score lowers the trial budget to log(1 - conf) / log(1 - w^4).
    thr_gap: smallest |e - thr| / thr over every scored (slot, point); score_gap: smallest relative
    difference of two scored slots' scores (slots with the same pose left aside).  Summation is
    numpy's: the result is the oracle's when both gaps are far above float64 rounding."""
    img = np.asarray(img, np.float64).reshape(-1, 2)
    world = np.asarray(world, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64).reshape(3, 3)
    n = img.shape[0]
    res = dict(status=-3, T=np.eye(4), mask=np.zeros(n, bool), n_inliers=0, best=-1, slots=[], thr_gap=math.inf,
               score_gap=math.inf)
    if n < 4:
        return res
    thr, conf = max_reprojection_error ** 2, confidence / 100.0
    budget, trials, best_score, best_in, best = max_num_trials, 0, math.inf, 0, None
    scored = []
    for s in range(max_num_trials):
        if not trials < budget:
            break
        idx = msac_sample(oracle, seed, frame_key, s, n)
        if idx is None:
            continue
        Rs, ts = oracle.p3p(img[idx[:3]], world[idx[:3]], K)
        e4 = [reproj_err2(R, t, K, world[idx[3:]], img[idx[3:]])[0] for R, t in zip(Rs, ts)]
        if not e4 or not min(e4) < math.inf:
            continue
        k = int(np.argmin(e4))
        trials += 1
        e = reproj_err2(Rs[k], ts[k], K, world, img)
        res["thr_gap"] = min(res["thr_gap"], float(np.abs(e[np.isfinite(e)] - thr).min(initial=math.inf) / thr))
        score, n_in = float(np.minimum(e, thr).sum()), int((e < thr).sum())
        for R0, t0, sc0 in scored:
            if not (np.array_equal(R0, Rs[k]) and np.array_equal(t0, ts[k])):
                res["score_gap"] = min(res["score_gap"], abs(score - sc0) / max(score, sc0))
        scored.append((Rs[k], ts[k], score))
        res["slots"].append(s)
        if score < best_score:
            best_score, best_in, best = score, n_in, (s, Rs[k], ts[k], e < thr)
            budget = min(budget, trials_needed(n_in, n, conf))
    if best is None or best_in < 4:
        res["status"] = -4
        return res
    s, R, t, mask = best
    T = np.eye(4)
    T[:3, :3] = R.T
    T[:3, 3] = [-(R[0, i] * t[0] + R[1, i] * t[1] + R[2, i] * t[2]) for i in range(3)]   # camera centre -R^T t
    res.update(status=0, T=T, mask=mask, n_inliers=int(mask.sum()), best=s)
    return res


def pose_problem(rng, n, outlier_frac, noise=0.2, outlier_px=(5.0, 40.0)):
    """n KITTI-like correspondences of a small forward motion: `noise` px Gaussian noise, a share
    of gross outliers (offsets of outlier_px magnitude, either sign).  The outlier share is exact:
    the first round(outlier_frac n) rows of a random order."""
    Xw = np.stack([rng.uniform(-15, 15, n), rng.uniform(-2, 2, n), rng.uniform(5, 60, n)], 1)
    R = rodrigues([0.0, 1.0, 0.0], np.deg2rad(0.4))
    t = np.array([0.02, -0.01, -0.95])
    uv = project(KITTI_K, R, t, Xw) + rng.normal(0, noise, (n, 2))
    bad = rng.permutation(n)[: int(round(outlier_frac * n))]
    uv[bad] += rng.uniform(*outlier_px, (len(bad), 2)) * rng.choice([-1.0, 1.0], (len(bad), 2))
    return uv, Xw, KITTI_K.copy()


# --------------------------------------------------------------------------- landmarks
def landmarks_np(l_pos, r_pos, old_l, old_r, P1, P2, pose, triangulate):
    """VO.m:145-160 + CreateLandmarksFromFeatures.m.  A stereo match is new unless its left x or
    left y equals ANY old left x / y, or its right x or y ANY old right x / y (exact equality);
    of the new matches the odd 1-based ones are triangulated (`triangulate`: the oracle's, whose
    points are rounded through single) and kept unless z < 0 or z > 80; the output has as many rows
    as the last kept one (at least the two of zeros(2, 3)), all others zero; kept rows are
    single(pose * [X; 1]).  -> (rows [R, 3] float64, info)."""
    l, r, ol, orr = (np.asarray(a, F32).reshape(-1, 2) for a in (l_pos, r_pos, old_l, old_r))
    pose = np.asarray(pose, np.float64).reshape(4, 4)
    hit = (np.isin(l[:, 0], ol[:, 0]) | np.isin(l[:, 1], ol[:, 1]) | np.isin(r[:, 0], orr[:, 0]) | np.isin(r[:, 1], orr[:, 1]))
    new = np.flatnonzero(~hit)
    odd = new[0::2]
    X = np.asarray(triangulate(l[odd], r[odd], P1, P2), np.float64).reshape(-1, 3)
    keep = ~(X[:, 2] < 0) & ~(X[:, 2] > 80)
    kept = np.flatnonzero(keep)
    rows = max(2, 2 * int(kept[-1]) + 1) if len(kept) else 2
    out = np.zeros((rows, 3))
    Xs = X[kept].astype(F32).astype(np.float64)
    for a in range(3):
        w = pose[a, 0] * Xs[:, 0] + pose[a, 1] * Xs[:, 1] + pose[a, 2] * Xs[:, 2] + pose[a, 3]
        out[2 * kept, a] = w.astype(F32)
    return out, dict(hit=hit, M=len(new), kept=len(kept))


LANDMARK_SIZES = [(0, 0), (1, 0), (2, 0), (3, 5), (1023, 7), (1024, 1023), (1025, 1024), (2049, 1025), (2500, 2100)]
LANDMARK_POSE = np.array([[0.9998, 0.0, 0.02, 1.5], [0.0, 1.0, 0.0, -0.2], [-0.02, 0.0, 0.9998, 30.0], [0.0, 0.0, 0.0, 1.0]])
COORDS = ("lx", "ly", "rx", "ry")


def stereo_rows(rng, S, zlo=2.0, zhi=120.0):
    """S KITTI-calibrated stereo matches (1-based single pixel positions), depths zlo .. zhi: the
    z > 80 gate takes its share."""
    X = np.stack([rng.uniform(-20, 20, S), rng.uniform(-3, 3, S), rng.uniform(zlo, zhi, S)], 1)
    tb = np.linalg.solve(KITTI_K, KITTI_P2[:, 3])
    l = (project(KITTI_K, np.eye(3), np.zeros(3), X) + 1.0).astype(F32)
    r = (project(KITTI_K, np.eye(3), tb, X) + 1.0).astype(F32)
    return l, r


def far_rows(rng, Kn):
    """Kn old points no stereo row can equal in any coordinate (the stereo rows are below 3000)."""
    return rng.uniform(5000, 9000, (Kn, 2)).astype(F32), rng.uniform(5000, 9000, (Kn, 2)).astype(F32)


def landmark_case(S, Kn, seed=0):
    """One (S, Kn) case with planted equalities -> (l, r, old_l, old_r, plants).  Old rows start
    far from every stereo row; then for each coordinate (lx, ly, rx, ry) and each pair of an
    old-row region (first 1024-chunk, later chunks, the last Kn % 8 rows) with a stereo-row region
    (rows < 1024, >= 1024, >= 2048) one old row takes that one coordinate of one stereo row.
    At most max(1, S // 3) plants, so new rows remain.
    plants: list of (coord, old row, stereo row); the hit set is exactly their stereo rows."""
    rng = np.random.default_rng([0x1A7D, S, Kn, seed])
    l, r = stereo_rows(rng, S)
    old_l, old_r = far_rows(rng, Kn)
    old_regions = [(0, min(Kn, 1024))]
    if Kn > 1024:
        old_regions.append((1024, Kn))
    if Kn > 2048:
        old_regions.append((2048, Kn))
    if Kn % 8:
        old_regions.append((Kn - Kn % 8, Kn))
    # (a round's only row stays new: it is what shows that round's compaction offset)
    st_regions = [(a, min(S, b)) for a, b in ((0, 1024), (1024, 2048), (2048, 1 << 30)) if S > a + 1 or (a == 0 and S)]
    plants, used_o, used_s = [], set(), set()
    if S and Kn:
        for c in (np.arange(4) + seed + S) % 4:              # small S: the first coordinate varies by case
            for oa, ob in old_regions:
                for sa, sb in st_regions:
                    if len(plants) >= max(1, S // 3):        # leave new rows
                        continue
                    free_o = [k for k in range(oa, ob) if k not in used_o]
                    free_s = [j for j in range(sa, sb) if j not in used_s]
                    if not free_o or not free_s:
                        continue
                    k, j = int(rng.choice(free_o)), int(rng.choice(free_s))
                    used_o.add(k)
                    used_s.add(j)
                    (old_l if c < 2 else old_r)[k, c & 1] = (l if c < 2 else r)[j, c & 1]
                    plants.append((COORDS[c], k, j))
    return l, r, old_l, old_r, plants


def landmark_variants():
    """name -> (l, r, old_l, old_r, expected dict): the constructed cases of the filter and the gates."""
    out = {}
    rng = np.random.default_rng(0x7A21)
    S = 40
    for M in (0, 1, 2, 3):
        # every stereo row but M of them equals an old row in one coordinate (cycling lx, ly, rx, ry)
        l, r = stereo_rows(rng, S, 3.0, 60.0)
        old_l, old_r = far_rows(rng, S)
        new = sorted(rng.choice(S, M, replace=False).tolist())
        for j in range(S):
            if j not in new:
                c = j % 4
                (old_l if c < 2 else old_r)[S - 1 - j, c & 1] = (l if c < 2 else r)[j, c & 1]
        out[f"M{M}"] = (l, r, old_l, old_r, dict(M=M))
    l, r = stereo_rows(rng, S, 81.0, 400.0)
    out["all_beyond_80"] = (l, r, *far_rows(rng, 9), dict(M=S, rows=2, kept=0))
    l, r = stereo_rows(rng, S, 3.0, 60.0)
    out["negative_disparity"] = (r.copy(), l.copy(), *far_rows(rng, 9), dict(M=S, rows=2, kept=0))
    # near rows first, then 13 rows beyond the z gate: the output ends at the last kept odd row
    ln, rn = stereo_rows(rng, 27, 3.0, 60.0)
    lf, rf = stereo_rows(rng, 13, 90.0, 300.0)
    out["tail_gated"] = (np.vstack([ln, lf]), np.vstack([rn, rf]), *far_rows(rng, 9), dict(M=S, rows=27, kept=14))
    return out
