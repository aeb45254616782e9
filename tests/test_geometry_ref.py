"""The CPU oracle's geometry (triangulate, P3P, estworldpose, landmarks) against the float64
numpy references of geom_ref.py, which are written from the definitions: the GPU tests compare
libvo.so with the oracle, and the two mirror each other operation for operation -- these tests
are what says the oracle itself is right."""
import numpy as np
import pytest

import geom_ref as G

K = G.KITTI_K


# ----------------------------------------------------------------- triangulate
TRI_MEASURED = 0.9722       # worst ratio over the three fixtures (see the docstring below)


@pytest.fixture(scope="module")
def tri_fixtures():
    return G.tri_fixtures()


@pytest.mark.parametrize("name", ["kitti_low_disparity", "one_based", "general_P2"])
def test_triangulate_against_svd(oracle, tri_fixtures, name):
    """oracle.triangulate (one-sided Jacobi on the 4x4 DLT system, result rounded through single)
    against numpy's SVD of the same system.  Error unit: 2^-24 max|ref row|, the rounding of the
    row's largest coordinate to single.  Measured worst ratios: kitti_low_disparity (2000 points,
    disparity 0.5 .. 120 px) 0.972, one_based 0.943, general_P2 0.958 -- the single rounding
    alone; the Jacobi / LAPACK difference is below 1e-6 of it.  Asserted at 4 x the worst.  Rows
    whose reference null vector has |w| / |v| < 1e-6 (a point near infinity) are left out: none
    on these fixtures (smallest |w| / |v|: 1.06e-3), at most 1 % allowed."""
    x1, x2, P1, P2 = tri_fixtures[name]
    ref, wn = G.tri_svd(x1, x2, P1, P2)
    got = oracle.triangulate(x1, x2, P1, P2)
    ok = wn >= 1e-6
    assert (~ok).mean() <= 0.01
    ratio = G.tri_ulp_ratio(got[ok], ref[ok]).max()
    print(f"{name}: worst ratio {ratio:.3f}, excluded {(~ok).mean():.4f}, min |w|/|v| {wn.min():.3e}")
    assert np.isfinite(got[ok]).all()
    assert ratio <= 4 * TRI_MEASURED


# ----------------------------------------------------------------- P3P
@pytest.fixture(scope="module")
def families():
    return G.p3p_families()


def test_quartic_closed_form_equals_substitution(families):
    """The published closed form of Grunert's coefficients equals the law-of-cosines substitution
    carried out with numpy's polynomial products -- two derivations of the reference's quartic.
    Bound: either form is under 40 operations on terms no larger than
    T = (1 + |q|)^2 + 4 (a^2 + b^2 + c^2) / b^2, so they differ by less than 80 eps T."""
    fam, _ = families
    for cases in fam.values():
        for uv, Xw, _, _ in cases:
            A, aux = G.grunert_quartic(uv, Xw, K)
            B = G.quartic_by_substitution(aux)
            T = (1 + abs(aux["q"])) ** 2 + 4 * (aux["a2"] + aux["b2"] + aux["c2"]) / aux["b2"]
            assert np.abs(A - B).max() <= 80 * np.finfo(float).eps * T


def test_fixture_triangles_dropped_for_conditioning(families):
    """well_posed() (the reference's own solutions reproject within 1e-8 px) turns away few of the
    drawn triangles: 4 of 134 with this seed.  What it turns away are isosceles / right-angled
    triangles seen from near their axis, where u = N / D is 0 / 0 for all four roots and numpy's
    own solutions are off by up to 5e-6 px (the oracle's by up to 1.4e-5 px on the same ones)."""
    fam, dropped = families
    drawn = dropped + sum(len(v) for k, v in fam.items() if k != "cubic")
    print(f"dropped {dropped} of {drawn}")
    assert dropped <= 0.05 * drawn


@pytest.mark.parametrize("name", ["large_rotation", "isosceles", "right_angle", "depth_50_to_1", "cubic"])
def test_p3p_against_roots(oracle, families, name):
    """oracle.p3p (polynomial products, bracketing + bisection, frame alignment) against
    p3p_roots (closed-form coefficients, numpy.roots, Kabsch) as solution sets: every oracle
    solution reprojects its three points within 1e-6 px; the generating pose is among them within
    2e-5 (test_p3p_recovers_pose's measure); and there are as many as the reference has admissible
    roots, unless the reference's roots are closer than 1e-6 relative.
    Families: rotations up to 2.5 rad; isosceles triangles with a^2 == c^2 bit for bit (Kq = 0);
    a right angle at each vertex in turn; one point 50 x deeper than the others; triangles whose
    quartic's leading coefficient vanishes (the cubic path of the root finder).
    Measured (worst per family): reprojection 2.9e-9 / 1.8e-8 / 7.3e-9 / 7.0e-9 / 1.2e-11 px, pose
    9.0e-10 / 5.2e-10 / 1.4e-9 / 1.4e-11 / 1.2e-12; no case skipped for close roots."""
    fam, _ = families
    worst_px = worst_pose = 0.0
    for uv, Xw, R, t in fam[name]:
        Rs, ts = oracle.p3p(uv, Xw, K)
        rRs, _, close = G.p3p_roots(uv, Xw, K)
        assert 1 <= len(Rs) <= 4
        for Ri, ti in zip(Rs, ts):
            assert abs(np.linalg.det(Ri) - 1.0) < 1e-12 and np.abs(Ri @ Ri.T - np.eye(3)).max() < 1e-12
            px = G.reproj_px(K, Ri, ti, Xw, uv)
            worst_px = max(worst_px, px)
            assert px <= 1e-6
        err = min(G.pose_err(Ri, ti, R, t) for Ri, ti in zip(Rs, ts))
        worst_pose = max(worst_pose, err)
        assert err < 2e-5
        if not close:
            assert len(Rs) == len(rRs), (len(Rs), len(rRs))
    print(f"{name}: worst reprojection {worst_px:.2e} px, worst pose error {worst_pose:.2e}")


def test_p3p_share_skipped_for_close_roots(families):
    """At most 5 % of all the P3P cases may have gone without the solution count."""
    fam, _ = families
    close = [G.p3p_roots(uv, Xw, K)[2] for cases in fam.values() for uv, Xw, _, _ in cases]
    assert len(close) == 142 and np.mean(close) <= 0.05


def test_cubic_family_is_cubic(oracle, families):
    """The cubic fixture: |A4| <= 1e-15 max|A| in the reference's coefficients (ten times inside the
    root finder's 1e-14 trim, so another evaluation order trims too), the other coefficients do
    not vanish, and the oracle recovers the generating pose to 1e-8 (measured 1.2e-12)."""
    fam, _ = families
    for uv, Xw, R, t in fam["cubic"]:
        A, _ = G.grunert_quartic(uv, Xw, K)
        assert abs(A[4]) <= 1e-15 * np.abs(A).max() and abs(A[3]) > 1e-3 * np.abs(A).max()
        Rs, ts = oracle.p3p(uv, Xw, K)
        assert min(G.pose_err(Ri, ti, R, t) for Ri, ti in zip(Rs, ts)) < 1e-8


# ----------------------------------------------------------------- estworldpose
# (n, outlier share, outlier offsets px, MaxNumTrials, MaxReprojectionError, Confidence, frame keys)
# The keys are those at which the reference's own run meets the gap conditions below.
MSAC_FIXTURES = [
    (300, 0.3, (1.5, 6.0), 1000, 1.0, 99.0, (0, 8, 11, 17)),
    (257, 0.4, (2.0, 10.0), 50, 2.0, 99.0, (0, 10, 34)),
]


@pytest.mark.parametrize("fx", MSAC_FIXTURES, ids=lambda f: f"n{f[0]}")
def test_estworldpose_against_replay(oracle, fx):
    """oracle.estworldpose against msac_replay: the sampler restated in Python, scores, inlier
    counts, the adaptive trial budget and the mask in numpy float64 (numpy's summation, not the
    64-lane tree).  Status, pose, mask and inlier count are equal.  Conditions on the inputs,
    asserted on the reference: no point's error within 1e-9 relative of the threshold in any
    scored slot, no two scored slots' scores within 1e-9 relative (measured at the closest: 1.1e-3
    and 5.3e-6).  18 .. 47 slots are scored per run; at key 34 of the second fixture the winner is
    the last slot scored, slot 47 of 50."""
    n, frac, px, trials, err, conf, keys = fx
    uv, Xw, Kk = G.pose_problem(np.random.default_rng([n, 7]), n, frac, 0.2, px)
    rp = oracle.ransac_params(trials)
    rp.max_reprojection_error, rp.confidence = err, conf
    for key in keys:
        ref = G.msac_replay(oracle, uv, Xw, Kk, trials, conf, err, rp.seed, key)
        assert ref["thr_gap"] > 1e-9 and ref["score_gap"] > 1e-9
        assert len(ref["slots"]) >= 10
        st, T, inl, nin = oracle.estworldpose(uv, Xw, Kk, params=rp, frame_key=key)
        assert st == ref["status"] == 0
        assert np.array_equal(T, ref["T"]), key
        assert np.array_equal(inl, ref["mask"]) and nin == ref["n_inliers"]
        assert nin >= 0.5 * n


def test_trials_needed_known_values():
    """log(1 - conf) / log(1 - w^4), rounded up, at least 1."""
    assert G.trials_needed(300, 300, 0.99) == 1
    assert G.trials_needed(150, 300, 0.99) == 72          # log(0.01) / log(15/16) = 71.36
    assert G.trials_needed(0, 300, 0.99) == 0x7FFFFFFF
    assert G.trials_needed(3, 4, 0.99) == 13              # log(0.01) / log(1 - 81/256) = 12.11


# ----------------------------------------------------------------- landmarks
@pytest.mark.parametrize("S,Kn", G.LANDMARK_SIZES)
def test_landmarks_np_equals_oracle(oracle, S, Kn):
    """landmarks_np (numpy.isin per coordinate) is oracle.landmarks bit for bit on every planted
    (S, Kn) case of the GPU test, and the filter's hit set is exactly the planted rows."""
    l, r, old_l, old_r, plants = G.landmark_case(S, Kn)
    ref = oracle.landmarks(l, r, old_l, old_r, G.KITTI_P1, G.KITTI_P2, G.LANDMARK_POSE)
    got, info = G.landmarks_np(l, r, old_l, old_r, G.KITTI_P1, G.KITTI_P2, G.LANDMARK_POSE, oracle.triangulate)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()
    assert sorted(np.flatnonzero(info["hit"]).tolist()) == sorted(j for _, _, j in plants)
    if S >= 1023:
        assert {c for c, _, _ in plants} == set(G.COORDS)
        assert info["kept"] > 100 and len(ref) > S // 2


def test_landmarks_variants_equal_oracle(oracle):
    """The constructed cases: M = 0 .. 3 new rows, every depth beyond 80, negative disparity, a
    gated tail -- landmarks_np == oracle.landmarks, and M / rows / kept are the constructed ones."""
    for name, (l, r, old_l, old_r, want) in G.landmark_variants().items():
        ref = oracle.landmarks(l, r, old_l, old_r, G.KITTI_P1, G.KITTI_P2, G.LANDMARK_POSE)
        got, info = G.landmarks_np(l, r, old_l, old_r, G.KITTI_P1, G.KITTI_P2, G.LANDMARK_POSE, oracle.triangulate)
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), name
        assert info["M"] == want["M"], name
        if "rows" in want:
            assert len(ref) == want["rows"] and info["kept"] == want["kept"], name
        if want["M"] <= 2:
            assert len(ref) == 2, name
