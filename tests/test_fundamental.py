"""CPU: the specification of estimateFundamentalMatrix (include/vo_spec.h vo_fund_*), through its CPU
build tests/fund_ref -- the functions k_fund_msac calls, which tests/test_gpu_fundamental.py compares
with the kernel by bytes.  Here the reference is held to an independent evaluation written from the
definitions (fund_ref.norm8_svd / sampson_ld: numpy.linalg.svd for both decompositions, longdouble
sums), its properties are checked on every case, and a census is asserted so that the table the GPU
test replays reaches every branch.

Margins.  The Jacobi fit and the SVD evaluation are different but valid orders of f64 operations, so
they agree to the conditioning of the problem times rounding; every bound below is 100 x the figure the
C reference measured on these very inputs, the factor test_pose_refine.py uses for
the same reason.  Each test prints its figures before it asserts."""
import numpy as np
import pytest

import fund_ref as R

SEEDS = range(5)
NOISE = 0.3
# measured max|F - F_svd| over SEEDS and both motions at 0.3 px noise, x 100
SVD_BOUND = {8: 100 * 1.2e-10, 9: 100 * 6.4e-11, 65: 100 * 1.6e-12, 300: 100 * 7.9e-13}
NORM_ULPS = 4 * 2.0 ** -52            # |F| = 1 after one division per entry and a sqrt: a few ulp
DET_BOUND = 100 * 1.8e-19             # measured max |det F| 1.8e-19 (n = 8; 4.5e-21 and below from n = 9 on)
# measured max Sampson distance of noise-free points (px^2), x 100; see test_noise_free_points_lie_on_their_epipolar_lines
CLEAN_SAMPSON = {8: 100 * 1.2e-7, 9: 100 * 1.2e-9, 65: 100 * 5.5e-10, 300: 100 * 1.1e-9}
# |d - thr| <= BAND_REL * thr: where the f64 and the longdouble evaluation of d may fall on different sides.  At
# d = thr = 0.1 px^2 the residual r ~ 0.03 is off by ~1e-14 (see the noise-free test), 1e-12 relative in d; x 1000
BAND_REL = 1e-9


def _properties(F):
    return abs(np.linalg.norm(F) - 1.0), F[2, 2], abs(np.linalg.det(F))


@pytest.mark.parametrize("n", [8, 9, 65, 300])
def test_norm8_agrees_with_the_svd_evaluation(n):
    worst, props, sweeps = 0.0, [0.0, 1.0, 0.0], [0, 0]
    for motion in R.MOTIONS:
        for seed in SEEDS:
            x1, x2, _ = R.case(n, motion, NOISE, 0.0, seed)
            ok, F, sw = R.norm8(x1, x2)
            assert ok
            worst = max(worst, float(np.abs(F - R.norm8_svd(x1, x2)).max()))
            a, b, c = _properties(F)
            props = [max(props[0], a), min(props[1], b), max(props[2], c)]
            sweeps = [max(sweeps[0], sw[0]), max(sweeps[1], sw[1])]
    print(f"n={n}: max|F - F_svd| {worst:.3g}, | |F| - 1 | {props[0]:.3g}, min F[8] {props[1]:.3g}, |det F| {props[2]:.3g}, "
          f"sweeps {sweeps}")
    assert worst <= SVD_BOUND[n]
    assert props[0] <= NORM_ULPS and props[1] >= 0.0 and props[2] <= DET_BOUND
    assert sweeps[0] < 30 and sweeps[1] < 30                  # the cap never binds


@pytest.mark.parametrize("n", [8, 9, 65, 300])
def test_noise_free_points_lie_on_their_epipolar_lines(n):
    """Without noise the only error is the rounding of the pixels to single (2^-14 px at x ~ 1000),
    amplified by the conditioning of the fit: worst at the minimal n = 8."""
    worst = 0.0
    for motion in R.MOTIONS:
        for seed in SEEDS:
            x1, x2, _ = R.case(n, motion, 0.0, 0.0, seed)
            ok, F, _ = R.norm8(x1, x2)
            assert ok
            d = R.sampson(F, x1, x2)
            worst = max(worst, float(d.max()))
            # sqrt(d) = |r| / |grad|: r sums three terms of size <= |x| |F x| ~ 50 in f64, so it is off by ~1e-14, and
            # |grad| ~ 0.07: the distance in px agrees with the longdouble evaluation to ~1.4e-13; 100 x that
            assert np.abs(np.sqrt(d) - np.sqrt(R.sampson_ld(F, x1, x2))).max() <= 1.4e-11
    print(f"n={n}: max noise-free Sampson distance {worst:.3g} px^2")
    assert worst <= CLEAN_SAMPSON[n]


def test_masked_fit_and_sample_fit_are_the_fit_of_their_rows():
    x1, x2, _ = R.case(129, "general", NOISE, 0.0, 9)
    mask = np.arange(129) % 3 != 1
    ok, F, _ = R.norm8(x1, x2, mask)
    assert ok and np.abs(F - R.norm8_svd(x1, x2, mask)).max() <= SVD_BOUND[65]
    idx = np.array([5, 99, 17, 64, 3, 128, 40, 77], np.uint32)
    ok, Fs, _ = R.sample_fit(x1, x2, idx)
    assert ok and np.abs(Fs - R.norm8_svd(x1[idx], x2[idx])).max() <= SVD_BOUND[8]
    a, b, c = _properties(Fs)
    assert a <= NORM_ULPS and b >= 0 and c <= DET_BOUND


def test_jacobi_against_eigh():
    rng = np.random.default_rng(5)
    for n in (3, 9):
        for _ in range(20):
            B = rng.normal(size=(n + 3, n))
            A = B.T @ B
            lam, V, j, sw = R.jacobi(A)
            w, _ = np.linalg.eigh(A)
            assert sw < 30 and j == int(np.argmin(lam))
            assert np.abs(np.sort(lam) - w).max() <= 1e-13 * w.max()
            assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-14
            assert np.abs(A @ V[:, j] - lam[j] * V[:, j]).max() <= 1e-13 * w.max()
    lam, V, j, sw = R.jacobi(np.diag([3.0, 1.0, 1.0]))          # nothing to rotate: one sweep; ties go to the lowest index
    assert sw == 1 and j == 1 and np.array_equal(V, np.eye(3))
    A = np.full((3, 3), np.nan)
    assert R.jacobi(A)[3] == 30                                  # a NaN is never skipped: the cap ends the loop


def test_sample_trial_bound_and_nan_distance():
    ok, idx, att = R.sample(0x5EED, 0, 0, 300)
    assert ok and len(set(idx.tolist())) == 8 and idx.max() < 300
    assert not R.sample(0x5EED, 0, 0, 7)[0] and R.sample(0x5EED, 0, 0, 7)[2] == 16
    assert R.sample(0x5EED, 1, 0, 300)[1].tolist() != idx.tolist() and R.sample(0x5EEE, 0, 0, 300)[1].tolist() != idx.tolist()
    valid8 = [s for s in range(2000) if R.sample(0x5EED, 0, s, 8)[0]]
    assert 0.02 < len(valid8) / 2000 < 0.07                      # 1 - (1 - 8!/8^8)^16 = 3.8 %
    assert all(sorted(R.sample(0x5EED, 0, s, 8)[1].tolist()) == list(range(8)) for s in valid8)
    # ceil(log(0.01) / log(1 - w^8))
    for n_in, n in ((150, 300), (240, 300), (299, 300), (30, 300)):
        w8 = (n_in / n) ** 8
        exact = np.log(0.01) / np.log1p(-w8)
        # the spec rounds 1 - w^8 before the log: a relative error of 2^-53 / w^8 in the bound
        assert abs(R.trials_needed(n_in, n, 0.99) - np.ceil(exact)) <= 1 + exact * 2.0 ** -52 / w8
    assert R.trials_needed(300, 300, 0.99) == 1
    # 1 - w^8 rounds to 1 once w^8 < 2^-53, i.e. w < 0.0101: no bound (not 1 trial)
    assert R.trials_needed(3, 300, 0.99) == R.NO_BOUND and R.trials_needed(2, 300, 0.99) == R.NO_BOUND
    assert R.trials_needed(0, 300, 0.99) == R.NO_BOUND and R.trials_needed(4, 300, 0.99) == R.NO_BOUND      # N > 2^31 - 1
    # 0 / 0 is NaN: no inlier, scored as the threshold
    x = np.float32([[3.0, 4.0]])
    d = R.sampson(np.zeros((3, 3)), x, x)
    assert np.isnan(d[0]) and not (d[0] < 0.01)


@pytest.fixture(scope="module")
def results():
    return {name: (R.estimate(x1, x2, key, **p), x1, x2, p, key) for name, x1, x2, p, key in R.table()}


def test_msac_mask_is_the_threshold_rule_on_the_best_slot(results):
    """mask == (d < thr) with d evaluated independently (longdouble) on the best slot's own F, except
    within a relative rounding band of the threshold; F is the masked fit over that mask; status and
    n_inliers follow."""
    in_band = total = 0
    for name, (r, x1, x2, p, key) in results.items():
        if p["method"] != R.MSAC or r["status"] != R.OK:
            assert r["status"] != R.OK or (r["inliers"].all() and r["n_inliers"] == len(x1))
            continue
        thr = p["distance_threshold"]
        d = R.sampson_ld(r["best_F"], x1, x2)
        band = np.abs(d - thr) <= BAND_REL * thr
        in_band += int(band.sum())
        total += len(d)
        assert np.array_equal(r["inliers"][~band], (d < thr)[~band]), name
        assert r["n_inliers"] == int(r["inliers"].sum()) >= 8
        ok, F, _ = R.norm8(x1, x2, r["inliers"])
        assert ok and F.tobytes() == r["F"].tobytes()
        a, b, c = _properties(r["F"])
        assert a <= NORM_ULPS and b >= 0 and c <= 1e-16
    print(f"{in_band} of {total} points within the rounding band of the threshold")
    assert in_band <= 0.01 * total


def test_msac_finds_the_motion_and_drops_the_outliers():
    for motion in R.MOTIONS:
        x1, x2, bad = R.case(300, motion, 0.1, 0.3, 21)
        r = R.estimate(x1, x2, 0, distance_threshold=0.1)
        assert r["status"] == R.OK
        assert r["inliers"][bad].mean() < 0.05 and r["inliers"][~bad].mean() > 0.8
        d = R.sampson(r["F"], x1[~bad], x2[~bad])
        assert np.median(d) < 0.05
        # the planted motion's own F explains the rows MSAC kept as well as the estimate does (to the noise: 0.1 px)
        keep = r["inliers"] & ~bad                       # (a random second point may fall on its epipolar line by chance)
        dt = R.sampson_ld(R.true_F(motion), x1[keep], x2[keep])
        assert np.median(dt) < 0.05 and dt.max() < 1.0


def test_failed_calls_return_zeros(results):
    for name in ("n0", "norm8_n7", "msac_n7", "all_same", "all_same_norm8", "few_inliers", "no_bound", "msac_n9_noisy"):
        r = results[name][0]
        assert r["status"] in (R.TOO_FEW, R.NO_CONSENSUS) and not r["F"].any() and not r["inliers"].any() and r["n_inliers"] == 0


def test_census(results):
    """Every branch the kernel has is reached by the table the GPU test replays."""
    cen = {k: v[0]["census"] for k, v in results.items()}
    st = {k: v[0]["status"] for k, v in results.items()}
    msac = [k for k, v in results.items() if v[3]["method"] == R.MSAC and len(v[1]) >= 8]
    # sizes, chunk edges, both methods
    assert {len(v[1]) for v in results.values()} >= {0, 7, 8, 9, 63, 64, 65, 129, 300}
    assert {v[3]["num_trials"] for v in results.values()} >= {1, 10, 64, 65, 500}
    assert {v[3]["method"] for v in results.values()} == {R.NORM8, R.MSAC}
    # an adaptive stop before num_trials, and num_trials exhausted
    early = [k for k in msac if cen[k]["trials"] == cen[k]["bound"] < results[k][3]["num_trials"]]
    spent = [k for k in msac if cen[k]["slots"] == results[k][3]["num_trials"] and cen[k]["bound"] == results[k][3]["num_trials"]]
    assert early and spent
    # a stop in the first chunk and in a later one (chunks of 64 slots)
    assert any(cen[k]["slots"] <= 64 for k in early) and any(cen[k]["slots"] > 64 for k in early)
    assert any(64 < cen[k]["slots"] and cen[k]["slots"] % 64 not in (0,) for k in early)
    # a bound that fell below the trials already made: the loop stops at once
    assert any(cen[k]["bound"] < cen[k]["trials"] for k in msac)
    # a duplicate-index re-attempt; slots invalid after 16 attempts (n = 8 and 9)
    assert any(cen[k]["reattempt"] for k in msac)
    assert cen["msac_n8"]["no_sample"] > 0 and cen["msac_n9"]["no_sample"] > 0 and cen["msac_n8_tie"]["no_sample"] > 0
    # equal scores meet the strict <: the first of them stays the best
    assert cen["msac_n8_tie"]["trials"] > 1 and cen["msac_n8_tie"]["improved"] < cen["msac_n8_tie"]["trials"]
    assert any(cen[k]["ties"] for k in msac)
    # a degenerate sample of coincident points, with and without a model
    x1, x2 = results["coincident"][1:3]
    deg = 0
    for s in range(cen["coincident"]["slots"]):
        ok, idx, _ = R.sample(0x5EED, results["coincident"][4], s, len(x1))
        deg += ok and len({tuple(x1[i]) for i in idx}) < 8
    assert deg > 0 and st["coincident"] == R.OK
    assert cen["all_same"]["no_model"] > 0 and cen["all_same"]["trials"] == 0 and st["all_same"] == R.NO_CONSENSUS
    assert st["all_same_norm8"] == R.NO_CONSENSUS
    # the den == 0 no-bound branch
    assert cen["no_bound"]["no_bound"] > 0 and any(cen[k]["no_bound"] and st[k] == R.OK for k in msac)
    # TOO_FEW at n = 7; NO_CONSENSUS with no valid slot and with fewer than 8 inliers
    assert st["msac_n7"] == st["norm8_n7"] == st["n0"] == R.TOO_FEW
    assert st["all_same"] == R.NO_CONSENSUS and cen["all_same"]["best"] < 0
    assert st["few_inliers"] == R.NO_CONSENSUS and cen["few_inliers"]["best"] >= 0
    # a refit with and without a final partial
    assert [results[f"refit_{m}"][0]["n_inliers"] for m in (63, 64, 65)] == [63, 64, 65]
    assert all(st[f"refit_{m}"] == R.OK for m in (63, 64, 65))
    # the sweep counts the cap is judged by
    s9 = max(c["sweeps9"] for c in cen.values())
    s3 = max(c["sweeps3"] for c in cen.values())
    print(f"sweeps: at most {s9} at 9 x 9 and {s3} at 3 x 3 over the table; stops at",
          sorted({cen[k]['slots'] for k in msac}))
    assert s9 < 30 and s3 < 30


# ----------------------------------------------------------------- refusals on the host
def test_bad_parameters_and_points_are_refused_on_the_host(vo):
    x1, x2, _ = R.case(20, "general", 0.1, 0.0, 1)
    for kw in (dict(method=2), dict(method=-1), dict(num_trials=0), dict(num_trials=100001), dict(distance_threshold=0.0),
               dict(distance_threshold=-1.0), dict(distance_threshold=float("nan")), dict(distance_threshold=float("inf")),
               dict(confidence=0.0), dict(confidence=100.0), dict(confidence=float("nan"))):
        with pytest.raises(vo.VOError) as e:
            vo.check_fund_params(vo.default_fund_params(**kw))
        assert e.value.code == vo.VO_ERR_ARG and next(iter(kw)) in str(e.value)
    vo.check_fund_params(vo.default_fund_params())
    vo.check_fund_params(vo.default_fund_params(method=vo.VO_FUND_NORM8, num_trials=100000, confidence=99.999))
    with pytest.raises(vo.VOError) as e:
        vo.default_fund_params(trials=3)
    assert e.value.code == vo.VO_ERR_ARG
    for bad_val in (np.nan, np.inf, -np.inf):
        b = x2.copy()
        b[13, 1] = bad_val
        with pytest.raises(vo.VOError) as e:
            vo.fund_points(x1, b)
        assert e.value.code == vo.VO_ERR_ARG and "matchedPoints2 row 13" in str(e.value)
    with pytest.raises(vo.VOError) as e:
        vo.fund_points(x1, x2[:19])
    assert e.value.code == vo.VO_ERR_ARG
    with pytest.raises(vo.VOError) as e:
        vo.fund_points(x1.reshape(-1, 4), x2.reshape(-1, 4))
    assert e.value.code == vo.VO_ERR_ARG
    # the module-level function refuses what it does not implement before it needs a device
    for kw in (dict(Method="RANSAC"), dict(Method="LMedS"), dict(Method="LTS"), dict(DistanceType="Algebraic"),
               dict(InlierPercentage=50), dict(NumTrials=0), dict(Confidence=100.0), dict(DistanceThreshold=0.0)):
        with pytest.raises(vo.VOError) as e:
            vo.estimateFundamentalMatrix(x1, x2, **kw)
        assert e.value.code == vo.VO_ERR_ARG
    kp = np.zeros(20, vo.KP_DTYPE)
    kp["x"], kp["y"] = x1[:, 0], x1[:, 1]
    a, b = vo.fund_points(kp, x2)
    assert a.dtype == np.float32 and np.array_equal(a, x1) and a.flags.c_contiguous


def test_exports_and_header(vo):
    import re
    from pathlib import Path
    hdr = (Path(__file__).resolve().parent.parent / "include" / "vo.h").read_text()
    for sym in ("vo_default_fund_params", "vo_est_fundamental", "vo_est_fundamental_batch"):
        assert sym in vo.EXPORTS and re.search(rf"\b{sym}\(", hdr)
    assert hasattr(vo.Context, "est_fundamental") and hasattr(vo.Context, "est_fundamental_batch")
    import ctypes
    assert ctypes.sizeof(vo.FundParams) == 32                 # vo_fund_params: two int32, two doubles, a uint32, padding
