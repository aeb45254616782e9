"""triangulate's reprojectionErrors / validIndex on the CPU: the reference of the GPU tests
(tests/tri_quality_ref: include/vo_spec.h's vo_tri_quality, compiled with the oracle's flags) against
an independent longdouble evaluation of the formula in include/vo.h, the facts the two outputs are
for (a point behind the cameras reprojects perfectly; a row offset shows in the error), the
non-finite classes, and the MEX gateway's dispatch on the number of outputs against the recording
fake libvo, which has no vo_triangulate_ex."""
import numpy as np
import pytest

import geom_ref as G
import mexshim
import tri_quality_ref as T

P1, P2 = G.KITTI_P1, G.KITTI_P2
FIXTURE_ROWS = {"kitti_low_disparity": 2000, "one_based": 500, "general_P2": 500}


@pytest.mark.parametrize("name", sorted(FIXTURE_ROWS))
def test_reference_against_longdouble(oracle, name):
    """|err - err_ld| <= ulp32(err_ld) + 1e-9 px: the single rounding of the result, plus the
    cancellation in h0 / w - u, where the float64 error of a projection of magnitude 2^11 is about
    1e-12.  valid equal.  Every fixture row is valid with a finite error (not vacuous)."""
    x1, x2, Pa, Pb = G.tri_fixtures()[name]
    assert len(x1) == FIXTURE_ROWS[name]
    X = oracle.triangulate(x1, x2, Pa, Pb)
    err, valid = T.quality(x1, x2, X, Pa, Pb)
    err_ld, valid_ld = T.quality_longdouble(x1, x2, X, Pa, Pb)
    assert err.dtype == np.float32 and valid.dtype == bool
    assert np.isfinite(err).all() and valid.all()
    assert np.array_equal(valid, valid_ld)
    bound = np.spacing(err_ld.astype(np.float32)).astype(np.longdouble) + np.longdouble(1e-9)
    ratio = np.abs(err.astype(np.longdouble) - err_ld) / bound
    print(f"{name}: worst |err - err_ld| / bound = {float(ratio.max()):.3f}, err in [{err.min():.3g}, {err.max():.3g}] px")
    assert (ratio <= 1).all()


def test_probe_rows(oracle):
    """Under the KITTI calibration: negative disparity triangulates behind the cameras with a perfect
    reprojection, so only valid catches it; zero disparity gives a finite point beyond 1e17 that
    counts as in front; half a pixel of row offset is an error of exactly 0.25 px."""
    X = oracle.triangulate(T.PROBE_X1, T.PROBE_X2, P1, P2)
    err, valid = T.quality(T.PROBE_X1, T.PROBE_X2, X, P1, P2)
    print("X", X.tolist(), "err", err.tolist(), "valid", valid.tolist())
    assert valid.tolist() == [False, True, True, True]
    assert X[0, 2] < 0 and err[0] < 1e-6
    assert err[2] == np.float32(0.25)
    for k in (1, 3):
        assert np.isfinite(X[k]).all() and np.isfinite(err[k]) and abs(X[k, 2]) > 1e17


def test_non_finite_classes():
    """X rows holding NaN, +inf and -inf (in every coordinate, and NaN in each one alone), and a P
    whose third row makes w exactly 0: valid is 0, err is the NaN or inf IEEE arithmetic gives.
    (0 * inf is NaN, so under P's third row (0, 0, 1, 0) an infinite X0 or X1 makes w NaN.)"""
    nan, inf = np.nan, np.inf
    X = np.array([[nan] * 3, [inf] * 3, [-inf] * 3, [nan, 1, 10], [1, nan, 10], [1, 1, nan], [inf, 1, 10], [1, -inf, 10],
                  [-inf, inf, 5]])
    x = np.tile(np.float32([[600, 180]]), (len(X), 1))
    err, valid = T.quality(x, x, X, P1, P2)
    assert not valid.any()
    assert np.isnan(err).all()
    # w = 0 in the second view only: h / 0 is +-inf (or NaN where h is 0 too), the mean is not finite
    Pz = P2.copy()
    Pz[2] = 0.0
    Xf = np.array([[1.0, 2.0, 10.0], [-3.0, 0.5, 20.0], [0.0, 0.0, 5.0]])
    xf = np.tile(np.float32([[600, 180]]), (3, 1))
    err, valid = T.quality(xf, xf, Xf, P1, Pz)
    assert not valid.any() and not np.isfinite(err).any()
    assert np.isposinf(err[0]) and np.isposinf(err[1])
    err_ld, valid_ld = T.quality_longdouble(xf, xf, Xf, P1, Pz)
    assert not valid_ld.any() and np.array_equal(np.isnan(err), np.isnan(err_ld))
    # and w = 0 in the first view alone is enough
    err, valid = T.quality(xf, xf, Xf, Pz, P2)
    assert not valid.any() and not np.isfinite(err).any()


@pytest.fixture(scope="module")
def mex():
    mexshim.build()
    m = mexshim.Mex(mexshim.FAKE)
    yield m
    m.at_exit()


def test_gateway_dispatches_on_outputs_with_the_fake_libvo(mex):
    """One output calls vo_triangulate as before.  The fake libvo has no vo_triangulate_ex (the
    gateway's weak reference is null), so two or three outputs raise vo:triangulate:unavailable
    rather than come back empty."""
    rng = np.random.default_rng(3)
    x1 = rng.uniform(0, 1000, (4, 2)).astype(np.float32)
    x2 = rng.uniform(0, 1000, (4, 2)).astype(np.float32)
    Pa, Pb = rng.normal(size=(3, 4)), rng.normal(size=(3, 4))
    X = mex.call("triangulate", x1, x2, Pa, Pb, nout=1)
    assert X.dtype == np.float32 and X.shape == (4, 3)
    exp = np.stack([x1[:, 0], x2[:, 1], Pa[0, 3] + Pb[1, 3] + np.arange(4)], 1).astype(np.float32)
    assert np.array_equal(X, exp)
    for nout in (2, 3):
        with pytest.raises(mexshim.MexError) as e:
            mex.call("triangulate", x1, x2, Pa, Pb, nout=nout)
        assert e.value.ident == "vo:triangulate:unavailable"
    assert np.array_equal(mex.call("triangulate", x1, x2, Pa, Pb), X)
