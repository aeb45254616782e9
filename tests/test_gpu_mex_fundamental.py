"""[F, inliersIndex, status] = vo_mex('fundamental', matchedPoints1, matchedPoints2, opts) through the
real gateway (matlab/vo_mex.c built against tests/mex_shim's mx-API, linked to the real libvo): MATLAB
column-major inputs, the outputs in MATLAB's classes and shapes, against tests/fund_ref.  The shim
counts leaked mxMalloc blocks and arrays on every call.  The weak reference's "unavailable" path runs
against the recording fake libvo, which has no vo_est_fundamental."""
import numpy as np
import pytest

import fund_ref as R
import mexshim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex(vo):
    vo.load_library()                    # torch, then libvo: one HIP runtime in the process
    m = mexshim.Mex(mexshim.REAL)
    yield m
    m.at_exit()


def test_mex_fundamental_outputs(mex):
    x1, x2, bad = R.case(129, "general", 0.1, 0.3, 4)
    exp = R.estimate(x1, x2, 0, distance_threshold=0.1)
    opts = np.array([[1.0, 500.0, 0.1, 99.0]])
    F, inl, status = mex.call("fundamental", x1, x2, opts, nout=3)
    assert F.dtype == np.float64 and F.shape == (3, 3) and inl.dtype == np.bool_ and inl.shape == (129, 1)
    assert status.dtype == np.int32 and status.shape == (1, 1) and status[0, 0] == 0 and exp["status"] == R.OK
    assert F.tobytes() == exp["F"].tobytes()                      # F(i, j) is the row-major F[3 i + j]
    assert np.array_equal(inl[:, 0], exp["inliers"]) and not inl[bad, 0].any()
    # column-major (Fortran) inputs, double points (rounded to single by the gateway), fewer outputs
    Fd, inld = mex.call("fundamental", np.asfortranarray(x1.astype(np.float64)), np.asfortranarray(x2.astype(np.float64)), opts, nout=2)
    assert Fd.tobytes() == F.tobytes() and np.array_equal(inld, inl)
    assert mex.call("fundamental", x1, x2, opts).tobytes() == F.tobytes()
    # the defaults (DistanceThreshold 0.01) and Norm8Point over the planted rows
    Fdef, _, sdef = mex.call("fundamental", x1, x2, nout=3)
    edef = R.estimate(x1, x2, 0)
    assert Fdef.tobytes() == edef["F"].tobytes() and sdef[0, 0] == {R.OK: 0, R.NO_CONSENSUS: 2}[edef["status"]]
    F8, inl8, s8 = mex.call("fundamental", x1[~bad], x2[~bad], np.array([[0.0, 500.0, 0.01, 99.0]]), nout=3)
    assert s8[0, 0] == 0 and inl8.all() and F8.tobytes() == R.norm8(x1[~bad], x2[~bad])[1].tobytes()
    # the two failures as status, with zeros(3) and an all-false column
    F1, i1, s1 = mex.call("fundamental", x1[:7], x2[:7], nout=3)
    assert s1[0, 0] == 1 and not F1.any() and i1.shape == (7, 1) and not i1.any()
    F2, i2, s2 = mex.call("fundamental", x1, x2, np.array([[1.0, 2.0, 1e-12, 99.0]]), nout=3)
    assert s2[0, 0] == 2 and not F2.any() and i2.shape == (129, 1) and not i2.any()
    F0, i0, s0 = mex.call("fundamental", np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), nout=3)
    assert s0[0, 0] == 1 and i0.shape == (0, 1) and i0.dtype == np.bool_


def test_mex_fundamental_refusals(mex):
    x1, x2, _ = R.case(20, "general", 0.1, 0.0, 1)
    with pytest.raises(mexshim.MexError) as e:                    # without the status output the failures are errors
        mex.call("fundamental", x1[:7], x2[:7], nout=2)
    assert e.value.ident == "vision:estimateFundamentalMatrix:notEnoughPts"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("fundamental", x1, x2, np.array([[1.0, 2.0, 1e-12, 99.0]]))
    assert e.value.ident == "vision:estimateFundamentalMatrix:notEnoughInliers"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("fundamental", x1, x2[:19])
    assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("fundamental", x1.astype(np.int32), x2)
    assert e.value.ident == "vo:badArgument"
    bad = x2.copy()
    bad[3, 0] = np.nan
    with pytest.raises(mexshim.MexError) as e:
        mex.call("fundamental", x1, bad)
    assert e.value.ident == "vo:badArgument" and "index 3" in str(e.value)
    for opts in ([[2.0, 500.0, 0.01, 99.0]], [[0.5, 500.0, 0.01, 99.0]], [[1.0, 0.0, 0.01, 99.0]], [[1.0, 2.5, 0.01, 99.0]],
                 [[1.0, 500.0, 0.0, 99.0]], [[1.0, 500.0, 0.01, 100.0]]):
        with pytest.raises(mexshim.MexError) as e:
            mex.call("fundamental", x1, x2, np.array(opts))
        assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("fundamental", x1, x2, np.array([[1.0, 500.0, 0.01]]))
    assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("fundamental", x1)
    assert e.value.ident == "vo:nargin"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("fundamental", x1, x2, nout=4)
    assert e.value.ident == "vo:badArgument"


def test_mex_fundamental_is_unavailable_without_the_entry():
    fake = mexshim.Mex(mexshim.FAKE)
    try:
        x = np.zeros((9, 2), np.float32)
        with pytest.raises(mexshim.MexError) as e:
            fake.call("fundamental", x, x, nout=3)
        assert e.value.ident == "vo:estimateFundamentalMatrix:unavailable"
    finally:
        fake.at_exit()
