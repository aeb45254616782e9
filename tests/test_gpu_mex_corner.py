"""[Location, Metric] = vo_mex('corners', I, opts) through the real gateway (matlab/vo_mex.c built against
tests/mex_shim's mx-API, linked to the real libvo): a MATLAB column-major image, the outputs in MATLAB's classes
and shapes, equal to the ctypes call and to tests/corner_ref by bytes.  The shim counts leaked mxMalloc blocks
and arrays on every call."""
import numpy as np
import pytest

import corner_ref as R
import mexshim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex(vo):
    vo.load_library()                    # torch, then libvo: one HIP runtime in the process
    m = mexshim.Mex(mexshim.REAL)
    yield m
    m.at_exit()


def test_mex_corners_equals_the_ctypes_call(vo, mex):
    img = np.asfortranarray(R.image("b:noise"))          # 37 x 53, column-major as MATLAB holds it
    rows, cols = img.shape
    ctx = vo.Context(rows, cols, 1)
    try:
        for opts, kw in ((None, {}), ([[1.0, 7.0, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0]], dict(method=R.HARRIS, f=7, min_quality=0.05)),
                         ([[0.0, 3.0, 0.0, 9.0, 5.0, 4.0, 30.0, 20.0]], dict(f=3, min_quality=0.0, strongest=9, roi=(5, 4, 30, 20)))):
            exp = R.detect(img, max_keypoints=16384, **kw)
            p = vo.default_corner_params(method=kw.get("method", 0), filter_size=kw.get("f", 5), min_quality=kw.get("min_quality", 0.01),
                                         strongest=kw.get("strongest", 0), roi=kw.get("roi"))
            c_loc, c_met = ctx.detect_corners(img, p)
            args = (img,) + (() if opts is None else (np.array(opts, np.float64),))
            m_loc, m_met = mex.call("corners", *args, nout=2)
            n = exp["count"]
            assert n > 0 and m_loc.dtype == np.float32 and m_loc.shape == (n, 2) and m_met.dtype == np.float32 and m_met.shape == (n, 1)
            assert np.ascontiguousarray(m_loc).tobytes() == c_loc.tobytes() == exp["loc"].tobytes()
            assert np.ascontiguousarray(m_met[:, 0]).tobytes() == c_met.tobytes() == exp["metric"].tobytes()
        only = mex.call("corners", img)                  # one output
        assert np.ascontiguousarray(only).tobytes() == R.detect(img)["loc"].tobytes()
        e_loc, e_met = mex.call("corners", np.asfortranarray(R.image("b:flat")), nout=2)
        assert e_loc.shape == (0, 2) and e_met.shape == (0, 1)
    finally:
        ctx.close()


def test_mex_corners_refusals(mex):
    img = np.asfortranarray(R.image("b:noise"))
    with pytest.raises(mexshim.MexError) as e:
        mex.call("corners", img.astype(np.float64))
    assert e.value.ident == "vo:badArgument"
    for opts in ([[2.0, 5, 0.01, 0, 0, 0, 0, 0]], [[0.0, 4, 0.01, 0, 0, 0, 0, 0]], [[0.0, 17, 0.01, 0, 0, 0, 0, 0]],
                 [[0.0, 5.5, 0.01, 0, 0, 0, 0, 0]], [[0.0, 5, 1.5, 0, 0, 0, 0, 0]], [[0.0, 5, np.nan, 0, 0, 0, 0, 0]],
                 [[0.0, 5, 0.01, -1, 0, 0, 0, 0]], [[0.0, 5, 0.01, 0, 1, 1, 54, 5]], [[0.0, 5, 0.01, 0, 0, 1, 5, 5]],
                 [[0.0, 5, 0.01, 0, 1, 1, 5, 0]]):
        with pytest.raises(mexshim.MexError) as e:
            mex.call("corners", img, np.array(opts, np.float64))
        assert e.value.ident == "vo:badArgument", opts
    with pytest.raises(mexshim.MexError) as e:
        mex.call("corners", img, np.array([[0.0, 5.0, 0.01, 0.0]]))
    assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("corners")
    assert e.value.ident == "vo:nargin"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("corners", img, nout=3)
    assert e.value.ident == "vo:badArgument"
