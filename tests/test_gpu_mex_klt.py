"""[points, validity, scores] = vo_mex('trackpoints', I0, I1, points, opts) through the real gateway
(matlab/vo_mex.c built against tests/mex_shim's mx-API, linked to the real libvo): MATLAB column-major
images and points, the outputs in MATLAB's classes and shapes, equal to the ctypes call and to
tests/klt_ref by bytes.  The shim counts leaked mxMalloc blocks and arrays on every call."""
import numpy as np
import pytest

import klt_ref as R
import mexshim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex(vo):
    vo.load_library()                    # torch, then libvo: one HIP runtime in the process
    m = mexshim.Mex(mexshim.REAL)
    yield m
    m.at_exit()


def test_mex_trackpoints_equals_the_ctypes_call(vo, mex):
    img0, img1 = (np.asfortranarray(a) for a in R.images("a:s8"))
    rows, cols = img0.shape
    pts = np.concatenate([R.interior_points(rows, cols, 60, 1), R.side_points(rows, cols, (11, 11))])
    ctx = vo.Context(rows, cols, 1, sift=vo.default_sift_params(512))
    try:
        for opts, kw in ((None, {}), (np.array([[2.0, 11.0, 21.0, 10.0, 0.5]]), dict(levels=2, block=(11, 21), max_it=10, max_bidir=0.5))):
            exp = R.track(img0, img1, pts, **dict(R.DEFAULTS, **kw))
            p = vo.default_klt_params(num_pyramid_levels=kw.get("levels", 3), block_size=kw.get("block", (31, 31)),
                                      max_iterations=kw.get("max_it", 30), max_bidirectional_error=kw.get("max_bidir", float("inf")))
            c_pts, c_ok, c_sc, _ = ctx.track_points(img0, img1, pts, params=p)
            args = (img0, img1, pts) + (() if opts is None else (opts,))
            m_pts, m_ok, m_sc = mex.call("trackpoints", *args, nout=3)
            n = len(pts)
            assert m_pts.dtype == np.float32 and m_pts.shape == (n, 2) and m_ok.dtype == np.bool_ and m_ok.shape == (n, 1)
            assert m_sc.dtype == np.float32 and m_sc.shape == (n, 1)
            assert np.ascontiguousarray(m_pts).tobytes() == c_pts.tobytes() == exp["pts1"].tobytes()
            assert np.array_equal(m_ok[:, 0], c_ok) and np.array_equal(c_ok, exp["valid"]) and not m_ok.all() and m_ok.any()
            assert np.ascontiguousarray(m_sc[:, 0]).tobytes() == c_sc.tobytes() == exp["scores"].tobytes()
        # double points are rounded to single by the gateway; fewer outputs; no points
        d_pts = mex.call("trackpoints", img0, img1, np.asfortranarray(pts.astype(np.float64)))
        assert np.ascontiguousarray(d_pts).tobytes() == R.track(img0, img1, pts)["pts1"].tobytes()
        e_pts, e_ok, e_sc = mex.call("trackpoints", img0, img1, np.zeros((0, 2), np.float32), nout=3)
        assert e_pts.shape == (0, 2) and e_ok.shape == (0, 1) and e_sc.shape == (0, 1)
    finally:
        ctx.close()


def test_mex_trackpoints_refusals(mex):
    img0, img1 = (np.asfortranarray(a) for a in R.images("b:s0"))
    pts = R.interior_points(64, 64, 10, 1, 8.0)
    with pytest.raises(mexshim.MexError) as e:
        mex.call("trackpoints", img0, img1[:-1], pts)
    assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("trackpoints", img0.astype(np.float64), img1, pts)
    assert e.value.ident == "vo:badArgument"
    bad = pts.copy()
    bad[3, 0] = np.nan
    with pytest.raises(mexshim.MexError) as e:
        mex.call("trackpoints", img0, img1, bad)
    assert e.value.ident == "vo:badArgument" and "index 3" in str(e.value)
    for opts in ([[0.0, 31, 31, 30, np.inf]], [[7.0, 31, 31, 30, np.inf]], [[3.0, 30, 31, 30, np.inf]], [[3.0, 31, 33, 30, np.inf]],
                 [[3.0, 31, 31, 0, np.inf]], [[3.0, 31, 31, 2.5, np.inf]], [[3.0, 31, 31, 30, 0.0]], [[3.0, 31, 31, 30, np.nan]]):
        with pytest.raises(mexshim.MexError) as e:
            mex.call("trackpoints", img0, img1, pts, np.array(opts, np.float64))
        assert e.value.ident == "vo:badArgument", opts
    with pytest.raises(mexshim.MexError) as e:
        mex.call("trackpoints", img0, img1, pts, np.array([[3.0, 31.0, 31.0, 30.0]]))
    assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("trackpoints", img0, img1)
    assert e.value.ident == "vo:nargin"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("trackpoints", img0, img1, pts, nout=4)
    assert e.value.ident == "vo:badArgument"
