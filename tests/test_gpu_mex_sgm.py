"""disparityMap = vo_mex('disparitysgm', I1, I2, opts) and xyz = vo_mex('reconstructscene', disparityMap, Q) through
the real gateway (matlab/vo_mex.c built against tests/mex_shim's mx-API, linked to the real libvo): MATLAB
column-major images and maps, the outputs in MATLAB's classes and shapes, equal to the ctypes calls and to
tests/sgm_ref by bytes.  The shim counts leaked mxMalloc blocks and arrays on every call."""
import numpy as np
import pytest

import mexshim
import sgm_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex(vo):
    vo.load_library()                    # torch, then libvo: one HIP runtime in the process
    m = mexshim.Mex(mexshim.REAL)
    yield m
    m.at_exit()


def test_mex_sgm_and_scene_equal_the_ctypes_calls(vo, mex, syn):
    rows, cols = 37, 53
    ctx = vo.Context(rows, cols, 1, sift=vo.default_sift_params(64))
    Q = vo.reprojection_matrix(*syn.calib(0.25))
    try:
        for opts, (dmin, D, U, P1, P2) in (([[-4.0, 12.0, 15.0]], (-4, 16, 15, 10, 120)), ([[0.0, 32.0, 40.0, 5.0, 60.0]], (0, 32, 40, 5, 60)),
                                           (None, (0, 128, 15, 10, 120))):
            left, right = (np.asfortranarray(a) for a in R.pair("step", rows, cols, -4, 16))
            exp = R.disparity(left, right, dmin, D, P1, P2, U)["disp"]
            p = vo.default_sgm_params(disparity_range=(dmin, dmin + D), uniqueness_threshold=U, p1=P1, p2=P2)
            c_disp = ctx.disparity_sgm(left, right, p)
            args = (left, right) + (() if opts is None else (np.array(opts, np.float64),))
            m_disp = mex.call("disparitysgm", *args)
            assert m_disp.dtype == np.float32 and m_disp.shape == (rows, cols)
            assert np.ascontiguousarray(m_disp).tobytes() == np.ascontiguousarray(c_disp).tobytes() == exp.tobytes()
            m_xyz = mex.call("reconstructscene", np.asfortranarray(m_disp), Q)
            assert m_xyz.dtype == np.float32 and m_xyz.shape == (rows, 3 * cols)
            ref = R.reconstruct(exp, Q)                                         # [rows, cols, 3]
            c_xyz = ctx.reconstruct_scene(np.asfortranarray(exp), Q)
            for k in range(3):                                                  # MATLAB's planes side by side
                assert np.ascontiguousarray(m_xyz[:, k * cols:(k + 1) * cols]).tobytes() == np.ascontiguousarray(ref[:, :, k]).tobytes()
                assert np.ascontiguousarray(c_xyz[:, :, k]).tobytes() == np.ascontiguousarray(ref[:, :, k]).tobytes()
    finally:
        ctx.close()


def test_mex_sgm_refusals(mex):
    rows, cols = 37, 53
    left, right = (np.asfortranarray(a) for a in R.pair("texture", rows, cols, -4, 16))
    for opts in ([[0.0, 12.0, 15.0]], [[0.0, 136.0, 15.0]], [[8.0, 8.0, 15.0]], [[0.0, 16.5, 15.0]], [[0.0, 16.0, 101.0]],
                 [[0.0, 16.0, np.nan]], [[0.0, 16.0, 15.0, -1.0, 120.0]], [[0.0, 16.0, 15.0, 20.0, 10.0]], [[0.0, 16.0, 15.0, 10.0, 256.0]]):
        with pytest.raises(mexshim.MexError) as e:
            mex.call("disparitysgm", left, right, np.array(opts, np.float64))
        assert e.value.ident == "vo:badArgument", opts
    with pytest.raises(mexshim.MexError) as e:
        mex.call("disparitysgm", left, right.astype(np.float32))
    assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("reconstructscene", np.zeros((rows, cols), np.float32, order="F"), np.eye(3))
    assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("disparitysgm", left)
    assert e.value.ident == "vo:nargin"
