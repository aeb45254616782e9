"""[refinedPose, reprojectionErrors] = vo_mex('refinepose', xyzPoints, imagePoints, A, K, opts)
through the real gateway (matlab/vo_mex.c built against tests/mex_shim's mx-API, linked to the real
libvo): MATLAB column-major inputs, the outputs in MATLAB's classes and shapes, against
Context.refine_pose and tests/pose_refine_ref.  The shim counts leaked mxMalloc blocks and arrays on
every call."""
import numpy as np
import pytest

import geom_ref as G
import mexshim
import pose_refine_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex(vo):
    vo.load_library()                    # torch, then libvo: one HIP runtime in the process
    m = mexshim.Mex(mexshim.REAL)
    yield m
    m.at_exit()


def _problem():
    rng = np.random.default_rng(0x3E8)
    uv, Xw, K = G.pose_problem(rng, 150, 0.0, noise=0.2)
    return uv, Xw, K, P.start_pose(rng, 0.5, 0.1)


def test_mex_refinepose_outputs(mex, vo):
    uv, Xw, K, T0 = _problem()
    n = len(uv)
    ctx = vo.Context(64, 64, 1)
    try:
        T, st = ctx.refine_pose(uv, Xw, T0, K)
        T5, st5 = ctx.refine_pose(uv, Xw, T0, K, params=vo.default_refine_params(max_iterations=3, absolute_tolerance=0.5,
                                                                                 relative_tolerance=1e-4))
    finally:
        ctx.close()
    Tr, sr = P.refine(uv, Xw, T0, K)
    assert T.tobytes() == Tr.tobytes() and st.tobytes() == sr.tobytes() and st["accepted"] > 0
    A, err = mex.call("refinepose", Xw, uv, T0, K, nout=2)
    assert A.dtype == np.float64 and A.shape == (4, 4) and err.dtype == np.float64 and err.shape == (n, 1)
    assert A.tobytes() == T.tobytes()
    # each point's pixel distance at the refined pose: sqrt of the terms of cost_final
    R, t = P.from_T(A)
    d = np.linalg.norm(G.project(K, R, t, Xw) - uv, axis=1)
    assert np.abs(err[:, 0] - d).max() <= 1e-9
    assert abs((err ** 2).sum() - st["cost_final"]) <= 1e-9 * st["cost_final"]
    # one output, and the options [MaxIterations AbsoluteTolerance RelativeTolerance]
    A1 = mex.call("refinepose", Xw, uv, T0, K)
    assert A1.tobytes() == A.tobytes()
    A5 = mex.call("refinepose", Xw, uv, T0, K, np.array([[3.0, 0.5, 1e-4]]))
    assert A5.tobytes() == T5.tobytes() and st5["passes"] <= 3
    # no points: the input pose and an empty error column
    A0, e0 = mex.call("refinepose", np.zeros((0, 3)), np.zeros((0, 2)), T0, K, nout=2)
    assert A0.tobytes() == T0.tobytes() and e0.shape == (0, 1) and e0.dtype == np.float64


def test_mex_refinepose_refusals(mex):
    uv, Xw, K, T0 = _problem()
    with pytest.raises(mexshim.MexError) as e:
        mex.call("refinepose", Xw, uv[:7], T0, K)
    assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("refinepose", Xw, uv, T0[:3], K)
    assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("refinepose", Xw.astype(np.float32), uv, T0, K)
    assert e.value.ident == "vo:badArgument"
    bad = uv.copy()
    bad[3, 0] = np.nan
    with pytest.raises(mexshim.MexError) as e:
        mex.call("refinepose", Xw, bad, T0, K)
    assert e.value.ident == "vo:badArgument" and "index 3" in str(e.value)
    for opts in ([[0.0, 0.0, 1e-9]], [[2.5, 0.0, 1e-9]], [[20.0, -1.0, 1e-9]]):
        with pytest.raises(mexshim.MexError) as e:
            mex.call("refinepose", Xw, uv, T0, K, np.array(opts))
        assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("refinepose", Xw, uv, T0)
    assert e.value.ident == "vo:nargin"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("refinepose", Xw, uv, T0, K, nout=3)
    assert e.value.ident == "vo:badArgument"
