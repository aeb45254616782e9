"""[worldPoints, reprojectionErrors, validIndex] = vo_mex('triangulate', x1, x2, P1, P2) through the
real gateway (matlab/vo_mex.c built against tests/mex_shim's mx-API, linked to the real libvo):
MATLAB column-major inputs, the three outputs in MATLAB's classes and shapes, against
Context.triangulate(..., quality=True) and tests/tri_quality_ref.  The shim counts leaked mxMalloc
blocks and arrays on every call."""
import numpy as np
import pytest

import geom_ref as G
import mexshim
import tri_quality_ref as T

pytestmark = pytest.mark.gpu

P1, P2 = G.KITTI_P1, G.KITTI_P2


@pytest.fixture(scope="module")
def mex(vo):
    vo.load_library()                    # torch, then libvo: one HIP runtime in the process
    m = mexshim.Mex(mexshim.REAL)
    yield m
    m.at_exit()


def _points():
    l, r = G.stereo_rows(np.random.default_rng(0x3E7), 300, 2.0, 300.0)
    r[::7, 0] = l[::7, 0] + np.float32(2.5)               # negative disparity: behind the cameras
    r[::5, 1] += np.float32(0.75)                         # row offsets: errors up to 0.4 px
    return np.vstack([l, T.PROBE_X1]), np.vstack([r, T.PROBE_X2])


def test_mex_triangulate_three_outputs(mex, vo, oracle):
    x1, x2 = _points()
    n = len(x1)
    ctx = vo.Context(64, 64, 1)
    try:
        X, err, valid = ctx.triangulate(x1, x2, P1, P2, quality=True)
    finally:
        ctx.close()
    rerr, rvalid = T.quality(x1, x2, X, P1, P2)
    assert err.tobytes() == rerr.tobytes() and np.array_equal(valid, rvalid)
    assert (~valid).sum() >= n // 7 and valid.sum() > n // 2 and err.max() > 0.2
    Xm, em, vm = mex.call("triangulate", x1, x2, P1, P2, nout=3)
    assert Xm.dtype == np.float32 and Xm.shape == (n, 3)
    assert em.dtype == np.float32 and em.shape == (n, 1)
    assert vm.dtype == np.bool_ and vm.shape == (n, 1)
    assert Xm.tobytes() == X.astype(np.float32).tobytes()
    assert em[:, 0].tobytes() == err.tobytes()
    assert np.array_equal(vm[:, 0], valid)
    # two outputs: the same errors (the gateway passes valid = NULL)
    X2, e2 = mex.call("triangulate", x1, x2, P1, P2, nout=2)
    assert X2.tobytes() == Xm.tobytes() and e2.tobytes() == em.tobytes()
    # one output is unchanged: vo_triangulate, the oracle's points as single
    X1 = mex.call("triangulate", x1, x2, P1, P2)
    assert X1.dtype == np.float32 and np.array_equal(X1, oracle.triangulate(x1, x2, P1, P2).astype(np.float32))
    assert X1.tobytes() == Xm.tobytes()
    # double points (MATLAB's double Location) are rounded to single first
    Xd, ed, vd = mex.call("triangulate", x1.astype(np.float64), x2.astype(np.float64), P1, P2, nout=3)
    assert Xd.tobytes() == Xm.tobytes() and ed.tobytes() == em.tobytes() and np.array_equal(vd, vm)
    # no points: empty outputs of the right classes
    z = np.zeros((0, 2), np.float32)
    X0, e0, v0 = mex.call("triangulate", z, z, P1, P2, nout=3)
    assert X0.shape == (0, 3) and e0.shape == (0, 1) and v0.shape == (0, 1)


def test_mex_triangulate_refusals(mex):
    x1, x2 = _points()
    for nout in (1, 3):
        with pytest.raises(mexshim.MexError) as e:
            mex.call("triangulate", x1, x2[:3], P1, P2, nout=nout)
        assert e.value.ident == "vo:badArgument"
        with pytest.raises(mexshim.MexError) as e:
            mex.call("triangulate", x1, x2, P1[:, :3], P2, nout=nout)
        assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("triangulate", x1, x2, P1, nout=3)
    assert e.value.ident == "vo:nargin"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("triangulate", x1, x2, P1, P2, nout=4)
    assert e.value.ident == "vo:badArgument"
