"""The MEX gateway's `undistort` and `distortion` commands (matlab/vo_mex.c, matlab/undistortImage.m)
linked to the real libvo on the GPU: the column-major uint8 frame as MATLAB holds it, MATLAB's
1-based PrincipalPoint, against kitti.undistort and the ctypes path -- bit for bit (VO.m:75-76)."""
import numpy as np
import pytest

import mexshim

pytestmark = pytest.mark.gpu

ROWS, COLS = 375, 1242
F = 718.856 * COLS / 1242
CX, CY = 0.489 * COLS, 0.493 * ROWS
LEFT = (-0.28, 0.07, 0.001, -0.0007, 0.0)                      # kitti.undistort order k1 k2 p1 p2 k3
RIGHT = (0.21, -0.03, 0.0, 0.0, 0.01)


def cam_row(dist):
    """[fx fy cx cy skew k1 k2 k3 p1 p2] with MATLAB's PrincipalPoint = (cx + 1, cy + 1)"""
    return np.array([[F, 1.003 * F, CX + 1.0, CY + 1.0, 0.0, dist[0], dist[1], dist[4], dist[2], dist[3]]])


def K0():
    """what the gateway hands to libvo: PrincipalPoint - 1"""
    return np.array([[F, 0.0, (CX + 1.0) - 1.0], [0.0, 1.003 * F, (CY + 1.0) - 1.0], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def mex(vo):
    vo.load_library()                    # torch, then libvo: one HIP runtime in the process
    m = mexshim.Mex(mexshim.REAL)
    yield m
    m.call("distortion", np.zeros((0, 0)), np.zeros((0, 0)), nout=0)   # the session's cameras: none again
    m.at_exit()


@pytest.fixture(scope="module")
def kitti():
    from r7020e_visual_odometry_amd import kitti as k
    return k


def test_mex_undistort_column_major_frame(mex, kitti):
    img = np.random.default_rng(11).integers(0, 256, (ROWS, COLS), dtype=np.uint8)
    for dist in (LEFT, RIGHT):
        J = mex.call("undistort", img, cam_row(dist))
        assert J.dtype == np.uint8 and J.shape == img.shape
        assert np.array_equal(J, kitti.undistort(img, K0(), dist))
    J = mex.call("undistort", img, cam_row(RIGHT), "linear", "OutputView", "same", "FillValues", np.float64(0.0))
    assert np.array_equal(J, kitti.undistort(img, K0(), RIGHT))
    with pytest.raises(mexshim.MexError, match="vo:undistortImage:options"):
        mex.call("undistort", img, cam_row(RIGHT), "OutputView", "full")
    bad = cam_row(RIGHT)
    bad[0, 0] = 0.0                                               # fx = 0: libvo's VO_ERR_ARG
    with pytest.raises(mexshim.MexError, match="vo:badArgument"):
        mex.call("undistort", img, bad)


def test_mex_distortion_then_step(mex, vo, syn):
    L, R, _ = syn.sequence(3)
    P1, P2 = syn.KITTI00_P0, syn.KITTI00_P1
    ctx = vo.Context(ROWS, COLS, 3, calib=vo.calib_from(P1, P2))
    ctx.set_distortion(vo.distortion_from_kitti(K0(), LEFT), vo.distortion_from_kitti(K0(), RIGHT))
    ref = ctx.step_batch(L, R)
    lm = ctx.get_landmarks()
    ctx.close()
    assert (ref["n_stereo"] >= 100).all()
    mex.call("close", nout=0)                                     # the next step creates its context anew
    mex.call("distortion", cam_row(LEFT), cam_row(RIGHT), nout=0)
    for f in range(len(L)):
        rel, A, st, nl = mex.call("step", L[f], R[f], P1, P2, nout=4)
        assert st[0, 0] == ref["status"][f] and nl[0, 0] == ref["n_landmarks"][f]
        assert np.array_equal(rel, ref["rel_pose"][f]) and np.array_equal(A, ref["pose"][f])
    assert np.array_equal(mex.call("landmarks_all"), lm)
    # set on the live context too, and cleared again: the plain loop body
    mex.call("reset", nout=0)
    mex.call("distortion", np.zeros((0, 0)), np.zeros((0, 0)), nout=0)
    plain = vo.Context(ROWS, COLS, 1, calib=vo.calib_from(P1, P2))
    for f in (0, 1):
        o = plain.step(L[f], R[f])
        rel, A, st, nl = mex.call("step", L[f], R[f], P1, P2, nout=4)
        assert nl[0, 0] == o["n_landmarks"] and np.array_equal(A, o["pose"]) and np.array_equal(rel, o["rel_pose"])
    assert not np.array_equal(o["pose"], ref["pose"][1])          # (the distorted run differed)
    plain.close()
