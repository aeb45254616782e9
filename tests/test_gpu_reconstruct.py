"""GPU: reconstructScene through libvo.so (vo_reconstruct_scene; k_reconstruct) against tests/sgm_ref, the CPU build
of include/vo_spec.h's vo_reconstruct_point: xyz equal by bytes for a map with NaNs, zeros (h_3 = 0 when both
principal points agree: the point at infinity) and negative disparities, in both storage orders and with a padded
leading dimension; and disparity -> scene chained on one rendered pair."""
import ctypes as C

import numpy as np
import pytest

import sgm_ref as R

pytestmark = pytest.mark.gpu


def _map(rows, cols):
    rng = np.random.default_rng(11)
    d = (rng.integers(-40, 400, (rows, cols)) / 8.0).astype(np.float32)        # eighths of a pixel, negative ones too
    d[rng.random((rows, cols)) < 0.1] = np.nan
    d[rng.random((rows, cols)) < 0.1] = 0.0
    d[0, 0], d[rows - 1, cols - 1], d[1, 2] = 0.0, np.nan, -3.25
    return d


def test_xyz_equals_the_reference_by_bytes_in_both_orders(vo, syn):
    rows, cols = 37, 53
    P0, P1 = syn.calib(0.25)                                                   # cx1 = cx2, neither an integer
    Q = vo.reprojection_matrix(P0, P1)
    assert Q[3, 3] == 0.0
    P1s = P1.copy(); P1s[0, 2] -= 3.5                                          # and a pair whose principal points differ
    d = _map(rows, cols)
    ctx = vo.Context(rows, cols, 1, sift=vo.default_sift_params(64))
    try:
        for q in (Q, vo.reprojection_matrix(P0, P1s), np.arange(1.0, 17.0).reshape(4, 4) / 7.0):
            exp = R.reconstruct(d, q)
            got = ctx.reconstruct_scene(d, q)
            assert got.dtype == np.float32 and got.shape == (rows, cols, 3) and got.flags.c_contiguous
            assert got.tobytes() == exp.tobytes()
            F = ctx.reconstruct_scene(np.asfortranarray(d), q)                 # MATLAB's rows x cols x 3
            assert F.flags.f_contiguous and F.tobytes(order="F") == R.reconstruct(np.asfortranarray(d), q).tobytes(order="F")
            assert np.array_equal(F, exp, equal_nan=True)
        exp = R.reconstruct(d, Q)
        assert (exp[np.isnan(d)].view(np.uint32) == R.NAN_BITS).all()
        assert np.isinf(exp[d == 0.0][:, 2]).all()                             # h_3 = 0: what IEEE gives
        assert (exp[d < 0.0][:, 2] < 0.0).all()                                # behind the camera, unclamped
        # padded leading dimensions, both orders
        PF = C.POINTER(C.c_float)
        q = np.ascontiguousarray(Q.reshape(-1))
        for cm in (0, 1):
            major, minor = (rows, cols) if cm else (cols, rows)
            buf = np.full((minor, major + 6), np.float32(123.0))
            buf[:, :major] = d.T if cm else d
            out = np.zeros(3 * rows * cols, np.float32)
            assert ctx.lib.vo_reconstruct_scene(ctx.h, buf.ctypes.data_as(PF), rows, cols, major + 6, cm,
                                                q.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(PF)) == vo.VO_OK
            ref = R.reconstruct(np.asfortranarray(d) if cm else d, Q)
            assert out.tobytes() == ref.tobytes(order="F" if cm else "C"), cm
        # refusals
        assert ctx.lib.vo_reconstruct_scene(ctx.h, buf.ctypes.data_as(PF), rows, cols, cols - 1, 0, q.ctypes.data_as(C.POINTER(C.c_double)),
                                            out.ctypes.data_as(PF)) == vo.VO_ERR_ARG
        assert ctx.lib.vo_reconstruct_scene(ctx.h, buf.ctypes.data_as(PF), rows + 1, cols, cols, 0, q.ctypes.data_as(C.POINTER(C.c_double)),
                                            out.ctypes.data_as(PF)) == vo.VO_ERR_ARG
        assert ctx.lib.vo_reconstruct_scene(ctx.h, buf.ctypes.data_as(PF), rows, cols, cols, 0, None, out.ctypes.data_as(PF)) == vo.VO_ERR_ARG
        with pytest.raises(vo.VOError):
            ctx.reconstruct_scene(d[:-1], Q)
    finally:
        ctx.close()


def test_disparity_to_scene_on_a_rendered_pair(vo, syn):
    """94 x 310 at calib(0.25): the device's map and scene equal the reference's by bytes, and the reliable points lie
    at the depths of the scene's planes (5 .. 120 m)."""
    scale, rows, cols, D = 0.25, 94, 310, 32
    P0, P1 = syn.calib(scale)
    K = P0[:, :3]
    planes = syn.random_scene(1, rows, cols, f=K[0, 0], px_per_cell=16.0 * scale)
    rng = np.random.default_rng(1 ^ 0xABCDEF)
    left = syn._to_u8(syn._render(planes, np.eye(3), np.zeros(3), rows, cols, K), rng, 2.0)
    right = syn._to_u8(syn._render(planes, np.eye(3), np.array([syn.baseline_m(), 0.0, 0.0]), rows, cols, K), rng, 2.0)
    Q = vo.reprojection_matrix(P0, P1)
    ref = R.disparity(left, right, 0, D)
    ctx = vo.Context(rows, cols, 1, sift=vo.default_sift_params(64))
    try:
        disp = ctx.disparity_sgm(left, right, vo.default_sgm_params(disparity_range=(0, D)))
        assert disp.tobytes() == ref["disp"].tobytes()
        assert ctx.fetch_sgm_cost(0, D).tobytes() == ref["S"].tobytes()
        xyz = ctx.reconstruct_scene(disp, Q)
        assert xyz.tobytes() == R.reconstruct(ref["disp"], Q).tobytes()
        ok = ~np.isnan(disp) & (disp > 0.5)
        assert ok.mean() > 0.8
        z = xyz[ok][:, 2]
        assert np.isfinite(z).all() and z.min() > 4.0 and np.median(z) < 130.0
        assert np.isnan(xyz[np.isnan(disp)]).all()
    finally:
        ctx.close()
