"""GPU parity of undistortImage (VO.m:75-76) through libvo.so: k_undistort against
kitti.undistort (the spec: Brown-Conrady map in f64, bilinear taps, 0 outside, rint to u8), bit
for bit -- the host entry in both storage orders with padded leading dimensions, the device
batch entry across the frames-per-thread chunk, and vo_set_distortion ahead of the scale space
of the batched SIFT path and of the whole loop body (synchronous and three batches in flight)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# kitti.undistort order: k1, k2, p1, p2, k3
SETS = {
    "barrel": ((-0.28, 0.07, 0.0, 0.0, 0.0), 0.0),
    "pincushion": ((0.21, -0.03, 0.0, 0.0, 0.01), 0.0),
    "tang+skew": ((-0.11, 0.02, 0.004, -0.003, 0.001), 0.7),
    "zero": ((0.0, 0.0, 0.0, 0.0, 0.0), 0.0),
}
SIZES = [(101, 163), (64, 64)]


def cam(rows, cols, skew=0.0):
    f = 718.856 * cols / 1242
    return np.array([[f, skew, 0.489 * cols], [0.0, 1.003 * f, 0.493 * rows], [0.0, 0.0, 1.0]])


def split(dist):
    """kitti order -> (radial, tangential)"""
    return (dist[0], dist[1], dist[4]), (dist[2], dist[3])


@pytest.fixture(scope="module")
def kitti():
    from r7020e_visual_odometry_amd import kitti as k
    return k


@pytest.fixture(scope="module")
def ctxs(vo):
    c = {s: vo.Context(s[0], s[1], 1) for s in SIZES}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def small(kitti):
    """(image, {set: reference}) per size: random u8 (the worst case for the rounding)."""
    out = {}
    for k, (rows, cols) in enumerate(SIZES):
        img = np.random.default_rng(100 + k).integers(0, 256, (rows, cols), dtype=np.uint8)
        out[(rows, cols)] = (img, {n: kitti.undistort(img, cam(rows, cols, s), d) for n, (d, s) in SETS.items()})
    return out


# ---- 1. host entry ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", list(SETS))
def test_host_entry_bit_exact(vo, ctxs, small, size, name):
    rows, cols = size
    img, refs = small[size]
    dist, skew = SETS[name]
    rad, tan = split(dist)
    K = cam(rows, cols, skew)
    ctx = ctxs[size]
    if name == "pincushion":                                  # the fill value is exercised
        assert (refs[name] == 0).mean() > 0.1
    assert np.array_equal(ctx.undistort(img, K, rad, tan), refs[name])
    got_cm = ctx.undistort(img, K, rad, tan, col_major=True)
    assert got_cm.flags.f_contiguous and np.array_equal(got_cm, refs[name])
    if name == "zero":
        assert np.array_equal(refs[name], img) and np.array_equal(got_cm, img)
    # padded leading dimensions, poison in the padding: ld = n + 3 in, n + 5 out
    d = vo.distortion_from(K, rad, tan)
    for col_major in (0, 1):
        lines, n = (cols, rows) if col_major else (rows, cols)    # lines of n pixels
        src = np.full((lines, n + 3), 0xA5, np.uint8)
        src[:, :n] = img.T if col_major else img
        dst = np.full((lines, n + 5), 0x5A, np.uint8)
        rc = ctx.lib.vo_undistort(ctx.h, src.ctypes.data_as(C.POINTER(C.c_uint8)), rows, cols, n + 3, col_major, C.byref(d),
                                  dst.ctypes.data_as(C.POINTER(C.c_uint8)), n + 5)
        assert rc == 0, ctx.lib.vo_last_error(ctx.h)
        got = dst[:, :n].T if col_major else dst[:, :n]
        assert np.array_equal(got, refs[name]), col_major
        assert (dst[:, n:] == 0x5A).all(), col_major


# ---- 2. device batch -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["5", "2chunk+1"])
def test_device_batch_equals_host_entry(vo, ctxs, shape):
    import torch
    chunk = vo.UNDISTORT_CHUNK                                # the kernel's frames per thread (VO_UD_CHUNK)
    B = 5 if shape == "5" else 2 * chunk + 1                  # two full chunks and a tail of one frame
    rows, cols = 101, 163
    ctx = ctxs[(rows, cols)]
    frames = np.random.default_rng(7).integers(0, 256, (B, rows, cols), dtype=np.uint8)
    d_in = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    for name in ("barrel", "pincushion", "tang+skew"):
        dist, skew = SETS[name]
        rad, tan = split(dist)
        K = cam(rows, cols, skew)
        d_out = torch.full((B, rows, cols), 0x77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.undistort_batch_dev(d_in.data_ptr(), d_out.data_ptr(), B, K, rad, tan)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        for f in range(B):
            assert np.array_equal(got[f], ctx.undistort(frames[f], K, rad, tan)), (name, f)


# ---- 3, 4. the loop-body entries ---------------------------------------------------------------
K375 = cam(375, 1242)
LEFT = (-0.28, 0.07, 0.001, -0.0007, 0.0)                      # barrel with a little tangential
RIGHT = SETS["pincushion"][0]


def _dist(vo, d):
    rad, tan = split(d)
    return vo.distortion_from(K375, rad, tan)


def _same_kps(a, b):
    assert len(a) == len(b), (len(a), len(b))
    assert a.tobytes() == b.tobytes()


def test_batched_sift_path(vo, oracle, syn, kitti):
    import torch
    B = 3
    pairs = [syn.stereo_pair(3 + f) for f in range(B)]
    L = np.stack([p[0] for p in pairs])
    R = np.stack([p[1] for p in pairs])
    UL = np.stack([kitti.undistort(x, K375, LEFT) for x in L])
    UR = np.stack([kitti.undistort(x, K375, RIGHT) for x in R])
    dev = [torch.from_numpy(x).cuda() for x in (L, R, UL, UR)]
    torch.cuda.synchronize()
    ctx = vo.Context(375, 1242, B)
    ctx.set_distortion(_dist(vo, LEFT), _dist(vo, RIGHT))
    stats = ctx.sift_match_batch_dev(dev[0].data_ptr(), dev[1].data_ptr(), B)
    for f in range(B):
        assert np.array_equal(ctx.fetch_rectified(2 * f), UL[f]), f
        assert np.array_equal(ctx.fetch_rectified(2 * f + 1), UR[f]), f
        assert stats[f][2] >= 100, stats[f]
    ref = vo.Context(375, 1242, B)                            # no distortion, host-undistorted frames
    rstats = ref.sift_match_batch_dev(dev[2].data_ptr(), dev[3].data_ptr(), B)
    assert stats == rstats
    for f in (0, 1):
        for i in (2 * f, 2 * f + 1):
            (k, d), (rk, rd) = ctx.fetch_keypoints(i), ref.fetch_keypoints(i)
            _same_kps(k, rk)
            assert np.array_equal(d, rd)
        assert np.array_equal(ctx.fetch_stereo_pairs(f), ref.fetch_stereo_pairs(f))
    okl, odl = oracle.sift(UL[2])
    okr, odr = oracle.sift(UR[2])
    (kl, dl), (kr, dr) = ctx.fetch_keypoints(4), ctx.fetch_keypoints(5)
    _same_kps(kl, okl)
    _same_kps(kr, okr)
    assert np.array_equal(dl, odl) and np.array_equal(dr, odr)
    assert np.array_equal(ctx.fetch_stereo_pairs(2), oracle.match(odl, odr))
    ctx.close()
    ref.close()


@pytest.fixture(scope="module")
def seq(syn, kitti):
    L, R, _ = syn.sequence(6)
    UL = np.stack([kitti.undistort(x, K375, LEFT) for x in L])
    UR = np.stack([kitti.undistort(x, K375, RIGHT) for x in R])
    return L, R, UL, UR


@pytest.fixture(scope="module")
def seq_ref(vo, syn, seq):
    """The loop body of a context that never set a distortion, fed the host-undistorted frames."""
    _, _, UL, UR = seq
    ctx = vo.Context(375, 1242, 3, calib=vo.calib_from(syn.KITTI00_P0, syn.KITTI00_P1))
    outs = np.concatenate([ctx.step_batch(UL[0:3], UR[0:3]), ctx.step_batch(UL[3:6], UR[3:6])])
    lm = ctx.get_landmarks()
    ctx.close()
    assert (outs["n_stereo"] >= 100).all(), outs["n_stereo"]
    return outs, lm


def _same_steps(outs, lm, ref):
    routs, rlm = ref
    assert outs.tobytes() == routs.tobytes()                  # every vo_step_out field
    assert np.array_equal(lm, rlm)


def test_full_path_step_batch(vo, syn, seq, seq_ref):
    L, R, _, _ = seq
    ctx = vo.Context(375, 1242, 3, calib=vo.calib_from(syn.KITTI00_P0, syn.KITTI00_P1))
    ctx.set_distortion(_dist(vo, LEFT), _dist(vo, RIGHT))
    outs = np.concatenate([ctx.step_batch(L[0:3], R[0:3]), ctx.step_batch(L[3:6], R[3:6])])
    _same_steps(outs, ctx.get_landmarks(), seq_ref)
    ctx.close()


def test_full_path_three_batches_in_flight(vo, syn, seq, seq_ref):
    """2 frames per submit, three batches pending before the first collect: every batch's
    pre-pass writes the one rectified buffer while earlier batches are still running."""
    import torch
    L, R, _, _ = seq
    dl, dr = torch.from_numpy(np.ascontiguousarray(L)).cuda(), torch.from_numpy(np.ascontiguousarray(R)).cuda()
    torch.cuda.synchronize()
    fs = L[0].size
    ctx = vo.Context(375, 1242, 2, calib=vo.calib_from(syn.KITTI00_P0, syn.KITTI00_P1))
    ctx.set_distortion(_dist(vo, LEFT), _dist(vo, RIGHT))
    for a in (0, 2, 4):
        ctx.step_submit_dev(dl.data_ptr() + a * fs, dr.data_ptr() + a * fs, 2)
    assert ctx.steps_pending() == 3
    with pytest.raises(vo.VOError) as e:                      # 5. state: refused while batches are pending
        ctx.set_distortion(None, None)
    assert e.value.code == vo.VO_ERR_STATE
    outs = np.concatenate([ctx.step_collect() for _ in range(3)])
    _same_steps(outs, ctx.get_landmarks(), seq_ref)
    ctx.close()


# ---- 5. state ------------------------------------------------------------------------------------
def test_clearing_the_distortion_restores_the_plain_path(vo, syn, seq):
    import torch
    L, R, _, _ = seq
    dl, dr = torch.from_numpy(L[:2].copy()).cuda(), torch.from_numpy(R[:2].copy()).cuda()
    torch.cuda.synchronize()
    ctx = vo.Context(375, 1242, 2)
    with pytest.raises(vo.VOError) as e:
        ctx.fetch_rectified(0)
    assert e.value.code == vo.VO_ERR_STATE
    ctx.set_distortion(_dist(vo, LEFT), None)                 # the right camera passes through
    s1 = ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), 2)
    assert np.array_equal(ctx.fetch_rectified(1), R[0]) and np.array_equal(ctx.fetch_rectified(3), R[1])
    assert not np.array_equal(ctx.fetch_rectified(0), L[0])
    ctx.set_distortion(None, None)
    with pytest.raises(vo.VOError) as e:
        ctx.fetch_rectified(0)
    assert e.value.code == vo.VO_ERR_STATE
    s2 = ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), 2)
    got = [ctx.fetch_keypoints(i) for i in range(4)] + [ctx.fetch_stereo_pairs(f) for f in range(2)]
    ref = vo.Context(375, 1242, 2)                            # never set
    s3 = ref.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), 2)
    exp = [ref.fetch_keypoints(i) for i in range(4)] + [ref.fetch_stereo_pairs(f) for f in range(2)]
    assert s2 == s3 and s1 != s2
    for g, x in zip(got, exp):
        if isinstance(g, tuple):
            assert g[0].tobytes() == x[0].tobytes() and np.array_equal(g[1], x[1])
        else:
            assert np.array_equal(g, x)
    # an all-zero side is a pass-through too: nothing is set
    ctx.set_distortion(_dist(vo, SETS["zero"][0]), None)
    with pytest.raises(vo.VOError):
        ctx.fetch_rectified(0)
    ctx.close()
    ref.close()


# ---- 6. arguments --------------------------------------------------------------------------------
def test_bad_arguments(vo, ctxs):
    import torch
    rows, cols = 64, 64
    ctx = ctxs[(rows, cols)]
    img = np.zeros((rows, cols), np.uint8)
    K = cam(rows, cols)
    rad, tan = split(SETS["barrel"][0])

    def arg_error(fn):
        with pytest.raises(vo.VOError) as e:
            fn()
        assert e.value.code == vo.VO_ERR_ARG, e.value

    arg_error(lambda: ctx.undistort(img, K, (float("nan"), 0.0, 0.0), tan))
    arg_error(lambda: ctx.undistort(img, K, rad, (0.0, float("inf"))))
    K0 = K.copy()
    K0[0, 0] = 0.0
    arg_error(lambda: ctx.undistort(img, K0, rad, tan))
    K1 = K.copy()
    K1[2] = [0.0, 1e-3, 1.0]
    arg_error(lambda: ctx.undistort(img, K1, rad, tan))
    arg_error(lambda: ctx.set_distortion(vo.distortion_from(K1, rad, tan), None))
    arg_error(lambda: ctx.undistort(np.zeros((rows, cols + 1), np.uint8), K, rad, tan))       # not the context's size
    d = vo.distortion_from(K, rad, tan)
    p8 = C.POINTER(C.c_uint8)
    out = np.zeros((rows, cols), np.uint8)
    for ld, ld_out in ((cols - 1, cols), (cols, cols - 1)):
        assert ctx.lib.vo_undistort(ctx.h, img.ctypes.data_as(p8), rows, cols, ld, 0, C.byref(d), out.ctypes.data_as(p8),
                                    ld_out) == vo.VO_ERR_ARG
    buf = torch.zeros((2, rows, cols), dtype=torch.uint8, device="cuda")
    arg_error(lambda: ctx.undistort_batch_dev(buf.data_ptr(), buf.data_ptr(), 2, K, rad, tan))
    arg_error(lambda: ctx.undistort_batch_dev(buf.data_ptr(), buf.data_ptr() + rows * cols, 0, K, rad, tan))
