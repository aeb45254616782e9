"""selectStrongest on the device (vo_set_strongest): k_sel_keys / k_sel_rank between the keypoint
scan and k_expand, through every entry that detects, against tests/strongest_ref.py -- the stable
descending sort over the oracle's detections and the VO.m loop over the oracle's per-call
functions -- bit for bit."""
import numpy as np
import pytest

import mexshim
import strongest_ref as sr

pytestmark = pytest.mark.gpu

ROWS, COLS = 188, 621


def _same(got, ref):
    """(keypoints, descriptors): the keypoint records bit for bit as structured arrays"""
    (k, d), (rk, rd) = got, ref
    assert len(k) == len(rk), (len(k), len(rk))
    assert k.dtype.itemsize == rk.dtype.itemsize and k.tobytes() == rk.tobytes()
    assert np.array_equal(d, rd)


def _same_steps(outs, lm, ref):
    routs, rlm = ref
    for k in routs.dtype.names:
        assert np.array_equal(outs[k], routs[k]), k
    assert lm.shape == rlm.shape and np.array_equal(lm, rlm)


# ---- a. ties and straddled peaks ----------------------------------------------------------------
def test_sift_ties_and_straddled_peaks(vo, oracle):
    img = sr.tie_image()
    kps, desc = oracle.sift(img)
    n = len(kps)
    assert n == 692
    ctx = vo.Context(img.shape[0], img.shape[1], 1)
    cap = ctx.sift_params.max_keypoints
    for N in list(range(1, 41)) + [n - 1, n, n + 1, cap]:
        ctx.set_strongest(N)
        _same(ctx.sift(img), sr.select(kps, desc, N))
        assert ctx.fetch_detected_count(0) == n, N
        k, d = ctx.fetch_keypoints(0)
        assert len(k) == min(N, n)
    ctx.set_strongest(0)
    _same(ctx.sift(img), (kps, desc))
    assert ctx.fetch_detected_count(0) == n
    ctx.close()


def test_off_path_launches_no_selection_kernel(vo):
    img = sr.tie_image()
    ctx = vo.Context(img.shape[0], img.shape[1], 1)
    ctx.set_profiling(True)
    ctx.sift(img)
    off = set(ctx.kernel_times())
    ctx.set_strongest(10)
    ctx.sift(img)
    on = set(ctx.kernel_times())
    ctx.close()
    assert "k_expand" in off and not any(k.startswith("k_sel") for k in off), off
    assert on - off == {"k_sel_keys", "k_sel_rank"}, on - off


# ---- b. batched path ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs5(syn, oracle):
    B = 5
    P = [syn.stereo_pair(11 + f, ROWS, COLS, noise_sd=1.0) for f in range(B)]
    L, R = np.stack([p[0] for p in P]), np.stack([p[1] for p in P])
    feats = sr.detect(L, R)
    return L, R, feats


def test_batched_sift_match(vo, oracle, pairs5):
    import torch
    L, R, feats = pairs5
    B = len(L)
    counts = sorted(len(x[0]) for fr in feats for x in fr)
    med = int(np.median(counts))
    assert counts[0] < med < counts[-1] and counts[0] > 64       # one batch: images with fewer than N and with more
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    torch.cuda.synchronize()
    ctx = vo.Context(ROWS, COLS, B)
    for N in (64, med):
        sel = [[sr.select(k, d, N) for k, d in fr] for fr in feats]
        ref_pairs = [oracle.match(fr[0][1], fr[1][1]) for fr in sel]
        assert all(len(p) >= 8 for p in ref_pairs), [len(p) for p in ref_pairs]
        ctx.set_strongest(N)
        for conc in (1, 2):
            ctx.set_concurrency(conc)
            for rep in range(2):                                  # back to back: both buffer sets
                stats = ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), B)
                for f in range(B):
                    for side in (0, 1):
                        _same(ctx.fetch_keypoints(2 * f + side), sel[f][side])
                        assert ctx.fetch_detected_count(2 * f + side) == len(feats[f][side][0])
                    assert np.array_equal(ctx.fetch_stereo_pairs(f), ref_pairs[f]), (N, conc, rep, f)
                    assert stats[f] == (len(sel[f][0][0]), len(sel[f][1][0]), len(ref_pairs[f]), 0), (N, conc, rep, f)
    ctx.close()


# ---- c. loop body -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seq(syn, oracle):
    L, R, _ = syn.sequence(5, ROWS, COLS, scale=0.5)
    P1, P2 = syn.calib(0.5)
    return L, R, P1, P2, sr.detect(L, R)


@pytest.fixture(scope="module")
def loops(seq):
    L, R, P1, P2, feats = seq
    cache = {}

    def get(N):
        if N not in cache:
            cache[N] = sr.loop(L, R, P1, P2, N=N, feats=feats)
        return cache[N]
    return get


@pytest.mark.parametrize("N", [150, 300])
def test_loop_body_three_forms(vo, seq, loops, N):
    import torch
    L, R, P1, P2, _ = seq
    ref = loops(N)
    assert (ref[0]["status"][1:] == 0).all() and (ref[0]["n_left"] == N).all() and (ref[0]["n_tracked"][1:] >= 40).all()
    cal = vo.calib_from(P1, P2)
    ctx = vo.Context(ROWS, COLS, 5, calib=cal)
    ctx.set_strongest(N)
    _same_steps(ctx.step_batch(L, R), ctx.get_landmarks(), ref)                      # one call
    ctx.reset()                                                                      # (keeps the setting)
    outs = np.concatenate([ctx.step_batch(L[:2], R[:2]), ctx.step_batch(L[2:], R[2:])])
    _same_steps(outs, ctx.get_landmarks(), ref)                                      # split 2 + 3
    ctx.close()
    dl, dr = torch.from_numpy(np.ascontiguousarray(L)).cuda(), torch.from_numpy(np.ascontiguousarray(R)).cuda()
    torch.cuda.synchronize()
    fs = L[0].size
    ctx = vo.Context(ROWS, COLS, 2, calib=cal)
    ctx.set_strongest(N)
    for a, b in ((0, 2), (2, 2), (4, 1)):                                            # three batches in flight
        ctx.step_submit_dev(dl.data_ptr() + a * fs, dr.data_ptr() + a * fs, b)
    assert ctx.steps_pending() == 3
    outs = np.concatenate([ctx.step_collect() for _ in range(3)])
    _same_steps(outs, ctx.get_landmarks(), ref)
    ctx.close()


def test_loop_body_n_above_every_count_is_sorted_not_detection_order(vo, oracle, seq, loops):
    L, R, P1, P2, feats = seq
    N = 4096
    assert N > max(len(x[0]) for fr in feats for x in fr)
    ref = loops(N)
    plain = oracle.run_sequence(L, R, P1, P2)
    ctx = vo.Context(ROWS, COLS, 5, calib=vo.calib_from(P1, P2))
    ctx.set_strongest(N)
    outs = ctx.step_batch(L, R)
    lm = ctx.get_landmarks()
    _same_steps(outs, lm, ref)
    assert np.array_equal(outs["n_left"], plain[0]["n_left"]) and np.array_equal(outs["n_right"], plain[0]["n_right"])
    assert not np.array_equal(outs["pose"], plain[0]["pose"]) or not np.array_equal(lm, plain[1])
    ctx.reset()
    ctx.set_strongest(0)                                          # off again: the plain loop body
    _same_steps(ctx.step_batch(L, R), ctx.get_landmarks(), plain)
    ctx.close()


# ---- d. with distortion -------------------------------------------------------------------------
def test_with_distortion(vo, syn, seq):
    from r7020e_visual_odometry_amd import kitti
    L, R, P1, P2, _ = seq
    K = np.ascontiguousarray(P1[:, :3])
    left, right = (-0.28, 0.07, 0.001, -0.0007, 0.0), (0.21, -0.03, 0.0, 0.0, 0.01)
    UL = np.stack([kitti.undistort(x, K, left) for x in L[:2]])
    UR = np.stack([kitti.undistort(x, K, right) for x in R[:2]])
    N = 200
    ref = sr.loop(UL, UR, P1, P2, N=N)
    # the reference is not degenerate: frame 1 tracks more than the 4 points P3P needs and finds a pose
    assert (ref[0]["n_left"] == N).all() and ref[0]["n_tracked"][1] > 4 and ref[0]["status"][1] == 0 and len(ref[1]) > 2
    ctx = vo.Context(ROWS, COLS, 2, calib=vo.calib_from(P1, P2))
    ctx.set_distortion(vo.distortion_from_kitti(K, left), vo.distortion_from_kitti(K, right))
    ctx.set_strongest(N)
    _same_steps(ctx.step_batch(L[:2], R[:2]), ctx.get_landmarks(), ref)
    ctx.close()


# ---- e. errors ----------------------------------------------------------------------------------
def test_errors_leave_the_setting_unchanged(vo, oracle, seq, loops):
    import torch
    img = sr.tie_image()
    kps, desc = oracle.sift(img)
    ctx = vo.Context(img.shape[0], img.shape[1], 1)
    ctx.set_strongest(33)
    for bad in (-1, ctx.sift_params.max_keypoints + 1):
        with pytest.raises(vo.VOError) as e:
            ctx.set_strongest(bad)
        assert e.value.code == vo.VO_ERR_ARG
        _same(ctx.sift(img), sr.select(kps, desc, 33))
    ctx.close()
    L, R, P1, P2, _ = seq
    dl, dr = torch.from_numpy(np.ascontiguousarray(L)).cuda(), torch.from_numpy(np.ascontiguousarray(R)).cuda()
    torch.cuda.synchronize()
    fs = L[0].size
    ctx = vo.Context(ROWS, COLS, 3, calib=vo.calib_from(P1, P2))
    ctx.set_strongest(150)
    ctx.step_submit_dev(dl.data_ptr(), dr.data_ptr(), 2)
    for n in (0, 300):
        with pytest.raises(vo.VOError) as e:
            ctx.set_strongest(n)
        assert e.value.code == vo.VO_ERR_STATE
    ctx.step_submit_dev(dl.data_ptr() + 2 * fs, dr.data_ptr() + 2 * fs, 3)
    outs = np.concatenate([ctx.step_collect(), ctx.step_collect()])
    _same_steps(outs, ctx.get_landmarks(), loops(150))
    ctx.close()


# ---- f. the MEX gateway against the real libvo --------------------------------------------------
def test_mex_strongest_then_sift(vo, oracle):
    vo.load_library()                    # torch, then libvo: one HIP runtime in the process
    m = mexshim.Mex(mexshim.REAL)
    try:
        img = sr.tie_image()
        kps, desc = oracle.sift(img)
        m.call("close", nout=0)
        m.call("strongest", np.float64(37), nout=0)               # before any context: kept for the session
        for N in (37, 5):
            if N != 37:
                m.call("strongest", np.float64(N), nout=0)        # on the live context
            loc, scale, ori, metric, d, octave, layer = m.call("sift", img, nout=7)
            rk, rd = sr.select(kps, desc, N)
            assert loc.shape == (N, 2) and np.array_equal(loc[:, 0], rk["x"]) and np.array_equal(loc[:, 1], rk["y"])
            assert np.array_equal(scale[:, 0], rk["scale"]) and np.array_equal(metric[:, 0], rk["response"])
            assert np.array_equal(ori[:, 0], (rk["angle"].astype(np.float64) * (np.pi / 180)).astype(np.float32))
            assert np.array_equal(d, rd.astype(np.float32))
            assert np.array_equal(octave[:, 0], rk["octave"]) and np.array_equal(layer[:, 0], rk["layer"])
        with pytest.raises(mexshim.MexError, match="vo:badArgument"):
            m.call("strongest", np.float64(-3), nout=0)
        m.call("strongest", np.float64(0), nout=0)
        assert m.call("sift", img, nout=1).shape == (len(kps), 2)
    finally:
        m.call("strongest", np.float64(0), nout=0)
        m.at_exit()
