"""GPU: bundleAdjustmentMotion through libvo.so (vo_refine_pose, vo_set_pose_refinement,
vo_fetch_pose_refinement; k_refine_pose) against the CPU build of the same include/vo_spec.h
functions (tests/pose_refine_ref, which test_pose_refine.py holds to a longdouble minimiser): the pose
and the stats are compared by bytes.  Contexts are the smallest the calls accept (64 x 64 images, one
frame); the loop runs the 150 x 497 four-frame scene of test_gpu_tri_quality.py in batches of 2."""
import numpy as np
import pytest

import geom_ref as G
import pose_refine_ref as P

pytestmark = pytest.mark.gpu

I4 = np.eye(4)


@pytest.fixture(scope="module")
def ctx(vo):
    c = vo.Context(64, 64, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx256(vo):
    c = vo.Context(64, 64, 1, sift=vo.default_sift_params(256))
    yield c
    c.close()


def _same(vo, c, uv, Xw, T0, K, use=None, **params):
    """Context.refine_pose and the reference on one input: equal by bytes -> (T, stats)."""
    T, st = c.refine_pose(uv, Xw, T0, K, use=use, params=vo.default_refine_params(**params) if params else None)
    Tr, sr = P.refine(uv, Xw, T0, K, use=use, **params)
    assert T.shape == (4, 4) and T.dtype == np.float64 and st.dtype == vo.REFINE_STATS_DTYPE
    assert vo.REFINE_STATS_DTYPE == P.STATS_DTYPE
    assert st.tobytes() == sr.tobytes(), (st, sr)
    assert T.tobytes() == Tr.tobytes(), np.abs(T - Tr).max()
    return T, st


def _problem(n, seed):
    rng = np.random.default_rng([0x6F0, n, seed])
    uv, Xw, K = G.pose_problem(rng, n, 0.2, noise=0.2)
    return uv, Xw, K, P.start_pose(rng, 0.3, 0.05)


@pytest.mark.parametrize("n", [0, 2, 3, 4, 63, 64, 65, 129])
def test_sizes_and_masks(vo, ctx, n):
    """use = all, = every third point, = the MSAC mask of vo_estworldpose on the same input (the
    start is then its pose); 20 % of the points are gross outliers, so the three differ."""
    uv, Xw, K, T0 = _problem(n, 0)
    T, st = _same(vo, ctx, uv, Xw, T0, K)
    assert st["n_used"] == n and (st["status"] == P.TOO_FEW) == (n < 3)
    if n < 3:
        assert T.tobytes() == T0.tobytes() and st["passes"] == 1 and st["accepted"] == 0
    third = np.arange(n) % 3 == 0
    T3, st3 = _same(vo, ctx, uv, Xw, T0, K, use=third)
    assert st3["n_used"] == int(third.sum())
    if n >= 4:
        rc, Te, mask, nin = ctx.estworldpose(uv, Xw, K, raise_on_failure=False)
        if rc == 0:
            Tm, stm = _same(vo, ctx, uv, Xw, Te, K, use=mask)
            assert stm["n_used"] == nin
            print(f"n {n}: all {st}, third {st3}, msac mask ({nin} inliers) {stm}")
    _same(vo, ctx, uv, Xw, T0, K, use=np.zeros(n, bool))


@pytest.mark.parametrize("max_iterations", [1, 2, 20])
def test_iteration_cap(vo, ctx, max_iterations):
    uv, Xw, K, T0 = _problem(129, 1)
    T, st = _same(vo, ctx, uv, Xw, T0, K, max_iterations=max_iterations)
    assert st["passes"] <= max_iterations
    if max_iterations == 1:
        assert T.tobytes() == T0.tobytes() and st["status"] == P.MAX_ITER


def test_rejections_skew_tolerances_and_full_capacity(vo, ctx, ctx256):
    uv, Xw, K, T0 = P.far_case()
    _, a = _same(vo, ctx, uv, Xw, T0, K)
    _, b = _same(vo, ctx, uv, Xw, T0, K, lambda0=1e-9)
    assert b["accepted"] < b["passes"] - 1 and b.tobytes() != a.tobytes()      # rejections, and another path than 1e-3
    for seed in range(3):                                                       # a candidate behind the camera
        uv, Xw, K, T0 = P.behind_case(seed)
        _, st = _same(vo, ctx, uv, Xw, T0, K)
        assert st["accepted"] < st["passes"] - 1
    rng = np.random.default_rng(0x5CE)
    uv, Xw, _ = G.pose_problem(rng, 100, 0.0, noise=0.3)
    uv = G.project(P.SKEWED_K, P.PLANTED_R, P.PLANTED_T, Xw) + rng.normal(0, 0.3, uv.shape)
    T0 = P.start_pose(rng, 1.0, 0.2)
    T, st = _same(vo, ctx, uv, Xw, T0, P.SKEWED_K)
    assert st["status"] == P.CONVERGED and P.pose_err_T(T) < P.pose_err_T(T0)
    _same(vo, ctx, uv, Xw, T0, P.SKEWED_K, relative_tolerance=1e-3)
    _same(vo, ctx, uv, Xw, T0, P.SKEWED_K, absolute_tolerance=1.0, relative_tolerance=0.0)
    uv, Xw, K, T0 = _problem(256, 2)                                            # n = max_keypoints
    _, st = _same(vo, ctx256, uv, Xw, T0, K)
    assert st["n_used"] == 256
    # points at or behind the camera plane at the start are not used
    R0, t0 = P.from_T(T0)
    Xw[5:40] = (np.array([0.5, 0.1, -2.0]) - t0) @ R0
    _, st = _same(vo, ctx256, uv, Xw, T0, K)
    assert st["n_used"] == 256 - 35


def test_refusals(vo, ctx256):
    uv, Xw, K, T0 = _problem(64, 3)
    c = ctx256
    bad = uv.copy()
    bad[17, 1] = np.nan
    with pytest.raises(vo.VOError) as e:
        c.refine_pose(bad, Xw, T0, K)
    assert e.value.code == vo.VO_ERR_ARG and "index 17" in str(e.value) and "imagePoints" in str(e.value)
    bad = Xw.copy()
    bad[41, 2] = np.inf
    with pytest.raises(vo.VOError) as e:
        c.refine_pose(uv, bad, T0, K)
    assert e.value.code == vo.VO_ERR_ARG and "index 41" in str(e.value) and "worldPoints" in str(e.value)
    for Tb, Kb in ((np.where(np.arange(16).reshape(4, 4) == 7, np.nan, T0), K), (T0, np.where(np.eye(3) == 1, K, np.nan))):
        with pytest.raises(vo.VOError) as e:
            c.refine_pose(uv, Xw, Tb, Kb)
        assert e.value.code == vo.VO_ERR_ARG
    Tb = T0.copy()
    Tb[3] = [0.0, 0.0, 1e-3, 1.0]
    with pytest.raises(vo.VOError) as e:
        c.refine_pose(uv, Xw, Tb, K)
    assert e.value.code == vo.VO_ERR_ARG and "last row" in str(e.value)
    for kw in (dict(max_iterations=0), dict(max_iterations=101), dict(relative_tolerance=-1.0), dict(absolute_tolerance=float("nan")),
               dict(lambda0=0.0), dict(lambda0=1e13)):
        with pytest.raises(vo.VOError) as e:
            c.refine_pose(uv, Xw, T0, K, params=vo.default_refine_params(**kw))
        assert e.value.code == vo.VO_ERR_ARG and next(iter(kw)) in str(e.value)
        with pytest.raises(vo.VOError) as e:
            c.set_pose_refinement(vo.default_refine_params(**kw))
        assert e.value.code == vo.VO_ERR_ARG
    uv, Xw, K, T0 = _problem(257, 3)
    with pytest.raises(vo.VOError) as e:
        c.refine_pose(uv, Xw, T0, K)
    assert e.value.code == vo.VO_ERR_CAPACITY
    with pytest.raises(vo.VOError) as e:                       # nothing collected, and never switched on
        c.fetch_pose_refinement(0)
    assert e.value.code == vo.VO_ERR_STATE


# ----------------------------------------------------------------- the loop
ROWS, COLS, SCALE = 150, 497, 0.4


def _mul4(A, B):
    """The 4 x 4 product as the library's pose chain forms it: left to right, no contraction."""
    C = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            C[i, j] = float(A[i, 0]) * float(B[0, j]) + float(A[i, 1]) * float(B[1, j]) + float(A[i, 2]) * float(B[2, j]) \
                + float(A[i, 3]) * float(B[3, j])
    return C


@pytest.fixture(scope="module")
def seq(syn):
    L, R, _ = syn.sequence(4, rows=ROWS, cols=COLS, scale=SCALE)
    return np.ascontiguousarray(L), np.ascontiguousarray(R), syn.calib(SCALE)


@pytest.fixture(scope="module")
def never_on(vo, seq):
    """The four frames through a context that never set the refinement: step outputs, landmarks,
    and per frame the tracked points with the MSAC pose and mask (the mask is not an output of the
    loop: vo_estworldpose on the fetched points with the frame's key gives the loop's own pose, which
    is checked, and with it the mask)."""
    L, R, (A, B) = seq
    K = np.ascontiguousarray(A[:, :3])
    c = vo.Context(ROWS, COLS, 2, calib=vo.calib_from(A, B))
    est = vo.Context(64, 64, 1)
    outs, frames = [], []
    try:
        for a in (0, 2):
            o = c.step_batch(L[a:a + 2], R[a:a + 2])
            outs.append(o)
            for f in range(2):
                tr = c.fetch_tracks(f)
                rec = dict(cur_l=tr["cur_l"].astype(np.float64), world=tr["world"], status=int(o[f]["status"]), T=None, mask=None)
                if o[f]["status"] == 0 and o[f]["n_tracked"] > 0:
                    rc, Te, mask, nin = est.estworldpose(rec["cur_l"], rec["world"], K, frame_key=a + f)
                    assert Te.tobytes() == o[f]["rel_pose"].tobytes() and nin == o[f]["n_inliers"]
                    rec.update(T=Te, mask=mask)
                frames.append(rec)
        return dict(outs=np.concatenate(outs), landmarks=c.get_landmarks(), frames=frames, K=K)
    finally:
        c.close()
        est.close()


def _expected_on(never_on):
    """Per frame (rel_pose, stats or None) of the refinement-on run, from the reference."""
    exp = []
    for rec in never_on["frames"]:
        if rec["T"] is None:
            exp.append((I4, None))
        else:
            exp.append(P.refine(rec["cur_l"], rec["world"], rec["T"], never_on["K"], use=rec["mask"]))
    return exp


def _check_on_batch(vo, c, o, a, never_on, exp, pose):
    for f in range(2):
        T, st = exp[a + f]
        got = c.fetch_pose_refinement(f)
        if st is None:
            assert (got["status"], got["n_used"], got["passes"], got["accepted"]) == (P.TOO_FEW, 0, 0, 0)
        else:
            assert got.tobytes() == st.tobytes(), (got, st)
            pose = _mul4(pose, T)
        assert o[f]["rel_pose"].tobytes() == np.ascontiguousarray(T).tobytes()
        assert o[f]["pose"].tobytes() == pose.tobytes()
        w = never_on["outs"][a + f]
        for name in ("status", "n_left", "n_right", "n_stereo", "n_tracked", "n_inliers", "n_landmarks", "flags"):
            assert o[f][name] == w[name], name
    return pose


def test_loop_refines_every_tracked_frame_and_off_is_untouched(vo, seq, never_on):
    L, R, (A, B) = seq
    exp = _expected_on(never_on)
    assert sum(st is not None for _, st in exp) >= 2
    assert any(st is not None and st["accepted"] > 0 for _, st in exp)               # not vacuous: poses do move
    c = vo.Context(ROWS, COLS, 2, calib=vo.calib_from(A, B))
    try:
        c.set_profiling(True)
        c.refine_pose(np.zeros((0, 2)), np.zeros((0, 3)), I4, never_on["K"])         # n = 0 launches nothing
        off = np.concatenate([c.step_batch(L[:2], R[:2]), c.step_batch(L[2:], R[2:])])
        assert off.tobytes() == never_on["outs"].tobytes()
        assert "k_msac" in c.kernel_times() and "k_refine_pose" not in c.kernel_times()
        with pytest.raises(vo.VOError) as e:
            c.fetch_pose_refinement(0)
        assert e.value.code == vo.VO_ERR_STATE
        c.reset()
        c.set_pose_refinement(vo.default_refine_params())
        pose = I4.copy()
        for k, a in enumerate((0, 2)):
            o = c.step_batch(L[a:a + 2], R[a:a + 2])
            pose = _check_on_batch(vo, c, o, a, never_on, exp, pose)
            assert c.kernel_times()["k_refine_pose"][1] == k + 1                     # once per step_batch
            for f in range(2):
                if exp[a + f][1] is not None:
                    print(f"frame {a + f}: {exp[a + f][1]}")
        assert c.get_landmarks().tobytes() != never_on["landmarks"].tobytes()        # the world transform follows the pose
        # off again on the same context (the setting survives the reset, so it is switched off by hand)
        c.reset()
        o = c.step_batch(L[:2], R[:2])
        _check_on_batch(vo, c, o, 0, never_on, exp, I4.copy())
        c.reset()
        c.set_pose_refinement(None)
        again = np.concatenate([c.step_batch(L[:2], R[:2]), c.step_batch(L[2:], R[2:])])
        assert again.tobytes() == never_on["outs"].tobytes()
        assert c.get_landmarks().tobytes() == never_on["landmarks"].tobytes()
    finally:
        c.close()


def test_pipelined_depth_two_gives_the_same_bytes(vo, seq, never_on):
    """vo_step_submit_dev / vo_step_collect with two batches in flight: the outputs and stats of
    step_batch; the fetch follows vo_fetch_tracks' state rules; the setters and the standalone call
    are refused while batches are pending."""
    import torch
    L, R, (A, B) = seq
    exp = _expected_on(never_on)
    c = vo.Context(ROWS, COLS, 2, calib=vo.calib_from(A, B))
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    torch.cuda.synchronize()
    fs = L[0].size
    try:
        c.set_pose_refinement(vo.default_refine_params())
        c.step_submit_dev(dl.data_ptr(), dr.data_ptr(), 2)
        c.step_submit_dev(dl.data_ptr() + 2 * fs, dr.data_ptr() + 2 * fs, 2)
        assert c.steps_pending() == 2
        for call in (lambda: c.set_pose_refinement(None), lambda: c.set_pose_refinement(vo.default_refine_params()),
                     lambda: c.refine_pose(np.zeros((0, 2)), np.zeros((0, 3)), I4, never_on["K"])):
            with pytest.raises(vo.VOError) as e:
                call()
            assert e.value.code == vo.VO_ERR_STATE
        o = c.step_collect()
        pose = _check_on_batch(vo, c, o, 0, never_on, exp, I4.copy())              # legal: the pending batch is on the other set
        for f in (-1, 2):
            with pytest.raises(vo.VOError) as e:
                c.fetch_pose_refinement(f)
            assert e.value.code == vo.VO_ERR_STATE
        c.step_submit_dev(dl.data_ptr(), dr.data_ptr(), 1)                          # reuses the collected batch's set
        with pytest.raises(vo.VOError) as e:
            c.fetch_pose_refinement(1)
        assert e.value.code == vo.VO_ERR_STATE
        o = c.step_collect()
        _check_on_batch(vo, c, o, 2, never_on, exp, pose)
        c.step_collect()
    finally:
        c.close()
