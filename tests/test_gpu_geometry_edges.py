"""GPU: the geometry kernels at their branch edges, through libvo.so against the CPU oracle
(which test_geometry_ref.py holds to float64 references): k_lm_filter's 1024-row LDS staging,
groups of 8 and rounds of 1024; k_msac below one wave, at 63/64/65 points, at kp_cap, at chunk
edges of MaxNumTrials and with chunks of invalid slots; the device P3P's cubic solver;
vo_triangulate's chunk loop; vo_track on empty and single-row sides; lost frames in the loop.
Contexts are the smallest the calls accept (64 x 64 images, one frame)."""
import numpy as np
import pytest

import geom_ref as G

pytestmark = pytest.mark.gpu

K = G.KITTI_K
P1, P2 = G.KITTI_P1, G.KITTI_P2


@pytest.fixture(scope="module")
def ctx(vo):
    c = vo.Context(64, 64, 1, calib=vo.calib_from(P1, P2))
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx256(vo):
    """kp_cap = 256: capacity edges and vo_triangulate's chunk loop."""
    c = vo.Context(64, 64, 1, calib=vo.calib_from(P1, P2), sift=vo.default_sift_params(256))
    yield c
    c.close()


# ----------------------------------------------------------------- landmarks
@pytest.mark.parametrize("S,Kn", G.LANDMARK_SIZES)
def test_landmarks_sizes_bit_exact(ctx, oracle, S, Kn):
    """S stereo rows against Kn old rows around k_lm_filter's edges (1024 stereo rows per round,
    1024 old rows per LDS stage, groups of 8): equalities planted one coordinate at a time (lx,
    ly, rx, ry) in old rows of the first stage, of later stages and of the last Kn % 8 rows,
    against stereo rows of the first, second and third round.  Bit-equal to the oracle, and the
    rows missing from the output are the planted ones (landmarks_np, which is pinned to the oracle
    on the CPU, names them)."""
    l, r, old_l, old_r, plants = G.landmark_case(S, Kn)
    ref = oracle.landmarks(l, r, old_l, old_r, P1, P2, G.LANDMARK_POSE)
    _, info = G.landmarks_np(l, r, old_l, old_r, P1, P2, G.LANDMARK_POSE, oracle.triangulate)
    assert sorted(np.flatnonzero(info["hit"]).tolist()) == sorted(j for _, _, j in plants)
    got = ctx.landmarks(l, r, old_l, old_r, G.LANDMARK_POSE)
    assert got.shape == ref.shape
    assert got.tobytes() == ref.tobytes()


def test_landmarks_variants_bit_exact(ctx, oracle):
    """Every stereo row hit (M = 0: the two zero rows), M = 1, 2, 3, every depth beyond 80, negative
    disparity (two rows), and a gated tail (rows end at the last kept one)."""
    for name, (l, r, old_l, old_r, want) in G.landmark_variants().items():
        ref = oracle.landmarks(l, r, old_l, old_r, P1, P2, G.LANDMARK_POSE)
        got = ctx.landmarks(l, r, old_l, old_r, G.LANDMARK_POSE)
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), name
        if "rows" in want:
            assert len(got) == want["rows"], name


def test_landmarks_capacity(ctx256, vo, oracle):
    """S = kp_cap is accepted (and equals the oracle); S = kp_cap + 1 and Kn = kp_cap + 1 are
    refused with VO_ERR_CAPACITY."""
    l, r, old_l, old_r, _ = G.landmark_case(256, 256, seed=1)
    ref = oracle.landmarks(l, r, old_l, old_r, P1, P2, G.LANDMARK_POSE)
    got = ctx256.landmarks(l, r, old_l, old_r, G.LANDMARK_POSE)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()
    l, r, old_l, old_r, _ = G.landmark_case(257, 257, seed=1)
    for args in ((l, r, old_l[:256], old_r[:256]), (l[:256], r[:256], old_l, old_r)):
        with pytest.raises(vo.VOError) as e:
            ctx256.landmarks(*args, G.LANDMARK_POSE)
        assert e.value.code == vo.VO_ERR_CAPACITY


# ----------------------------------------------------------------- estworldpose
def _same_as_oracle(vo, oracle, c, uv, Xw, key, trials=None):
    rp = orp = None
    if trials is not None:
        rp = vo.default_ransac_params()
        rp.max_num_trials = trials
        orp = oracle.ransac_params(trials)
    rst, rT, rinl, rnin = oracle.estworldpose(uv, Xw, K, params=orp, frame_key=key)
    st, T, inl, nin = c.estworldpose(uv, Xw, K, params=rp, frame_key=key, raise_on_failure=False)
    assert st == rst, (key, st, rst)
    assert nin == rnin
    if rst == 0:
        assert T.tobytes() == rT.tobytes(), key
        assert np.array_equal(inl, rinl)
    return rst, rT, rnin


@pytest.mark.parametrize("n", [4, 5, 6, 7, 8, 63, 64, 65, 127, 128, 129])
def test_estworldpose_small_n(ctx, vo, oracle, n):
    """Fewer points than a wave's 64 lanes, and one either side of one and two strides: 0.2 px
    noise, a quarter gross outliers from n = 8 up, three frame keys each; status, pose, mask and
    inlier count are the oracle's, and the oracle finds a pose every time."""
    uv, Xw, _ = G.pose_problem(np.random.default_rng([0xE57, n]), n, 0.25 if n >= 8 else 0.0, 0.2)
    for key in (0, 1, 2):
        rst, _, rnin = _same_as_oracle(vo, oracle, ctx, uv, Xw, key)
        assert rst == 0 and rnin >= 4


def test_estworldpose_at_capacity(ctx256, vo, oracle):
    """n = kp_cap runs and equals the oracle; n = kp_cap + 1 is refused."""
    uv, Xw, _ = G.pose_problem(np.random.default_rng(0xCA9), 257, 0.25, 0.2)
    rst, _, _ = _same_as_oracle(vo, oracle, ctx256, uv[:256], Xw[:256], 5)
    assert rst == 0
    with pytest.raises(vo.VOError) as e:
        ctx256.estworldpose(uv, Xw, K)
    assert e.value.code == vo.VO_ERR_CAPACITY


@pytest.mark.parametrize("trials", [1, 63, 64, 65, 128, 129])
def test_estworldpose_trials_at_chunk_edges(ctx, vo, oracle, trials):
    """MaxNumTrials one either side of k_msac's chunks of 64, at 75 % outliers so that the replay
    runs to the last slot (or nearly).  Three frame keys each."""
    uv, Xw, _ = G.pose_problem(np.random.default_rng(0x75), 200, 0.75, 0.2)
    for key in (0, 1, 2):
        _same_as_oracle(vo, oracle, ctx, uv, Xw, key, trials)


def test_estworldpose_degenerate_sets(ctx, vo, oracle):
    """No consensus on the device: four points behind the camera (every slot of every chunk
    invalid); 8 points of which 5 share one world position (most slots invalid: a zero side);
    collinear world points (the pose is free about the line: the oracle settles on one of them).
    Status and outputs are the oracle's."""
    uv = np.array([[100.0, 100], [300, 120], [500, 90], [200, 300]])
    rst, _, _ = _same_as_oracle(vo, oracle, ctx, uv, np.zeros((4, 3)), 0)
    assert rst == vo.VO_ERR_NO_CONSENSUS
    with pytest.raises(vo.VOError) as e:
        ctx.estworldpose(uv, np.zeros((4, 3)), K)
    assert e.value.code == vo.VO_ERR_NO_CONSENSUS
    uv8, Xw8, _ = G.pose_problem(np.random.default_rng(0xDE6), 8, 0.0, 0.2)
    Xw8[3:] = Xw8[3]
    for key in (0, 1, 2):
        _same_as_oracle(vo, oracle, ctx, uv8, Xw8, key)
    rng = np.random.default_rng(0xC011)
    s = rng.uniform(-4, 4, 12)
    Xl = np.array([0.5, -0.2, 20.0]) + s[:, None] * np.array([1.0, 0.1, 0.5])
    uvl = G.project(K, np.eye(3), np.zeros(3), Xl)
    for key in (0, 1, 2):
        _same_as_oracle(vo, oracle, ctx, uvl, Xl, key)


CUBIC_KEYS = 256          # keys 0..95 reach 23 of the 24 orderings (25 of them find no 4 distinct of 4 points
                          # in 16 attempts); 0..191 reach all, 0..255 sample a cubic ordering 21 times


def test_estworldpose_p3p_branches(vo, oracle):
    """The device P3P's fixed-degree solvers.  Four noise-free points, three of them a triple whose
    quartic has a vanishing leading coefficient when taken in the order (w0, w1, w2) or (w0, w2, w1);
    MaxNumTrials = 1, so slot 0's hypothesis is the answer, and the frame key decides the order
    in which slot 0 samples the points.  Over the keys every one of the 24 orderings occurs and at
    least 3 keys sample a cubic ordering; every key equals the oracle bit for bit, and the cubic
    keys give the generating pose to 1e-8."""
    uv3, Xw3, R, t = G.cubic_triples(1, seed=0xC0B1C + 1)[0]
    A, _ = G.grunert_quartic(uv3, Xw3, K)
    assert abs(A[4]) <= 1e-15 * np.abs(A).max()
    rng = np.random.default_rng(0x4F)
    x4 = (G.cam_points(rng, 1, 6.0, 20.0) - t) @ R
    Xw = np.vstack([Xw3, x4])
    uv = G.project(K, R, t, Xw)
    rp = vo.default_ransac_params()
    rp.max_num_trials = 1
    c = vo.Context(64, 64, 1, ransac=rp)
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = R.T, -R.T @ t
    orders, cubic = set(), 0
    try:
        for key in range(CUBIC_KEYS):
            idx = G.msac_sample(oracle, rp.seed, key, 0, 4)
            rst, rT, _ = _same_as_oracle(vo, oracle, c, uv, Xw, key, 1)
            if idx is None:
                assert rst == vo.VO_ERR_NO_CONSENSUS
                continue
            orders.add(tuple(idx))
            if idx[0] == 0 and set(idx[1:3]) == {1, 2}:
                cubic += 1
                assert rst == 0 and np.abs(rT - T0).max() < 1e-8, key
    finally:
        c.close()
    assert len(orders) == 24 and cubic >= 3


# ----------------------------------------------------------------- triangulate
def _same_class(got, ref):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    assert got[fin].tobytes() == ref[fin].tobytes()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref))


def _tri_points(n, seed):
    rng = np.random.default_rng([0x791, seed])
    l, r = G.stereo_rows(rng, n, 2.0, 300.0)
    return l, r


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_triangulate_small_n(ctx, oracle, n):
    l, r = _tri_points(n, n)
    got = ctx.triangulate(l, r, P1, P2)
    assert got.shape == (n, 3) and got.tobytes() == oracle.triangulate(l, r, P1, P2).tobytes()


@pytest.mark.parametrize("n", [512, 513, 600])
def test_triangulate_chunk_loop(ctx256, oracle, n):
    """n > kp_cap: vo_triangulate runs chunks of kp_cap = 256 rows (two whole ones; two and one
    row; two and 88 rows), each landing at its own offset of the output."""
    l, r = _tri_points(n, n)
    got = ctx256.triangulate(l, r, P1, P2)
    ref = oracle.triangulate(l, r, P1, P2)
    assert len(np.unique(ref, axis=0)) == n
    assert got.tobytes() == ref.tobytes()


def test_triangulate_degenerate_rows(ctx, oracle):
    """Rows with zero disparity (the point at infinity: w = 0), negative disparity (behind the
    cameras), coordinates at 1e6, and a second camera that is not rectified: finite values equal
    the oracle's bit for bit, the others are of the same kind (nan, +inf, -inf)."""
    l, r = _tri_points(64, 99)
    r[0:8] = l[0:8]                                   # zero disparity, equal rows
    r[8:16, 0] = l[8:16, 0]                           # zero disparity, rows apart
    r[16:24, 0] = l[16:24, 0] + np.float32(3.5)       # negative disparity
    l[24:28] *= np.float32(1e6 / 600.0)
    r[24:28] *= np.float32(1e6 / 600.0)
    l[28:32] = np.float32(1e6)
    r[28:32] = np.float32(1e6)
    with np.errstate(all="ignore"):
        _same_class(ctx.triangulate(l, r, P1, P2), oracle.triangulate(l, r, P1, P2))
        x1, x2, Pa, Pb = G.tri_fixtures()["general_P2"]
        ref = oracle.triangulate(x1, x2, Pa, Pb)
        assert np.isfinite(ref).all()
        _same_class(ctx.triangulate(x1, x2, Pa, Pb), ref)


# ----------------------------------------------------------------- track
def _jitter(rng, x):
    return np.clip(x.astype(int) + rng.integers(-2, 3, x.shape), 0, 255).astype(np.uint8)


def _track_problem(seed, n_old, n_cl, n_cr):
    """Old stereo rows, and current sides that hold them (jittered) in permuted order among
    distractor rows -- or fewer of them when a current side is shorter than the old one."""
    rng = np.random.default_rng([0x7AC, seed])
    A = rng.integers(0, 200, (n_old, 128)).astype(np.uint8)
    B = _jitter(rng, A)
    def side(D, n):
        rows = _jitter(rng, D[rng.permutation(n_old)[: min(n_old, n)]])
        rows = np.vstack([rows, rng.integers(0, 200, (n - len(rows), 128)).astype(np.uint8)])
        return rows[rng.permutation(n)]
    return A, B, side(A, n_cl), side(B, n_cr)


def test_track_empty_and_single_sides(ctx, oracle):
    """vo_track with no old rows, an empty current left side, an empty current right side, and one
    old row: the later match jobs run on empty index lists."""
    A, B, cl, cr = _track_problem(0, 40, 50, 45)
    none = np.zeros((0, 128), np.uint8)
    for old_l, old_r, l, r in ((none, none, cl, cr), (A, B, none, cr), (A, B, cl, none), (A[:1], B[:1], cl, cr),
                               (A, B, cl[:1], cr), (A, B, cl, cr)):
        ref = oracle.track(old_l, old_r, l, r)
        got = ctx.track(old_l, old_r, l, r)
        assert got.shape == ref.shape and np.array_equal(got, ref)
    assert len(oracle.track(A, B, cl, cr)) == 40 and len(oracle.track(A[:1], B[:1], cl, cr)) == 1


def test_track_no_survivors(ctx, oracle):
    """Old rows unrelated to the current ones: step 0 accepts nothing and steps 1-3 match empty
    lists; the result is empty, as the oracle's."""
    rng = np.random.default_rng(0x0DD)
    old_l, old_r, cl, cr = (rng.integers(0, 256, (n, 128)).astype(np.uint8) for n in (30, 30, 70, 65))
    assert oracle.track(old_l, old_r, cl, cr).shape == (0, 3)
    assert ctx.track(old_l, old_r, cl, cr).shape == (0, 3)


def test_track_ragged_sizes(ctx, oracle):
    """33 old rows among 511 current left and 513 current right rows (one row either side of two
    256-row tiles of the finishing kernel), and the hand-built permutation chain of the oracle's
    KAT at n = 60: every old row survives and sits where the permutations put it."""
    A, B, cl, cr = _track_problem(1, 33, 511, 513)
    ref = oracle.track(A, B, cl, cr)
    assert len(ref) == 33
    assert np.array_equal(ctx.track(A, B, cl, cr), ref)
    rng = np.random.default_rng(6)
    n = 60
    A = rng.integers(0, 200, (n, 128)).astype(np.uint8)
    Bd = _jitter(rng, A)
    pl, pr = rng.permutation(n), rng.permutation(n)
    cur_l = np.vstack([_jitter(rng, A[pl]), rng.integers(0, 200, (7, 128)).astype(np.uint8)])
    cur_r = np.vstack([_jitter(rng, Bd[pr]), rng.integers(0, 200, (5, 128)).astype(np.uint8)])
    got = ctx.track(A, Bd, cur_l, cur_r)
    assert np.array_equal(got, oracle.track(A, Bd, cur_l, cur_r))
    assert len(got) == n
    inv_l, inv_r = np.argsort(pl), np.argsort(pr)
    assert all(cl_ - 1 == inv_l[o - 1] and cr_ - 1 == inv_r[o - 1] for o, cl_, cr_ in got)


# ----------------------------------------------------------------- lost frames
def _compare_seq(outs, lm, routs, rlm):
    for f in range(len(outs)):
        for k in ("status", "n_left", "n_right", "n_stereo", "n_tracked", "n_inliers", "n_landmarks"):
            assert outs[f][k] == routs[f][k], (f, k, outs[f][k], routs[f][k])
        assert np.array_equal(outs[f]["rel_pose"], routs[f]["rel_pose"]), f
        assert np.array_equal(outs[f]["pose"], routs[f]["pose"]), f
    assert np.array_equal(lm, rlm)


@pytest.fixture(scope="module")
def lost(syn, oracle):
    """7 frames at 150 x 497; frame 2 blank on both sides, frame 4 blank on the right only."""
    A, B = syn.calib(0.4)
    L, R, _ = syn.sequence(7, rows=150, cols=497, scale=0.4)
    L, R = np.ascontiguousarray(L).copy(), np.ascontiguousarray(R).copy()
    L[2] = 0
    R[2] = 0
    R[4] = 0
    routs, (X, keep) = oracle.run_sequence(L, R, A, B, camera_rows=True)
    # the world rows are the camera-frame rows under each frame's pose (one oracle run, not two)
    off = np.r_[0, np.cumsum(routs["n_landmarks"])]
    rlm = np.vstack([oracle.landmarks_to_world(routs["pose"][f], X[off[f]:off[f + 1]], keep[off[f]:off[f + 1]])
                     for f in range(7)])
    return L, R, A, B, routs, rlm, (X, keep)


def test_lost_frames_fixture_shows_loss_and_recovery(lost, vo):
    """The oracle on the fixture: a blank pair, the frame after it, a blank right image and the
    frame after that are lost (status -3, nothing tracked, the pose held; the frames without
    stereo matches append the two rows of zeros(2, 3)); frames 1 and 6 find a pose."""
    *_, routs, rlm, _ = lost
    st = routs["status"].tolist()
    assert st[2:6] == [vo.VO_ERR_TOO_FEW_POINTS] * 4 and st[1] == 0 and st[6] == 0
    assert routs["n_stereo"][[2, 4]].tolist() == [0, 0] and routs["n_landmarks"][[2, 4]].tolist() == [2, 2]
    assert routs["n_tracked"][2:6].tolist() == [0, 0, 0, 0] and routs["n_landmarks"][3] > 2
    for f in range(2, 6):
        assert np.array_equal(routs["pose"][f], routs["pose"][1])
    assert not np.array_equal(routs["pose"][6], routs["pose"][1])


def test_lost_frames_bit_exact(vo, oracle, lost):
    """The device loop over lost frames (empty carry slot, empty lists, lm_rows = 2, the pose
    chain skipping a failed frame) equals the oracle: as one batch of 7, frame by frame, and
    pipelined two deep with bounds (0,3), (3,4), (4,7), so that a lost frame ends one batch and
    starts another; the same through the camera-frame rows, zero rows included."""
    import torch
    L, R, A, B, routs, rlm, (oX, okeep) = lost
    ctx = vo.Context(150, 497, 7, calib=vo.calib_from(A, B))
    try:
        _compare_seq(ctx.step_batch(L, R), ctx.get_landmarks(), routs, rlm)
        ctx.reset()
        outs = np.array([ctx.step(L[f], R[f]) for f in range(7)], dtype=routs.dtype)
        _compare_seq(outs, ctx.get_landmarks(), routs, rlm)
        dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        torch.cuda.synchronize()
        fs = L[0].size

        def run():
            outs = []
            for a, b in ((0, 3), (3, 4), (4, 7)):
                ctx.step_submit_dev(dl.data_ptr() + a * fs, dr.data_ptr() + a * fs, b - a)
                if ctx.steps_pending() == 2:
                    outs.append(ctx.step_collect())
            while ctx.steps_pending():
                outs.append(ctx.step_collect())
            return np.concatenate(outs)
        ctx.reset()
        _compare_seq(run(), ctx.get_landmarks(), routs, rlm)
        ctx.reset()
        ctx.set_landmark_frame(True)
        outs = run()
        X, keep = ctx.get_landmark_rows()
        assert np.array_equal(keep.astype(bool), okeep.astype(bool))
        assert X.tobytes() == np.ascontiguousarray(oX, np.float32).tobytes()
        assert np.array_equal(vo.landmarks_to_world_frames(outs["pose"], outs["n_landmarks"], X, keep), rlm)
    finally:
        ctx.close()
