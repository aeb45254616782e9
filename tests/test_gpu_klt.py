"""GPU: the point tracker through libvo.so (vo_track_points, vo_track_points_batch, vo_fetch_klt_level;
k_klt_pyr, k_klt_track) against the CPU build of the same include/vo_spec.h functions (tests/klt_ref, which
test_klt.py holds to a float64 restatement and whose census it asserts): positions, validity, scores and
info are equal by bytes for the whole table, and so is every pyramid level.  Contexts are the smallest the
table needs (97 x 121 and 64 x 64 images, max_keypoints 512)."""
import numpy as np
import pytest

import klt_ref as R

pytestmark = pytest.mark.gpu

TABLE = R.table()
COUNTS = [0, 1, 63, 64, 65, 200]          # partial and full blocks of waves, an empty pair


@pytest.fixture(scope="module")
def ctxs(vo):
    c = {size: vo.Context(*R.SIZES[size], len(COUNTS), sift=vo.default_sift_params(512)) for size in R.SIZES}
    yield c
    for x in c.values():
        x.close()


def _params(vo, p):
    return vo.default_klt_params(num_pyramid_levels=p["levels"], block_size=p["block"], max_iterations=p["max_it"],
                                 max_bidirectional_error=p["max_bidir"])


def _same(got, exp, n):
    pts1, valid, scores, info = got
    assert pts1.shape == (n, 2) and pts1.dtype == np.float32 and valid.shape == (n,) and valid.dtype == bool
    assert np.array_equal(info["status"], exp["info"]["status"]), (info["status"], exp["info"]["status"])
    assert np.array_equal(valid, exp["valid"])
    assert info.tobytes() == exp["info"].tobytes()
    assert pts1.tobytes() == exp["pts1"].tobytes(), np.abs(pts1 - exp["pts1"]).max()
    assert scores.tobytes() == exp["scores"].tobytes(), np.abs(scores - exp["scores"]).max()


@pytest.mark.parametrize("row", range(len(TABLE)), ids=[t["name"] for t in TABLE])
def test_table_equals_the_reference_by_bytes(vo, ctxs, row):
    t, exp = TABLE[row], R.results()[row]
    img0, img1 = R.images(t["images"])
    got = ctxs[t["images"][0]].track_points(img0, img1, t["pts"], t["guess"], _params(vo, t["params"]))
    _same(got, exp, len(t["pts"]))


def test_default_params_are_the_librarys(vo):
    p = vo.KltParams()
    vo.load_library().vo_default_klt_params(p)
    d = vo.default_klt_params()
    assert (p.num_pyramid_levels, tuple(p.block_size), p.max_iterations, p.max_bidirectional_error) == \
           (d.num_pyramid_levels, tuple(d.block_size), d.max_iterations, d.max_bidirectional_error) == (3, (31, 31), 30, float("inf"))


@pytest.mark.parametrize("size", sorted(R.SIZES))
def test_every_pyramid_level_equals_the_reference_by_bytes(vo, ctxs, size):
    ctx = ctxs[size]
    imgs = R.images(size + ":s8")
    ctx.track_points(imgs[0], imgs[1], [[10.0, 10.0]], params=vo.default_klt_params(num_pyramid_levels=6))
    for which in range(2):
        for l, exp in enumerate(R.pyramid(imgs[which], 6)):
            got = ctx.fetch_klt_level(which, l)
            assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), (which, l)
    with pytest.raises(vo.VOError) as e:
        ctx.fetch_klt_level(2, 0)
    assert e.value.code == vo.VO_ERR_ARG
    ctx.track_points(imgs[0], imgs[1], [[10.0, 10.0]])
    with pytest.raises(vo.VOError) as e:
        ctx.fetch_klt_level(0, 3)                         # the last call had 3 levels
    assert e.value.code == vo.VO_ERR_ARG


def test_ragged_batch_equals_the_single_calls(vo, ctxs):
    """Counts 0, 1, 63, 64, 65 and 200 in one launch, with guesses: pair f is the single call, by bytes, and
    rows beyond a pair's count are untouched."""
    ctx = ctxs["a"]
    rows, cols = R.SIZES["a"]
    keys = ["a:s0", "a:s8", "a:s25", "a:same", "a:far", "a:s8"]
    imgs0 = np.stack([R.images(k)[0] for k in keys])
    imgs1 = np.stack([R.images(k)[1] for k in keys])
    sets = [np.concatenate([R.interior_points(rows, cols, 200, 20 + f, 3.0), R.side_points(rows, cols, (11, 11))])[:n]
            for f, n in enumerate(COUNTS)]
    guesses = [(s + np.float32([0.5, -0.25])).astype(np.float32) for s in sets]
    p = _params(vo, dict(R.DEFAULTS, block=(11, 11), max_bidir=0.75))
    batch = ctx.track_points_batch(imgs0, imgs1, sets, guesses, p)
    for f, n in enumerate(COUNTS):
        single = ctx.track_points(imgs0[f], imgs1[f], sets[f], guesses[f], p)
        exp = R.track(imgs0[f], imgs1[f], sets[f], guesses[f], **dict(R.DEFAULTS, block=(11, 11), max_bidir=0.75))
        _same(single, exp, n)
        _same(batch[f], exp, n)
    # the raw entry: rows beyond n_pts[f] stay as the caller has them
    import ctypes as C
    stride = 200
    pts = np.zeros((len(COUNTS), stride, 2), np.float32)
    for f, s in enumerate(sets):
        pts[f, :len(s)] = s
    out = np.full((len(COUNTS), stride, 2), -7.0, np.float32)
    valid = np.full((len(COUNTS), stride), 9, np.uint8)
    counts = np.array(COUNTS, np.int32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = ctx.lib.vo_track_points_batch(ctx.h, P(imgs0, C.c_uint8), P(imgs1, C.c_uint8), cols, 0, len(COUNTS), P(pts, C.c_float), None,
                                       P(counts, C.c_int32), stride, C.byref(p), P(out, C.c_float), P(valid, C.c_uint8), None, None)
    assert rc == vo.VO_OK
    for f, n in enumerate(COUNTS):
        assert (out[f, n:] == -7.0).all() and (valid[f, n:] == 9).all()
        assert (valid[f, :n] <= 1).all()


def test_col_major_and_padded_inputs(vo, ctxs):
    ctx = ctxs["a"]
    row, exp = TABLE[[t["name"] for t in TABLE].index("sides_a_31_L3")], None
    img0, img1 = R.images(row["images"])
    exp = R.results()[[t["name"] for t in TABLE].index("sides_a_31_L3")]
    p = _params(vo, row["params"])
    rows, cols = img0.shape
    _same(ctx.track_points(np.asfortranarray(img0), np.asfortranarray(img1), row["pts"], params=p), exp, len(row["pts"]))
    wide = [np.full((rows, cols + 13), 255, np.uint8) for _ in range(2)]
    tall = [np.full((rows + 5, cols), 255, np.uint8, order="F") for _ in range(2)]
    for w, t, im in zip(wide, tall, (img0, img1)):
        w[:, :cols] = im
        t[:rows] = im
    _same(ctx.track_points(wide[0][:, :cols], wide[1][:, :cols], row["pts"], params=p), exp, len(row["pts"]))
    _same(ctx.track_points(tall[0][:rows], tall[1][:rows], row["pts"], params=p), exp, len(row["pts"]))


def test_refusals_and_empty_calls(vo, ctxs):
    import ctypes as C
    ctx = ctxs["b"]
    img0, img1 = R.images("b:s0")
    pts, valid, scores, info = ctx.track_points(img0, img1, np.zeros((0, 2)))          # n = 0 launches nothing
    assert pts.shape == (0, 2) and valid.shape == (0,) and scores.shape == (0,) and info.shape == (0,)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    lib, h = ctx.lib, ctx.h
    rows, cols = img0.shape
    x = np.full((600, 2), 5.0, np.float32)
    out, ok = np.zeros_like(x), np.zeros(600, np.uint8)

    def call(n=4, pts=x, guess=None, params=None, r=rows, q=cols, ld=cols, cm=0):
        return lib.vo_track_points(h, P(img0, C.c_uint8), P(img1, C.c_uint8), r, q, ld, cm, P(pts, C.c_float),
                                   P(guess, C.c_float) if guess is not None else None, n, C.byref(params) if params is not None else None,
                                   P(out, C.c_float), P(ok, C.c_uint8), None, None)

    assert call() == vo.VO_OK
    assert call(n=513) == vo.VO_ERR_CAPACITY
    assert call(n=-1) == vo.VO_ERR_ARG and call(r=rows + 1) == vo.VO_ERR_ARG and call(ld=cols - 1) == vo.VO_ERR_ARG
    assert call(cm=2) == vo.VO_ERR_ARG
    bad = x.copy()
    bad[2, 1] = np.nan
    assert call(pts=bad) == vo.VO_ERR_ARG and "points(3, 2)" in lib.vo_last_error(h).decode()
    assert call(n=2, pts=bad) == vo.VO_OK                                              # the bad row is beyond n
    bad[2, 1] = 2.0 ** 20
    assert call(pts=bad) == vo.VO_ERR_ARG
    assert call(guess=bad) == vo.VO_ERR_ARG and "guess(3, 2)" in lib.vo_last_error(h).decode()
    for kw, word in ((dict(num_pyramid_levels=7), "num_pyramid_levels"), (dict(block_size=(31, 4)), "block_size[1]"),
                     (dict(block_size=(33, 5)), "block_size[0]"), (dict(max_iterations=0), "max_iterations"),
                     (dict(max_bidirectional_error=0.0), "max_bidirectional_error")):
        assert call(params=vo.default_klt_params(**kw)) == vo.VO_ERR_ARG
        assert word in lib.vo_last_error(h).decode()
    with pytest.raises(vo.VOError):
        ctx.track_points(img0, img1[:-1], x[:4])
    # a context that has not tracked has no level to fetch
    fresh = vo.Context(64, 64, 1, sift=vo.default_sift_params(512))
    try:
        with pytest.raises(vo.VOError) as e:
            fresh.fetch_klt_level(0, 0)
        assert e.value.code == vo.VO_ERR_STATE
        fresh.track_points(img0, img1, np.zeros((0, 2)))                               # still nothing launched
        with pytest.raises(vo.VOError) as e:
            fresh.fetch_klt_level(0, 0)
        assert e.value.code == vo.VO_ERR_STATE
    finally:
        fresh.close()


def test_point_tracker_carries_points_over_three_frames(vo, ctxs):
    ctx = ctxs["a"]
    rows, cols = R.SIZES["a"]
    f = R.field(rows, cols, 11)
    frames = [R.render(f, 1.5 * k, -0.75 * k) for k in range(3)]
    pts = R.interior_points(rows, cols, 50, 9, 30.0)
    tr = vo.PointTracker(ctx, MaxBidirectionalError=1.0)
    tr.initialize(pts, frames[0])
    for k in (1, 2):
        out, ok, sc = tr.step(frames[k])
        exp = pts + np.float32([1.5 * k, -0.75 * k])
        assert ok.all() and np.abs(out - exp).max() < 0.15 and (sc > 0.9).all()
    tr.set_points(pts[:5])
    assert tr.step(frames[2])[0].shape == (5, 2)


def test_tracking_between_steps_leaves_the_loop_untouched(vo, syn):
    """Two vo_step calls with a vo_track_points between them give the outputs of two without it (and the
    same landmarks); a context that never tracks launches neither kernel."""
    rows, cols, scale = 150, 497, 0.4
    L, Rt, _ = syn.sequence(2, rows=rows, cols=cols, scale=scale)
    cal = vo.calib_from(*syn.calib(scale))
    outs = []
    for between in (False, True):
        ctx = vo.Context(rows, cols, 1, calib=cal)
        try:
            ctx.set_profiling(True)
            rec = [ctx.step(L[0], Rt[0])]
            if between:
                pts1, valid, _, _ = ctx.track_points(L[0], L[1], R.interior_points(rows, cols, 100, 3))
                assert valid.sum() > 50
            rec.append(ctx.step(L[1], Rt[1]))
            names = set(ctx.kernel_times())
            assert ("k_klt_track" in names) == between and ("k_klt_pyr" in names) == between
            outs.append((np.array(rec).tobytes(), ctx.get_landmarks().tobytes()))
        finally:
            ctx.close()
    assert outs[0] == outs[1]


def test_refused_while_step_batches_are_pending(vo, syn):
    """VO_ERR_STATE while a submitted step batch has not been collected; the same call runs afterwards."""
    import torch
    rows, cols, scale = 150, 497, 0.4
    L, Rt, _ = syn.sequence(2, rows=rows, cols=cols, scale=scale)
    L, Rt = np.ascontiguousarray(L), np.ascontiguousarray(Rt)
    ctx = vo.Context(rows, cols, 1, calib=vo.calib_from(*syn.calib(scale)))
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(Rt).cuda()
    torch.cuda.synchronize()
    pts = R.interior_points(rows, cols, 20, 3)
    try:
        ctx.step_submit_dev(dl.data_ptr(), dr.data_ptr(), 1)
        with pytest.raises(vo.VOError) as e:
            ctx.track_points(L[0], L[1], pts)
        assert e.value.code == vo.VO_ERR_STATE
        ctx.step_collect()
        assert ctx.track_points(L[0], L[1], pts)[1].any()
    finally:
        ctx.close()
