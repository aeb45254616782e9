"""extractFeatures at caller-given points on the device (vo_describe / vo_describe_batch: k_points
and k_desc_pts behind the scale space) against tests/describe_ref -- the oracle's own build_pyramid
and descriptor behind the inverse keypoint mapping of include/vo.h -- bit for bit.  The points a
test passes are chosen with the reference's radius expression, never with the library's check."""
import numpy as np
import pytest

import describe_ref

pytestmark = pytest.mark.gpu

ROWS, COLS = 112, 168
BIG = (188, 621)


def _sp(mod, upsample=1, L=3, max_keypoints=16384):
    p = mod.sift_params(max_keypoints) if hasattr(mod, "sift_params") else mod.default_sift_params(max_keypoints)
    p.upsample, p.n_octave_layers = upsample, L
    return p


def _oscale(octave, upsample):
    return np.float32(2.0 ** (octave + upsample) * (0.5 if upsample else 1.0))


def _edge_scl(r):
    """(largest float32 scl of window radius r, the next float32: radius r + 1), by the reference."""
    lo, hi = np.float32(0.0), np.float32(64.0)
    while np.nextafter(lo, hi) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if describe_ref.radius(mid) <= r:
            lo = mid
        else:
            hi = mid
    return lo, hi


def _valid(q, upsample):
    """rows whose octave-relative scale has a window radius of 1 .. 127 (reference arithmetic)"""
    scl = q["scale"] / np.array([_oscale(o, upsample) for o in q["octave"]], np.float32)
    r = np.array([describe_ref.radius(s) for s in scl])
    return (r >= 1) & (r <= 127)


def _points(vo, x, y, scl, angle, octave, layer, upsample):
    """keypoint rows from octave-relative scales"""
    n = len(np.atleast_1d(x))
    q = np.zeros(n, vo.KP_DTYPE)
    q["x"], q["y"], q["angle"], q["octave"], q["layer"] = x, y, angle, octave, layer
    q["scale"] = np.asarray(scl, np.float32) * np.array([_oscale(o, upsample) for o in q["octave"]], np.float32)
    q["size"] = np.nan                                  # ignored fields
    q["response"] = np.nan
    return q


def _random_points(vo, rng, n, rows, cols, upsample, L, n_oct):
    """positions in and around the image, any level of the first three octaves, radii 5 .. 64"""
    return _points(vo, rng.uniform(-20, cols + 20, n), rng.uniform(-20, rows + 20, n), rng.uniform(0.5, 6.0, n),
                   rng.uniform(0, 360, n), rng.integers(-upsample, min(3, n_oct) - upsample, n), rng.integers(0, L + 3, n),
                   upsample)


def _n_oct(oracle, rows, cols, upsample):
    return oracle.lib().oracle_num_octaves(rows, cols, upsample)


@pytest.fixture(scope="module")
def img(syn):
    return syn.stereo_pair(syn.SEED_BASE + 11, ROWS, COLS)[0]


@pytest.fixture(scope="module")
def big(syn):
    return syn.stereo_pair(syn.SEED_BASE + 12, *BIG)[0]


@pytest.fixture(scope="module", params=[1, 0], ids=["up1", "up0"])
def own(request, vo, oracle, img):
    """(upsample, context, the context's own detections of img, the reference's rows for them)"""
    up = request.param
    ctx = vo.Context(ROWS, COLS, 1, sift=_sp(vo, up))
    kps, desc = ctx.sift(img)
    rk, rd = oracle.sift(img, _sp(oracle, up))
    assert len(kps) >= 20 and kps.tobytes() == rk.tobytes() and np.array_equal(desc, rd)
    ref = describe_ref.describe(img, kps, _sp(oracle, up))
    assert np.array_equal(ref, desc)                   # the pin (tests/test_describe_ref.py) on this image
    yield up, ctx, kps, desc
    ctx.close()


# ---- own detections -----------------------------------------------------------------------------
def test_own_detections_in_any_order(own, img):
    up, ctx, kps, desc = own
    n = len(kps)
    rng = np.random.default_rng(5)
    orders = {"in order": np.arange(n), "reversed": np.arange(n)[::-1], "subset": rng.permutation(n)[: n // 3],
              "repeated": np.concatenate([np.arange(n), [0, 0, n - 1, 7, 7]])}
    for name, idx in orders.items():
        got = ctx.describe(img, kps[idx])
        assert got.shape == (len(idx), 128) and np.array_equal(got, desc[idx]), name
    wide = np.zeros((ROWS, COLS + 7), np.uint8)
    wide[:, :COLS] = img
    assert np.array_equal(ctx.describe(wide[:, :COLS], kps), desc)              # a row stride above cols
    assert np.array_equal(ctx.describe(np.asfortranarray(img), kps), desc)      # MATLAB's storage


# ---- arbitrary points ---------------------------------------------------------------------------
def test_moved_rescaled_reoriented_detections(vo, oracle, own, img):
    up, ctx, kps, desc = own
    rng = np.random.default_rng(6)
    sets = []
    for mul in (0.5, 0.8, 1.0, 1.7, 3.0):
        q = kps.copy()
        q["x"] += rng.uniform(-3, 3, len(q)).astype(np.float32)
        q["y"] += rng.uniform(-3, 3, len(q)).astype(np.float32)
        q["scale"] *= np.float32(mul)
        q["angle"] = rng.choice(np.array([0.0, 359.99, 360.0, 90.0, 45.5, 180.0, 271.3], np.float32), len(q))
        sets.append(q[_valid(q, up)])
    q = np.concatenate(sets)
    assert len(q) > 3 * len(kps) and {0.0, np.float32(359.99), 360.0} <= set(q["angle"].tolist())
    ref = describe_ref.describe(img, q, _sp(oracle, up))
    got = ctx.describe(img, q)
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert len(bad) == 0, (len(bad), len(q), bad[:5])


def test_every_level_of_the_first_and_last_octave(vo, oracle, own, img):
    up, ctx, _, _ = own
    L, n_oct = 3, _n_oct(oracle, ROWS, COLS, up)
    rows = []
    for octave in (-up, n_oct - 1 - up):
        for layer in range(L + 3):
            for ang in (0.0, 33.0):
                rows.append((COLS / 2 + 0.4, ROWS / 2 - 0.3, 1.5, ang, octave, layer))
    x, y, s, a, o, l = map(np.array, zip(*rows))
    q = _points(vo, x, y, s, a, o, l, up)
    ref = describe_ref.describe(img, q, _sp(oracle, up))
    got = ctx.describe(img, q)
    assert np.array_equal(got, ref)
    assert ref[: 2 * (L + 3)].any(axis=1).all()         # the first octave's rows are real descriptors
    assert len({r.tobytes() for r in ref[: 2 * (L + 3)]}) == 2 * (L + 3)   # ... and each level its own


def test_corners_borders_and_outside(vo, oracle, own, img):
    up, ctx, _, _ = own
    xs = [1, COLS, 1, COLS, 1, COLS, COLS / 2, COLS / 2, 0.5, COLS + 0.5, 2.25, COLS - 1.25]
    ys = [1, 1, ROWS, ROWS, ROWS / 2, ROWS / 2, 1, ROWS, 0.5, ROWS + 0.5, 2.25, ROWS - 1.25]
    out_x = [-500.0, 1000.0, COLS / 2, COLS / 2, -(2.0 ** 20) + 1, 2.0 ** 20 - 1, 2.0 ** 20 - 1, -80.0]
    out_y = [50.0, 900.0, -300.0, ROWS + 300.0, 2.0 ** 20 - 1, -(2.0 ** 20) + 1, 2.0 ** 20 - 1, -80.0]
    n_in, n_out = len(xs), len(out_x)
    q = np.concatenate([_points(vo, xs + out_x, ys + out_y, [scl] * (n_in + n_out), [ang] * (n_in + n_out),
                                [octave] * (n_in + n_out), [1] * (n_in + n_out), up)
                        for scl, ang, octave in ((1.0, 0.0, -up), (2.5, 77.0, -up), (2.5, 200.0, 1 - up))])
    ref = describe_ref.describe(img, q, _sp(oracle, up))
    got = ctx.describe(img, q)
    assert np.array_equal(got, ref)
    block = n_in + n_out
    for b in range(3):
        assert ref[b * block: b * block + n_in].any(axis=1).sum() >= n_in // 2     # borders still gather samples
        assert not ref[b * block + n_in: (b + 1) * block].any()                     # fully outside: 128 zeros


# ---- radius bounds ------------------------------------------------------------------------------
def test_minimum_side_image_with_the_largest_scale(vo, oracle, syn):
    """64 x 64: the plane's diagonal (int)sqrt(2 * 64^2) = 90 caps the window, not the 127."""
    small = syn.stereo_pair(syn.SEED_BASE + 13, 64, 64)[0]
    last127, _ = _edge_scl(127)
    assert describe_ref.radius(last127) == 127
    for up, octaves in ((0, (0, 1)), (1, (0, 1, -1))):
        q = np.concatenate([_points(vo, [32.4, 10.0, 70.0], [31.7, 55.0, 20.0], [last127] * 3, [0.0, 123.0, 360.0], [o] * 3,
                                    [1, 0, 5], up) for o in octaves])
        ref = describe_ref.describe(small, q, _sp(oracle, up))
        ctx = vo.Context(64, 64, 1, sift=_sp(vo, up))
        got = ctx.describe(small, q)
        ctx.close()
        assert np.array_equal(got, ref) and ref.any(axis=1).all()


def test_radius_127_radius_1_and_above_the_detecting_cap(vo, oracle, big):
    last127, _ = _edge_scl(127)
    _, first1 = _edge_scl(0)
    assert describe_ref.radius(last127) == 127 and describe_ref.radius(first1) == 1
    r60 = np.float32(60 / (3.0 * np.sqrt(2.0) * 2.5))
    assert describe_ref.radius(r60) == 60               # above the detecting launch's cap (41 at the defaults)
    rows, cols = BIG
    for up in (1, 0):
        sets = []
        for scl in (last127, first1, r60):
            for octave in (-up, 1 - up, 2 - up):
                sets.append(_points(vo, [cols / 2 + 0.3, 30.0, cols - 5.0, 200.7], [rows / 2, 20.0, rows - 3.0, 100.2],
                                    [scl] * 4, [0.0, 45.0, 301.5, 360.0], [octave] * 4, [1, 2, 3, 0], up))
        q = np.concatenate(sets)
        ref = describe_ref.describe(big, q, _sp(oracle, up))
        ctx = vo.Context(rows, cols, 1, sift=_sp(vo, up))
        got = ctx.describe(big, q)
        ctx.close()
        bad = np.flatnonzero((got != ref).any(axis=1))
        assert len(bad) == 0, (up, bad, q[bad])
        assert ref.any(axis=1).sum() >= len(q) - 12       # (a radius-1 window at a flat spot may be empty)


# ---- counts -------------------------------------------------------------------------------------
def test_counts_zero_capacity_and_beyond(vo, oracle, img):
    rng = np.random.default_rng(8)
    ctx = vo.Context(ROWS, COLS, 1, sift=_sp(vo, max_keypoints=16))
    n_oct = _n_oct(oracle, ROWS, COLS, 1)
    q = _random_points(vo, rng, 17, ROWS, COLS, 1, 3, n_oct)
    assert ctx.describe(img, q[:0]).shape == (0, 128)
    ref = describe_ref.describe(img, q, _sp(oracle))
    assert np.array_equal(ctx.describe(img, q[:16]), ref[:16])
    assert np.array_equal(ctx.describe(img, q[16:]), ref[16:])
    with pytest.raises(vo.VOError) as e:
        ctx.describe(img, q)
    assert e.value.code == vo.VO_ERR_CAPACITY
    bad = q[:5].copy()
    bad["layer"][3] = 6
    with pytest.raises(vo.VOError) as e:
        ctx.describe(img, bad)
    assert e.value.code == vo.VO_ERR_ARG and "point 3" in str(e.value)
    ctx.close()


# ---- batches ------------------------------------------------------------------------------------
@pytest.mark.parametrize("upsample", [1, 0])
def test_describe_batch(vo, oracle, syn, upsample):
    rng = np.random.default_rng(9)
    imgs = np.stack([syn.stereo_pair(syn.SEED_BASE + 20 + i, ROWS, COLS)[0] for i in range(6)])
    n_oct = _n_oct(oracle, ROWS, COLS, upsample)
    ctx = vo.Context(ROWS, COLS, 3, sift=_sp(vo, upsample))
    for counts in ([37, 0, 1, 16, 300], [5, 9, 0, 2, 64, 1], [4, 4], [0, 0, 0]):      # 6 = 2 x max_batch images
        pts = [_random_points(vo, rng, n, ROWS, COLS, upsample, 3, n_oct) for n in counts]
        got = ctx.describe_batch(imgs[: len(counts)], pts)
        assert [len(g) for g in got] == counts
        for i, (g, q) in enumerate(zip(got, pts)):
            assert np.array_equal(g, describe_ref.describe(imgs[i], q, _sp(oracle, upsample))), (counts, i)
    with pytest.raises(vo.VOError) as e:
        ctx.describe_batch(np.concatenate([imgs, imgs[:1]]), [pts[0][:1]] * 7)          # 2 x max_batch + 1 images
    assert e.value.code == vo.VO_ERR_ARG
    bad = [p.copy() for p in pts[:2]] + [_random_points(vo, rng, 4, ROWS, COLS, upsample, 3, n_oct)]
    bad[2]["angle"][1] = 361.0
    with pytest.raises(vo.VOError) as e:
        ctx.describe_batch(imgs[:3], bad)
    assert e.value.code == vo.VO_ERR_ARG and "image 2 point 1" in str(e.value)
    ctx.close()


def test_describe_batch_leaves_rows_beyond_the_counts_untouched(vo, oracle, syn, img):
    import ctypes as C
    rng = np.random.default_rng(10)
    imgs = np.stack([img, img[::-1].copy()])
    counts = np.array([3, 5], np.int32)
    stride = 6
    pts = np.zeros((2, stride), vo.KP_DTYPE)
    n_oct = _n_oct(oracle, ROWS, COLS, 1)
    for i, n in enumerate(counts):
        pts[i, :n] = _random_points(vo, rng, n, ROWS, COLS, 1, 3, n_oct)
    pts[0, 3:]["x"] = np.nan                            # rows beyond the counts are not read as points
    desc = np.full((2, stride, 128), 0xAB, np.uint8)
    ctx = vo.Context(ROWS, COLS, 1)
    ctx._check(ctx.lib.vo_describe_batch(ctx.h, imgs.ctypes.data_as(C.POINTER(C.c_uint8)), COLS, 0, 2,
                                         pts.ctypes.data_as(C.POINTER(vo.Keypoint)), counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                         stride, desc.ctypes.data_as(C.POINTER(C.c_uint8))))
    ctx.close()
    for i, n in enumerate(counts):
        assert np.array_equal(desc[i, :n], describe_ref.describe(imgs[i], pts[i, :n].copy(), _sp(oracle)))
        assert (desc[i, n:] == 0xAB).all()


# ---- state --------------------------------------------------------------------------------------
DETECTING = ("k_seg_", "k_refine", "k_orient", "k_scan_cands", "k_sel_", "k_expand", "k_ext_")


def test_state_around_describe(vo, oracle, own, img, syn):
    up, ctx, kps, desc = own
    rng = np.random.default_rng(12)
    q = _random_points(vo, rng, 40, ROWS, COLS, up, 3, _n_oct(oracle, ROWS, COLS, up))
    ref = describe_ref.describe(img, q, _sp(oracle, up))
    other = syn.stereo_pair(syn.SEED_BASE + 30, ROWS, COLS)[0]
    ctx.set_strongest(10)                               # does not apply: the points are already chosen
    assert np.array_equal(ctx.describe(img, q), ref)
    ctx.set_strongest(0)
    ctx.set_profiling(True)
    ctx.describe(other, q)
    names = set(ctx.kernel_times())
    ctx.set_profiling(False)
    assert {"k_points", "k_desc_pts"} <= names and "k_desc" not in names, names
    assert not [k for k in names if k.startswith(DETECTING)], names
    # the fetches of a detecting call's results are refused; the scale space is this call's
    for fetch in (lambda: ctx.fetch_keypoints(0), lambda: ctx.fetch_candidate_counts(0), lambda: ctx.fetch_stereo_pairs(0),
                  lambda: ctx.fetch_detected_count(0)):
        with pytest.raises(vo.VOError) as e:
            fetch()
        assert e.value.code == vo.VO_ERR_STATE
    g = ctx.fetch_gaussian(0, 1, 2)
    k2, d2 = ctx.sift(other)
    assert np.array_equal(g, ctx.fetch_gaussian(0, 1, 2))
    assert len(ctx.fetch_keypoints(0)[0]) == len(k2)    # a detecting call: the fetches read again
    k3, d3 = ctx.sift(img)
    assert k3.tobytes() == kps.tobytes() and np.array_equal(d3, desc)     # sift after describe = sift before


def test_loop_state_is_untouched_and_pending_batches_refuse(vo, syn):
    import torch
    rows, cols = BIG
    L, R, _ = syn.sequence(3, rows, cols, scale=0.5)
    cal = vo.calib_from(*syn.calib(0.5))
    plain = vo.Context(rows, cols, 2, calib=cal)
    want = np.concatenate([plain.step_batch(L[:2], R[:2]), plain.step_batch(L[2:], R[2:])])
    want_lm = plain.get_landmarks()
    plain.close()
    ctx = vo.Context(rows, cols, 2, calib=cal)
    a = ctx.step_batch(L[:2], R[:2])
    k, _ = ctx.sift(L[1])
    ctx.describe_batch(np.stack([R[0], L[2], R[2], L[0]]), [k[:50], k[:0], k[50:60], k])
    outs = np.concatenate([a, ctx.step_batch(L[2:], R[2:])])
    for f in outs.dtype.names:
        assert np.array_equal(outs[f], want[f]), f
    assert np.array_equal(ctx.get_landmarks(), want_lm)
    assert (outs["status"][1:] == 0).all() and (outs["n_tracked"][1:] > 4).all()
    dl, dr = torch.from_numpy(np.ascontiguousarray(L[:1])).cuda(), torch.from_numpy(np.ascontiguousarray(R[:1])).cuda()
    torch.cuda.synchronize()
    ctx.step_submit_dev(dl.data_ptr(), dr.data_ptr(), 1)
    with pytest.raises(vo.VOError) as e:
        ctx.describe(L[0], k[:3])
    assert e.value.code == vo.VO_ERR_STATE
    ctx.step_collect()
    ctx.close()


# ---- the toolbox-named entry ----------------------------------------------------------------------
def test_extract_features_at_given_points(vo, oracle, img):
    rng = np.random.default_rng(13)
    q = _random_points(vo, rng, 25, ROWS, COLS, 1, 3, _n_oct(oracle, ROWS, COLS, 1))
    feats, valid = vo.extractFeatures(img, q)
    assert feats.shape == (len(q), 128) and valid.tobytes() == q.tobytes()
    assert np.array_equal(feats, describe_ref.describe(img, q, _sp(oracle)))
    hand = {"x": q["x"], "y": q["y"], "scale": np.full(len(q), 2.0, np.float32)}       # SIFTPoints built by hand: level 0
    feats, valid = vo.extractFeatures(img, hand)
    assert (valid["layer"] == 0).all() and (valid["octave"] == 0).all()
    assert np.array_equal(feats, describe_ref.describe(img, valid, _sp(oracle)))
    all_desc, all_kps = vo.extractFeatures(img)                                        # points=None: as before
    rk, rd = oracle.sift(img)
    assert all_kps.tobytes() == rk.tobytes() and np.array_equal(all_desc, rd)
