"""GPU: triangulate's reprojectionErrors / validIndex through libvo.so (vo_triangulate_ex,
vo_fetch_track_quality; k_tri_quality) against the CPU build of the same include/vo_spec.h function
(tests/tri_quality_ref, which test_tri_quality.py holds to a longdouble evaluation).  Finite values
are compared by bytes, the others by kind (nan, +inf, -inf).  Contexts are the smallest the calls
accept (64 x 64 images, one frame), the loop runs the 150 x 497 scene of the lost-frames test."""
import numpy as np
import pytest

import geom_ref as G
import tri_quality_ref as T

pytestmark = pytest.mark.gpu

P1, P2 = G.KITTI_P1, G.KITTI_P2


@pytest.fixture(scope="module")
def ctx(vo):
    c = vo.Context(64, 64, 1, calib=vo.calib_from(P1, P2))
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx256(vo):
    """kp_cap = 256: the chunk loop."""
    c = vo.Context(64, 64, 1, calib=vo.calib_from(P1, P2), sift=vo.default_sift_params(256))
    yield c
    c.close()


def _tri_points(n, seed):
    return G.stereo_rows(np.random.default_rng([0x791, seed]), n, 2.0, 300.0)


def _check_all_forms(c, oracle, l, r, Pa, Pb):
    """Every form of the call on one input -> (X, err, valid) of quality=True: X is vo_triangulate's
    and the oracle's, err / valid the reference's on that X; err-only and valid-only (the other
    pointer NULL) and quality=False give the same."""
    n = len(l)
    plain = c.triangulate(l, r, Pa, Pb)
    with np.errstate(all="ignore"):
        T.same_class(plain, oracle.triangulate(l, r, Pa, Pb))
        X, err, valid = c.triangulate(l, r, Pa, Pb, quality=True)
        assert X.shape == (n, 3) and err.shape == (n,) and err.dtype == np.float32 and valid.shape == (n,) and valid.dtype == bool
        T.same_class(X, plain)
        rerr, rvalid = T.quality(l, r, X, Pa, Pb)
        T.same_class(err, rerr)
        assert np.array_equal(valid, rvalid)
        Xe, e2, none = c.triangulate(l, r, Pa, Pb, quality="err")
        assert none is None
        T.same_class(Xe, plain)
        T.same_class(e2, rerr)
        Xv, none, v2 = c.triangulate(l, r, Pa, Pb, quality="valid")
        assert none is None and np.array_equal(v2, rvalid)
        T.same_class(Xv, plain)
        T.same_class(c.triangulate(l, r, Pa, Pb, quality=False), plain)
    return X, err, valid


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_small_n(ctx, oracle, n):
    l, r = _tri_points(n, n)
    X, err, valid = _check_all_forms(ctx, oracle, l, r, P1, P2)
    assert X.tobytes() == oracle.triangulate(l, r, P1, P2).tobytes()
    assert np.isfinite(err).all() and valid.all()


@pytest.mark.parametrize("n", [513, 600])
def test_chunk_loop(ctx256, oracle, n):
    """n > kp_cap = 256: two whole chunks and 1 or 88 rows, each chunk's err and valid landing at
    its own offset.  The reference errors differ from row to row, so a misplaced chunk shows; a few
    rows with negative disparity, one in each chunk, do the same for valid."""
    l, r = _tri_points(n, n)
    bad = [5, 300, n - 1]
    r[bad, 0] = l[bad, 0] + np.float32(4.0)
    X, err, valid = _check_all_forms(ctx256, oracle, l, r, P1, P2)
    assert len(np.unique(err)) > 1 and not np.array_equal(err[:256], err[256:512])
    assert np.flatnonzero(~valid).tolist() == bad


def test_degenerate_rows(ctx, oracle):
    """The rows of test_triangulate_degenerate_rows -- zero disparity (the point at infinity),
    negative disparity (behind the cameras), coordinates at 1e6 -- and the four probe pairs; then a
    second camera that is not rectified."""
    l, r = _tri_points(64, 99)
    r[0:8] = l[0:8]                                   # zero disparity, equal rows
    r[8:16, 0] = l[8:16, 0]                           # zero disparity, rows apart
    r[16:24, 0] = l[16:24, 0] + np.float32(3.5)       # negative disparity
    l[24:28] *= np.float32(1e6 / 600.0)
    r[24:28] *= np.float32(1e6 / 600.0)
    l[28:32] = np.float32(1e6)
    r[28:32] = np.float32(1e6)
    # The Jacobi null vector of a zero-disparity pair has a tiny last component, not a zero one, so
    # all rows above come out finite (huge).  Rows that do leave the finite range: a NaN pixel
    # coordinate in either view (NaN throughout), and a zero-disparity pair at 3e38, whose point
    # overflows single (+-inf, err NaN); the same pair with opposite signs stays finite, err ~ 4e30.
    big = np.float32(3e38)
    xl = np.float32([[np.nan, 180], [600, 180], [big, 180], [600, 180]])
    xr = np.float32([[590, 180], [590, np.nan], [big, 180], [-big, 180]])
    l, r = np.vstack([l, T.PROBE_X1, xl]), np.vstack([r, T.PROBE_X2, xr])
    X, err, valid = _check_all_forms(ctx, oracle, l, r, P1, P2)
    print("non-finite err rows", np.flatnonzero(~np.isfinite(err)).tolist(), "invalid rows", np.flatnonzero(~valid).tolist())
    assert (~valid).any() and (~np.isfinite(err)).any()            # not vacuous
    assert not valid[16:24].any()
    assert valid[64:68].tolist() == [False, True, True, True]
    assert X[64, 2] < 0 and err[64] < 1e-6 and err[66] == np.float32(0.25)
    assert np.isnan(X[68:70]).all() and np.isinf(X[70]).all() and np.isnan(err[68:71]).all() and not valid[68:71].any()
    assert np.isfinite(err[71]) and err[71] > 1e30
    x1, x2, Pa, Pb = G.tri_fixtures()["general_P2"]
    _, err, valid = _check_all_forms(ctx, oracle, x1, x2, Pa, Pb)
    assert np.isfinite(err).all() and valid.all()


def test_launches_only_when_asked(vo, oracle):
    """k_tri_quality runs once per chunk of a call that asks for an output, and in no other: not in
    vo_triangulate, not with both pointers NULL, not for n = 0."""
    c = vo.Context(64, 64, 1, sift=vo.default_sift_params(256))
    try:
        c.set_profiling(True)
        l, r = _tri_points(600, 7)
        c.triangulate(l, r, P1, P2)
        c.triangulate(l[:0], r[:0], P1, P2, quality=True)
        x = np.zeros((600, 3))
        _p = lambda a, t: a.ctypes.data_as(vo.C.POINTER(t))
        assert c.lib.vo_triangulate_ex(c.h, _p(l, vo.C.c_float), _p(r, vo.C.c_float), 600, _p(np.ascontiguousarray(P1), vo.C.c_double),
                                       _p(np.ascontiguousarray(P2), vo.C.c_double), _p(x, vo.C.c_double), None, None) == 0
        assert x.tobytes() == oracle.triangulate(l, r, P1, P2).tobytes()
        off = c.kernel_times()
        assert "k_tri_list" in off and "k_tri_quality" not in off, sorted(off)
        c.triangulate(l, r, P1, P2, quality=True)
        on = c.kernel_times()
        assert set(on) - set(off) == {"k_tri_quality"} and on["k_tri_quality"][1] == 3
    finally:
        c.close()


# ----------------------------------------------------------------- the loop
ROWS, COLS, SCALE = 150, 497, 0.4


@pytest.fixture(scope="module")
def seq(syn):
    L, R, _ = syn.sequence(4, rows=ROWS, cols=COLS, scale=SCALE)
    return np.ascontiguousarray(L), np.ascontiguousarray(R), syn.calib(SCALE)


def _quality_equals_reference(c, f, A, B, oracle):
    tr = c.fetch_tracks(f)
    old_r, err, valid = c.fetch_track_quality(f)
    n = len(tr["old_l"])
    assert len(old_r) == n and len(err) == n and len(valid) == n
    assert old_r.dtype == np.float32 and old_r.shape == (n, 2) and err.dtype == np.float32 and valid.dtype == bool
    if n:
        # old_r is the right half of the pair the loop triangulated into world
        assert tr["world"].tobytes() == oracle.triangulate(tr["old_l"], old_r, A, B).tobytes()
        rerr, rvalid = T.quality(tr["old_l"], old_r, tr["world"], A, B)
        T.same_class(err, rerr)
        assert np.array_equal(valid, rvalid)
    return n, err, valid


def test_loop_quality_equals_reference_and_changes_nothing(vo, oracle, seq):
    """Two batches of two frames; after each, every frame's fetch_tracks and fetch_track_quality
    agree on the count and (err, valid) is the reference on the fetched (old_l, old_r, world) under
    the context's P1, P2.  Frame 0 has no rows.  Step outputs and landmarks are byte-equal to a
    context that never fetches quality."""
    L, R, (A, B) = seq
    cal = vo.calib_from(A, B)
    plain = vo.Context(ROWS, COLS, 2, calib=cal)
    want = np.concatenate([plain.step_batch(L[:2], R[:2]), plain.step_batch(L[2:], R[2:])])
    want_lm = plain.get_landmarks()
    plain.close()
    c = vo.Context(ROWS, COLS, 2, calib=cal)
    try:
        outs, counts = [], []
        for a in (0, 2):
            o = c.step_batch(L[a:a + 2], R[a:a + 2])
            outs.append(o)
            for f in range(2):
                n, err, valid = _quality_equals_reference(c, f, A, B, oracle)
                assert n == o[f]["n_tracked"]
                counts.append(n)
                if n:
                    print(f"frame {a + f}: {n} tracked, {int(valid.sum())} valid, err median {np.median(err):.3g} max {err.max():.3g} px")
        outs = np.concatenate(outs)
        assert counts[0] == 0 and max(counts[1:]) > 0
        assert outs.tobytes() == want.tobytes()
        assert c.get_landmarks().tobytes() == want_lm.tobytes()
    finally:
        c.close()


def test_state_rules(vo, oracle, seq):
    """As vo_fetch_tracks: a frame outside the last collected batch is VO_ERR_STATE; the fetch is
    legal while one other batch is pending (it works on the other buffer set) and gives what it
    gave before; once a second batch is submitted the collected set is reused and both fetches are
    VO_ERR_STATE."""
    import torch
    L, R, (A, B) = seq
    c = vo.Context(ROWS, COLS, 2, calib=vo.calib_from(A, B))
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    torch.cuda.synchronize()
    fs = L[0].size
    try:
        with pytest.raises(vo.VOError) as e:                  # nothing collected yet
            c.fetch_track_quality(0)
        assert e.value.code == vo.VO_ERR_STATE
        c.step_submit_dev(dl.data_ptr(), dr.data_ptr(), 2)
        o = c.step_collect()
        for f in (-1, 2):
            with pytest.raises(vo.VOError) as e:
                c.fetch_track_quality(f)
            assert e.value.code == vo.VO_ERR_STATE
        n, err, valid = _quality_equals_reference(c, 1, A, B, oracle)
        assert n == o[1]["n_tracked"] and n > 0
        c.step_submit_dev(dl.data_ptr() + 2 * fs, dr.data_ptr() + 2 * fs, 1)
        assert c.steps_pending() == 1
        n2, err2, valid2 = _quality_equals_reference(c, 1, A, B, oracle)
        assert n2 == n and err2.tobytes() == err.tobytes() and np.array_equal(valid2, valid)
        c.step_submit_dev(dl.data_ptr() + 3 * fs, dr.data_ptr() + 3 * fs, 1)
        for fetch in (c.fetch_tracks, c.fetch_track_quality):
            with pytest.raises(vo.VOError) as e:
                fetch(1)
            assert e.value.code == vo.VO_ERR_STATE
        with pytest.raises(vo.VOError) as e:                  # vo_triangulate_ex, like its sibling, is refused
            c.triangulate(T.PROBE_X1, T.PROBE_X2, A, B, quality=True)
        assert e.value.code == vo.VO_ERR_STATE
        c.step_collect()
        c.step_collect()
        _quality_equals_reference(c, 0, A, B, oracle)
    finally:
        c.close()
