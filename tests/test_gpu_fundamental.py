"""GPU: estimateFundamentalMatrix through libvo.so (vo_est_fundamental, vo_est_fundamental_batch;
k_fund_msac) against the CPU build of the same include/vo_spec.h functions (tests/fund_ref, which
test_fundamental.py holds to an SVD evaluation and whose census it asserts): F by bytes, the mask,
n_inliers and the status are equal for the whole census table.  Contexts are the smallest the calls
accept (64 x 64 images)."""
import numpy as np
import pytest

import fund_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vo):
    c = vo.Context(64, 64, 5, sift=vo.default_sift_params(512))
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """The reference's result of every row of the table, computed once."""
    return {name: R.estimate(x1, x2, key, **p) for name, x1, x2, p, key in R.table()}


def _params(vo, p):
    return vo.default_fund_params(**p)


def _same(got, exp, n):
    rc, F, mask, nin = got
    assert F.shape == (3, 3) and F.dtype == np.float64 and mask.shape == (n,) and mask.dtype == bool
    assert rc == exp["status"], (rc, exp["status"])
    assert nin == exp["n_inliers"] and np.array_equal(mask, exp["inliers"])
    assert F.tobytes() == exp["F"].tobytes(), np.abs(F - exp["F"]).max()


TABLE = R.table()


@pytest.mark.parametrize("row", range(len(TABLE)), ids=[t[0] for t in TABLE])
def test_table_equals_the_reference_by_bytes(vo, ctx, expected, row):
    name, x1, x2, p, key = TABLE[row]
    _same(ctx.est_fundamental(x1, x2, _params(vo, p), key), expected[name], len(x1))


def test_default_params_are_the_librarys(vo):
    p = vo.FundParams()
    vo.load_library().vo_default_fund_params(p)
    d = vo.default_fund_params()
    assert all(getattr(p, k) == getattr(d, k) for k, _ in vo.FundParams._fields_)
    assert {k: getattr(d, k) for k, _ in vo.FundParams._fields_} == R.DEFAULTS


def test_ragged_batch_equals_the_single_calls(vo, ctx):
    """B = 5 with counts 0, 7, 65, 300 and 129 in one launch: problem f is the single call with key0 + f."""
    counts = [0, 7, 65, 300, 129]
    stride = 300
    x1 = np.full((5, stride, 2), 7.0, np.float32)                       # rows beyond a count are never read
    x2 = np.full((5, stride, 2), 9.0, np.float32)
    for f, n in enumerate(counts):
        a, b, _ = R.case(n, "general", 0.1, 0.3 if n > 100 else 0.0, 50 + f)
        x1[f, :n], x2[f, :n] = a, b
    for method in (R.MSAC, R.NORM8):
        p = vo.default_fund_params(method=method, distance_threshold=0.1)
        st, F, mask, nin = ctx.est_fundamental_batch(x1, x2, counts, p, key0=11)
        assert list(st) == [R.TOO_FEW, R.TOO_FEW, R.OK, R.OK, R.OK]
        for f, n in enumerate(counts):
            exp = R.estimate(x1[f, :n], x2[f, :n], 11 + f, method=method, distance_threshold=0.1)
            _same((int(st[f]), F[f], mask[f, :n], int(nin[f])), exp, n)
            assert not mask[f, n:].any()
            one = ctx.est_fundamental(x1[f, :n], x2[f, :n], p, 11 + f)
            assert one[1].tobytes() == F[f].tobytes() and np.array_equal(one[2], mask[f, :n])


def test_refusals(vo, ctx):
    x1, x2, _ = R.case(20, "general", 0.1, 0.0, 1)
    for kw in (dict(method=2), dict(num_trials=0), dict(num_trials=100001), dict(distance_threshold=0.0),
               dict(distance_threshold=float("inf")), dict(confidence=0.0), dict(confidence=100.0)):
        p = vo.default_fund_params(**kw)
        F = np.zeros(9)
        rc = ctx.lib.vo_est_fundamental(ctx.h, vo._p(x1, vo.C.c_float), vo._p(x2, vo.C.c_float), 20, vo.C.byref(p), 0,
                                        vo._p(F, vo.C.c_double), None, None)                 # past vo.py's own check
        assert rc == vo.VO_ERR_ARG and next(iter(kw)) in ctx.lib.vo_last_error(ctx.h).decode()
    bad = x2.copy()
    bad[13, 1] = np.nan
    F = np.zeros(9)
    rc = ctx.lib.vo_est_fundamental(ctx.h, vo._p(x1, vo.C.c_float), vo._p(bad, vo.C.c_float), 20, None, 0, vo._p(F, vo.C.c_double),
                                    None, None)
    msg = ctx.lib.vo_last_error(ctx.h).decode()
    assert rc == vo.VO_ERR_ARG and "matchedPoints2(14, 2)" in msg and "point index 13" in msg
    a, b, _ = R.case(513, "general", 0.1, 0.0, 2)
    with pytest.raises(vo.VOError) as e:
        ctx.est_fundamental(a, b)
    assert e.value.code == vo.VO_ERR_CAPACITY
    with pytest.raises(vo.VOError) as e:
        ctx.est_fundamental_batch(np.zeros((6, 8, 2), np.float32), np.zeros((6, 8, 2), np.float32), [0] * 6)
    assert e.value.code == vo.VO_ERR_CAPACITY
    with pytest.raises(vo.VOError) as e:
        ctx.est_fundamental(x1, x2, raise_on_failure=True, params=vo.default_fund_params(distance_threshold=1e-12, num_trials=3))
    assert e.value.code == vo.VO_ERR_NO_CONSENSUS
    with pytest.raises(vo.VOError) as e:
        ctx.est_fundamental(x1[:7], x2[:7], raise_on_failure=True)
    assert e.value.code == vo.VO_ERR_TOO_FEW_POINTS


def test_module_level_function(vo):
    x1, x2, bad = R.case(129, "general", 0.1, 0.3, 77)
    F, inl, status = vo.estimateFundamentalMatrix(x1, x2, Method="MSAC", NumTrials=500, DistanceThreshold=0.1, Confidence=99.0)
    exp = R.estimate(x1, x2, 0, distance_threshold=0.1)
    assert status == 0 and F.tobytes() == exp["F"].tobytes() and np.array_equal(inl, exp["inliers"])
    assert not inl[bad].any() and inl[~bad].mean() > 0.7
    F8, inl8, s8 = vo.estimateFundamentalMatrix(x1[~bad], x2[~bad], Method="Norm8Point")
    assert s8 == 0 and inl8.all() and F8.tobytes() == R.norm8(x1[~bad], x2[~bad])[1].tobytes()
    assert vo.estimateFundamentalMatrix(x1[:7], x2[:7])[2] == 1
    assert vo.estimateFundamentalMatrix(x1, x2, DistanceThreshold=1e-12, NumTrials=2)[2] == 2


# ----------------------------------------------------------------- the rest of the context is untouched
ROWS, COLS, SCALE = 150, 497, 0.4


def test_loop_state_and_untouched_contexts(vo, syn):
    """A context that never calls launches no k_fund_msac; calls with n < 8 launch and allocate nothing;
    a call between two step batches leaves the loop's outputs and landmarks as they are without it; and
    the call is refused while a batch is pending."""
    import torch
    L, Rt, _ = syn.sequence(4, rows=ROWS, cols=COLS, scale=SCALE)
    L, Rt = np.ascontiguousarray(L), np.ascontiguousarray(Rt)
    A, B = syn.calib(SCALE)
    x1, x2, _ = R.case(65, "general", 0.1, 0.2, 5)
    plain = vo.Context(ROWS, COLS, 2, calib=vo.calib_from(A, B))
    c = vo.Context(ROWS, COLS, 2, calib=vo.calib_from(A, B))
    try:
        plain.set_profiling(True)
        c.set_profiling(True)
        want = [plain.step_batch(L[a:a + 2], Rt[a:a + 2]) for a in (0, 2)]
        assert "k_msac" in plain.kernel_times() and "k_fund_msac" not in plain.kernel_times()
        o0 = c.step_batch(L[0:2], Rt[0:2])
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        assert c.est_fundamental(x1[:7], x2[:7])[0] == R.TOO_FEW
        assert c.est_fundamental_batch(np.zeros((2, 0, 2), np.float32), np.zeros((2, 0, 2), np.float32), [0, 0])[0].tolist() == [R.TOO_FEW] * 2
        assert torch.cuda.mem_get_info()[0] == free0 and "k_fund_msac" not in c.kernel_times()
        exp = R.estimate(x1, x2, 3, distance_threshold=0.1)
        _same(c.est_fundamental(x1, x2, vo.default_fund_params(distance_threshold=0.1), 3), exp, 65)
        assert c.kernel_times()["k_fund_msac"][1] == 1                         # one launch per call
        o1 = c.step_batch(L[2:4], Rt[2:4])
        assert o0.tobytes() == want[0].tobytes() and o1.tobytes() == want[1].tobytes()
        assert c.get_landmarks().tobytes() == plain.get_landmarks().tobytes()
        dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(Rt).cuda()
        torch.cuda.synchronize()
        c.step_submit_dev(dl.data_ptr(), dr.data_ptr(), 2)
        with pytest.raises(vo.VOError) as e:
            c.est_fundamental(x1, x2)
        assert e.value.code == vo.VO_ERR_STATE
        c.step_collect()
    finally:
        plain.close()
        c.close()
