"""matchFeatures options on the GPU: vo_match_ex / vo_match_f32_ex (Unique, MatchThreshold,
MaxRatio, matchMetric) against the numpy restatement of the spec (tests/match_ref.py, pinned to
the oracle by tests/test_match_options.py) -- pairs and metric bit for bit -- and, for general
single features, against a reference built from the oracle's match_f32 alone."""
import ctypes as C

import numpy as np
import pytest

import match_ref as mr
import mexshim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vo):
    c = vo.Context(64, 64, 1)
    yield c
    c.close()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n1,n2", mr.SHAPES + mr.DEGENERATE)
def test_match_ex_equals_the_restatement(ctx, n1, n2):
    F1, F2 = mr.features(n1, n2)
    for thr, ratio in mr.OPTIONS:
        for unique in (False, True):
            ref_p, ref_m = mr.reference(n1, n2, thr, ratio, unique)
            pairs, metric = ctx.match(F1, F2, unique=unique, match_threshold=thr, max_ratio=ratio, return_metric=True)
            assert np.array_equal(pairs, ref_p), (thr, ratio, unique)
            assert metric.dtype == np.float32 and np.array_equal(_bits(metric), _bits(ref_m)), (thr, ratio, unique)


@pytest.mark.parametrize("n1,n2", [(300, 257), (4100, 200), (0, 5)])
def test_null_opts_is_vo_match(ctx, vo, n1, n2):
    F1, F2 = mr.features(n1, n2)
    cap = max(n1, 1)
    pairs = np.zeros((cap, 2), np.uint32)
    n = C.c_int(0)
    rc = ctx.lib.vo_match_ex(ctx.h, vo._p(F1, C.c_uint8), n1, vo._p(F2, C.c_uint8), n2, None, vo._p(pairs, C.c_uint32), None, cap,
                             C.byref(n))
    assert rc == vo.VO_OK
    assert np.array_equal(pairs[: n.value], ctx.match(F1, F2))
    assert np.array_equal(pairs[: n.value], mr.reference(n1, n2)[0])


def test_crowded_column_follows_the_spec_order(ctx):
    F1, F2 = mr.crowded()
    spec, metric = mr.match(F1, F2, unique=True)
    swapped, _ = mr.match(F1, F2, unique=True, swapped_back=True)
    assert not np.array_equal(spec, swapped)
    pairs, got = ctx.match(F1, F2, unique=True, return_metric=True)
    assert np.array_equal(pairs, spec) and np.array_equal(_bits(got), _bits(metric))


def test_backward_tie_across_two_chunks(ctx):
    """F1 rows 10 and 4099 (one in each backward chunk of 4096 rows) are the same copy of F2 row
    5: the lower row wins the column.  The mirror: two distinct copies of a row in the second
    forward chunk."""
    F1, F2 = mr.chunk_tie_rows()
    assert ctx.match(F1, F2, unique=True).tolist() == [[11, 6]]
    assert ctx.match(F1, F2, unique=False, return_metric=True)[0].tolist() == [[11, 6], [4100, 6]]
    F1, F2 = mr.chunk_tie_cols()
    ref, ref_m = mr.match(F1, F2, unique=True)
    pairs, metric = ctx.match(F1, F2, unique=True, return_metric=True)
    assert len(ref) == 1 and np.array_equal(pairs, ref) and np.array_equal(_bits(metric), _bits(ref_m))


@pytest.mark.parametrize("n1,n2", [(33, 129), (300, 257), (4100, 200), (5, 0)])
def test_match_f32_ex_on_u8_valued_matrices(ctx, n1, n2):
    F1, F2 = mr.features(n1, n2)
    for unique in (False, True):
        ref_p, ref_m = mr.reference(n1, n2, 5.0, 0.8, unique)
        for order in ("C", "F"):
            A, B = np.array(F1, np.float32, order=order), np.array(F2, np.float32, order=order)
            pairs, metric = ctx.match_f32(A, B, unique=unique, match_threshold=5.0, max_ratio=0.8, return_metric=True)
            assert np.array_equal(pairs, ref_p) and np.array_equal(_bits(metric), _bits(ref_m)), (unique, order)


@pytest.mark.parametrize("n1,n2", [(33, 129), (129, 33), (300, 257)])
def test_match_f32_ex_general_features(ctx, oracle, n1, n2):
    """Reference from the oracle alone: forward = match_f32(F1, F2, params); back(j) = the F1 row
    match_f32(F2, F1) picks with MatchThreshold 100 and MaxRatio 1 (every F2 row returns one)."""
    F1, F2 = mr.general_features(n1, n2)
    back = oracle.match_f32(F2, F1, oracle.MatchParams(100.0, 1.0))
    assert np.array_equal(back[:, 0], np.arange(1, n2 + 1))
    for thr, ratio in mr.OPTIONS:
        fwd = oracle.match_f32(F1, F2, oracle.MatchParams(thr, ratio))
        ref = fwd[back[fwd[:, 1].astype(np.int64) - 1, 1] == fwd[:, 0]]
        assert 1 <= len(ref) < len(fwd)
        for order in ("C", "F"):
            A, B = np.array(F1, order=order), np.array(F2, order=order)
            p0, m0 = ctx.match_f32(A, B, match_threshold=thr, max_ratio=ratio, return_metric=True)
            p1, m1 = ctx.match_f32(A, B, unique=True, match_threshold=thr, max_ratio=ratio, return_metric=True)
            assert np.array_equal(p0, fwd) and np.array_equal(p1, ref), (thr, ratio, order)
            keep = (p0[:, None, :] == p1[None, :, :]).all(2).any(1)
            assert np.array_equal(_bits(m0[keep]), _bits(m1))


@pytest.mark.parametrize("thr,ratio,unique,reserved", [(0.0, 0.6, 0, 0), (30.0, 0.6, 0, 0), (1.0, 1.5, 0, 0), (1.0, 0.6, 0, 1)])
def test_argument_errors(ctx, vo, thr, ratio, unique, reserved):
    F1, F2 = mr.features(33, 129)
    opts = vo.MatchOpts(thr, ratio, unique, reserved)
    pairs = np.zeros((33, 2), np.uint32)
    n = C.c_int(0)
    rc = ctx.lib.vo_match_ex(ctx.h, vo._p(F1, C.c_uint8), 33, vo._p(F2, C.c_uint8), 129, C.byref(opts), vo._p(pairs, C.c_uint32),
                             None, 33, C.byref(n))
    assert rc == vo.VO_ERR_ARG
    A, B = F1.astype(np.float32), F2.astype(np.float32)
    rc = ctx.lib.vo_match_f32_ex(ctx.h, vo._p(A, C.c_float), 33, 128, vo._p(B, C.c_float), 129, 128, 0, C.byref(opts),
                                 vo._p(pairs, C.c_uint32), None, 33, C.byref(n))
    assert rc == vo.VO_ERR_ARG


def test_default_opts_and_capacity(ctx, vo):
    o = vo.MatchOpts()
    ctx.lib.vo_default_match_opts(C.byref(o))
    assert (o.match_threshold, o.max_ratio, o.unique, o.reserved) == (1.0, np.float32(0.6), 0, 0)
    F1, F2 = mr.features(33, 129)
    ref = mr.reference(33, 129)[0]
    pairs = np.zeros((4, 2), np.uint32)
    metric = np.zeros(4, np.float32)
    n = C.c_int(0)
    rc = ctx.lib.vo_match_ex(ctx.h, vo._p(F1, C.c_uint8), 33, vo._p(F2, C.c_uint8), 129, C.byref(o), vo._p(pairs, C.c_uint32),
                             vo._p(metric, C.c_float), 4, C.byref(n))
    assert rc == vo.VO_ERR_CAPACITY and n.value == len(ref) and np.array_equal(pairs, ref[:4])


def test_mex_match_options_through_the_real_library(ctx, vo):
    vo.load_library()                    # torch, then libvo: one HIP runtime in the process
    mex = mexshim.Mex(mexshim.REAL)
    try:
        F1, F2 = mr.features(300, 257)
        A, B = F1.astype(np.float32), F2.astype(np.float32)
        pairs, metric = mex.call("match", A, B, "unique", True, "MaxRatio", 0.8, nout=2)
        ref_p, ref_m = ctx.match(F1, F2, unique=True, max_ratio=0.8, return_metric=True)
        assert pairs.dtype == np.uint32 and np.array_equal(pairs, ref_p) and len(ref_p) == len(mr.reference(300, 257, 1.0, 0.8, True)[0])
        assert metric.dtype == np.float32 and metric.shape == (len(ref_p), 1) and np.array_equal(_bits(metric[:, 0]), _bits(ref_m))
        assert np.array_equal(mex.call("match", A, B), ctx.match(F1, F2))
        with pytest.raises(mexshim.MexError, match="vo:matchFeatures:options"):
            mex.call("match", A, B, "NoSuchOption", 1.0)
        with pytest.raises(mexshim.MexError, match="vo:badArgument"):
            mex.call("match", A, B, "MatchThreshold", 30.0)
    finally:
        mex.at_exit()
