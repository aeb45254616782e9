"""matchFeaturesInRadius on the GPU: vo_match_radius / vo_match_radius_f32 against the numpy
restatement (tests/match_radius_ref.py, held to match_ref and to the CPU build of vo_spec.h's gate
by tests/test_match_radius.py, which also asserts the census of these inputs) -- pairs and metric
bit for bit -- the chunk edges, the argument checks and the MEX command through the real library."""
import ctypes as C

import numpy as np
import pytest

import match_radius_ref as rr
import match_ref as mr
import mexshim

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ctx(vo):
    c = vo.Context(64, 64, 1)
    yield c
    c.close()


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def _same(got, ref, what=None):
    assert np.array_equal(got[0], ref[0]), what
    assert got[1].dtype == F32 and np.array_equal(_bits(got[1]), _bits(ref[1])), what


@pytest.mark.parametrize("layout", rr.LAYOUTS)
@pytest.mark.parametrize("n1,n2", rr.SHAPES)
def test_pairs_and_metric_equal_the_restatement(ctx, n1, n2, layout):
    F1, F2, P2, Cn, radius = rr.case(n1, n2, layout)
    for thr, ratio in mr.OPTIONS:
        for unique in (False, True):
            got = ctx.match_in_radius(F1, F2, P2, Cn, radius, unique=unique, match_threshold=thr, max_ratio=ratio,
                                      return_metric=True)
            _same(got, rr.reference(n1, n2, layout, thr, ratio, unique), (thr, ratio, unique))


def test_two_chunks_on_both_sides(ctx):
    """4100 x 4100, (y, x)-sorted: two forward and two backward chunks, whole tiles outside."""
    F1, F2, P2, Cn, radius = rr.case(4100, 4100, "sorted")
    for unique in (False, True):
        got = ctx.match_in_radius(F1, F2, P2, Cn, radius, unique=unique, return_metric=True)
        _same(got, rr.reference(4100, 4100, "sorted", 1.0, 0.6, unique), unique)


@pytest.mark.parametrize("n1,n2", [(33, 129), (300, 257), (4100, 200), (200, 4100)])
def test_huge_radius_is_match(ctx, n1, n2):
    F1, F2, P2, Cn, _ = rr.case(n1, n2, "perrow")
    for thr, ratio in mr.OPTIONS:
        for unique in (False, True):
            ref = ctx.match(F1, F2, unique=unique, match_threshold=thr, max_ratio=ratio, return_metric=True)
            for radius in (np.array([1e6], F32), np.full(n1, 1e6, F32)):
                got = ctx.match_in_radius(F1, F2, P2, Cn, radius, unique=unique, match_threshold=thr, max_ratio=ratio,
                                          return_metric=True)
                _same(got, ref, (thr, ratio, unique))
    # a radius whose square overflows to +inf admits every column as well
    _same(ctx.match_in_radius(F1, F2, P2, Cn, np.array([3e38], F32), return_metric=True), ctx.match(F1, F2, return_metric=True))


def test_degenerate_cases(ctx):
    rng = np.random.default_rng(9)
    b = rng.integers(0, 256, (1, 128), dtype=np.uint8)
    a = mr._noisy(b, rng)
    p2 = np.array([[100.0, 50.0]], F32)
    for centre, n in (([[101.5, 52.0]], 1), ([[103.0, 54.0]], 1), ([[103.25, 54.0]], 0)):     # inside, on the circle, outside
        pairs, metric = ctx.match_in_radius(a, b, p2, np.array(centre, F32), 5.0, return_metric=True)
        _same((pairs, metric), rr.match(a, b, p2, np.array(centre, F32), 5.0))
        assert len(pairs) == n and (n == 0 or (pairs.tolist() == [[1, 1]] and metric[0] == mr.scores(a, b)[0, 0]))
    F5 = rng.integers(0, 256, (5, 128), dtype=np.uint8)
    P5 = rng.uniform(0, 100, (5, 2)).astype(F32)
    none = np.zeros((0, 128), np.uint8), np.zeros((0, 2), F32)
    assert ctx.match_in_radius(none[0], F5, P5, none[1], 5.0).shape == (0, 2)
    assert ctx.match_in_radius(F5, none[0], none[1], P5, 5.0).shape == (0, 2)
    assert ctx.match_in_radius(F5, none[0], none[1], P5, np.full(5, 5.0, F32), unique=True).shape == (0, 2)
    # one candidate whose sv exceeds T: the ratio is 0, the threshold still decides
    far = rng.integers(0, 256, (1, 128), dtype=np.uint8)
    sv = mr.scores(far, b)[0, 0]
    assert F32(0.04) * F32(5.0) < sv <= F32(0.04) * F32(25.0)
    assert len(ctx.match_in_radius(far, b, p2, p2, 5.0, match_threshold=5.0, max_ratio=1.0)) == 0
    assert ctx.match_in_radius(far, b, p2, p2, 5.0, match_threshold=25.0, max_ratio=0.01).tolist() == [[1, 1]]
    # an exact duplicate pair inside the circle: 0 / 0 fails the ratio, as in matchFeatures
    bb = np.concatenate([b, b])
    pp = np.array([[100.0, 50.0], [101.0, 50.0]], F32)
    assert len(ctx.match_in_radius(b, bb, pp, p2, 5.0)) == 0 and len(rr.match(b, bb, pp, p2, 5.0)[0]) == 0
    assert ctx.match_in_radius(b, bb, pp, p2, 0.5).tolist() == [[1, 1]]


def test_forward_chunk_edge(ctx):
    """n2 = 4100: the row's best descriptor (an exact copy) sits in chunk 0 outside the circle, a
    noisy copy in chunk 1 inside: the pair is the one in chunk 1."""
    rng = np.random.default_rng(43)
    F1 = rng.integers(0, 256, (64, 128), dtype=np.uint8)
    F2 = rng.integers(0, 256, (4100, 128), dtype=np.uint8)
    P2 = np.stack([rng.integers(0, 4 * rr.WIDTH, 4100), rng.integers(0, 4 * rr.HEIGHT, 4100)], 1).astype(F32) * F32(0.25)
    Cn = np.full((64, 2), -500.0, F32)
    F2[7] = F1[3]
    F2[4098] = mr._noisy(F1[3:4], rng)[0]
    P2[7] = (900.0, 300.0)
    P2[4098] = (200.0, 100.0)
    Cn[3] = (203.0, 104.0)
    ref = rr.match(F1, F2, P2, Cn, 5.0)
    assert ref[0].tolist() == [[4, 4099]] and mr.match(F1, F2)[0].tolist() == [[4, 8]]
    for unique in (False, True):
        _same(ctx.match_in_radius(F1, F2, P2, Cn, 5.0, unique=unique, return_metric=True), ref)


def test_backward_chunk_edge(ctx):
    """n1 = 4100: rows 10 and 4099 (one in each backward chunk) are the same copy of F2 row 5, both
    inside: Unique keeps row 10.  With row 10's own radius shrunk so that the column is outside it,
    Unique keeps row 4099."""
    F1, F2 = mr.chunk_tie_rows()
    rng = np.random.default_rng(44)
    P2 = rng.uniform(0, 1000, (64, 2)).astype(F32)
    Cn = np.full((4100, 2), -500.0, F32)
    Cn[10] = P2[5] + F32(3.0)
    Cn[4099] = P2[5] - F32(2.0)
    radius = np.full(4100, 10.0, F32)
    assert ctx.match_in_radius(F1, F2, P2, Cn, radius).tolist() == [[11, 6], [4100, 6]]
    _same(ctx.match_in_radius(F1, F2, P2, Cn, radius, unique=True, return_metric=True), rr.match(F1, F2, P2, Cn, radius, unique=True))
    assert ctx.match_in_radius(F1, F2, P2, Cn, radius, unique=True).tolist() == [[11, 6]]
    radius[10] = 4.0                                      # d2 = 18 > 16
    assert ctx.match_in_radius(F1, F2, P2, Cn, radius, unique=True).tolist() == [[4100, 6]]
    _same(ctx.match_in_radius(F1, F2, P2, Cn, radius, unique=True, return_metric=True), rr.match(F1, F2, P2, Cn, radius, unique=True))


@pytest.mark.parametrize("n1,n2,layout", [(33, 129, "scalar"), (300, 257, "perrow"), (4100, 200, "sorted")])
def test_f32_entry_in_both_orders(ctx, vo, n1, n2, layout):
    F1, F2, P2, Cn, radius = rr.case(n1, n2, layout)
    for unique in (False, True):
        ref = ctx.match_in_radius(F1, F2, P2, Cn, radius, unique=unique, match_threshold=5.0, max_ratio=0.8, return_metric=True)
        _same(ref, rr.reference(n1, n2, layout, 5.0, 0.8, unique))
        for order in ("C", "F"):
            A, B = np.array(F1, F32, order=order), np.array(F2, F32, order=order)
            got = ctx.match_in_radius_f32(A, B, P2, Cn, radius, unique=unique, match_threshold=5.0, max_ratio=0.8, return_metric=True)
            _same(got, ref, (unique, order))
    A = np.array(F1, F32)
    A[1, 5] += F32(0.5)
    with pytest.raises(vo.VOError) as e:
        ctx.match_in_radius_f32(A, np.array(F2, F32), P2, Cn, radius)
    assert e.value.code == vo.VO_ERR_ARG


def _raw(ctx, vo, F1, F2, P2, Cn, radius, opts=None, cap=None):
    n1, n2 = len(F1), len(F2)
    cap = max(n1, 1) if cap is None else cap
    pairs = np.zeros((max(cap, 1), 2), np.uint32)
    metric = np.zeros(max(cap, 1), F32)
    n = C.c_int(-1)
    radius = np.ascontiguousarray(radius, F32)
    rc = ctx.lib.vo_match_radius(ctx.h, vo._p(F1, C.c_uint8), n1, vo._p(F2, C.c_uint8), n2, vo._p(P2, C.c_float), vo._p(Cn, C.c_float),
                                 vo._p(radius, C.c_float), len(radius), None if opts is None else C.byref(opts),
                                 vo._p(pairs, C.c_uint32), vo._p(metric, C.c_float), cap, C.byref(n))
    return rc, pairs, metric, n.value, ctx.lib.vo_last_error(ctx.h).decode()


def test_argument_errors(ctx, vo):
    F1, F2, P2, Cn, radius = rr.case(33, 129, "perrow")
    bad = P2.copy()
    bad[17, 1] = np.nan
    rc, *_, msg = _raw(ctx, vo, F1, F2, bad, Cn, radius)
    assert rc == vo.VO_ERR_ARG and "points2 row 17" in msg
    bad = Cn.copy()
    bad[4, 0] = np.inf
    rc, *_, msg = _raw(ctx, vo, F1, F2, P2, bad, radius)
    assert rc == vo.VO_ERR_ARG and "centers row 4" in msg
    for r in (0.0, -1.0, np.inf, np.nan):
        rc, *_, msg = _raw(ctx, vo, F1, F2, P2, Cn, [r])
        assert rc == vo.VO_ERR_ARG and "radius 0" in msg, r
        rr_ = radius.copy()
        rr_[20] = r
        rc, *_, msg = _raw(ctx, vo, F1, F2, P2, Cn, rr_)
        assert rc == vo.VO_ERR_ARG and "radius 20" in msg, r
    rc, *_, msg = _raw(ctx, vo, F1, F2, P2, Cn, [5.0, 5.0])
    assert rc == vo.VO_ERR_ARG and "n_radius 2" in msg
    for thr, ratio, unique, reserved in [(0.0, 0.6, 0, 0), (30.0, 0.6, 0, 0), (1.0, 1.5, 0, 0), (1.0, 0.6, 0, 1)]:
        rc, *_ = _raw(ctx, vo, F1, F2, P2, Cn, radius, vo.MatchOpts(thr, ratio, unique, reserved))
        assert rc == vo.VO_ERR_ARG
        A, B = F1.astype(F32), F2.astype(F32)
        pairs = np.zeros((33, 2), np.uint32)
        n = C.c_int(0)
        o = vo.MatchOpts(thr, ratio, unique, reserved)
        rc = ctx.lib.vo_match_radius_f32(ctx.h, vo._p(A, C.c_float), 33, 128, vo._p(B, C.c_float), 129, 128, 0, vo._p(P2, C.c_float),
                                         vo._p(Cn, C.c_float), vo._p(radius, C.c_float), 33, C.byref(o), vo._p(pairs, C.c_uint32),
                                         None, 33, C.byref(n))
        assert rc == vo.VO_ERR_ARG


def test_null_opts_and_capacity(ctx, vo):
    F1, F2, P2, Cn, radius = rr.case(300, 257, "perrow")
    ref_p, ref_m = rr.reference(300, 257, "perrow")
    rc, pairs, metric, n, _ = _raw(ctx, vo, F1, F2, P2, Cn, radius)
    assert rc == vo.VO_OK and n == len(ref_p) > 8 and np.array_equal(pairs[:n], ref_p) and np.array_equal(_bits(metric[:n]), _bits(ref_m))
    rc, pairs, metric, n, _ = _raw(ctx, vo, F1, F2, P2, Cn, radius, cap=4)
    assert rc == vo.VO_ERR_CAPACITY and n == len(ref_p)
    assert np.array_equal(pairs, ref_p[:4]) and np.array_equal(_bits(metric), _bits(ref_m[:4]))


def test_match_is_unchanged_around_an_in_radius_call(ctx):
    """vo_match, vo_match_ex and the in-radius entries share the staging buffers and partial slot."""
    F1, F2 = mr.features(300, 257)
    G1, G2, P2, Cn, radius = rr.case(4100, 200, "perrow")
    before = ctx.match(F1, F2), ctx.match(F1, F2, unique=True, return_metric=True)
    assert np.array_equal(before[0], mr.reference(300, 257)[0])
    _same(ctx.match_in_radius(G1, G2, P2, Cn, radius, unique=True, return_metric=True), rr.reference(4100, 200, "perrow", 1.0, 0.6, True))
    assert np.array_equal(ctx.match(F1, F2), before[0])
    _same(ctx.match(F1, F2, unique=True, return_metric=True), before[1])
    _same(ctx.match_in_radius(G1, G2, P2, Cn, radius, return_metric=True), rr.reference(4100, 200, "perrow"))


def test_module_level_function(vo):
    F1, F2, P2, Cn, radius = rr.case(129, 33, "perrow")
    kp = np.zeros(len(P2), vo.KP_DTYPE)
    kp["x"], kp["y"] = P2[:, 0], P2[:, 1]
    ref = rr.reference(129, 33, "perrow", 1.0, 0.6, True)
    _same(vo.matchFeaturesInRadius(F1, F2, kp, Cn, radius, unique=True, return_metric=True), ref)
    assert np.array_equal(vo.matchFeaturesInRadius(F1, F2, P2, Cn, radius, unique=True), ref[0])


def test_mex_matchradius_through_the_real_library(ctx, vo):
    vo.load_library()                    # torch, then libvo: one HIP runtime in the process
    mex = mexshim.Mex(mexshim.REAL)
    try:
        F1, F2, P2, Cn, radius = rr.case(300, 257, "perrow")
        A, B = F1.astype(F32), F2.astype(F32)
        pairs, metric = mex.call("matchradius", A, B, P2, Cn, radius.reshape(-1, 1), "Unique", True, "MaxRatio", 0.8, nout=2)
        ref_p, ref_m = ctx.match_in_radius(F1, F2, P2, Cn, radius, unique=True, max_ratio=0.8, return_metric=True)
        assert len(ref_p) == len(rr.reference(300, 257, "perrow", 1.0, 0.8, True)[0]) > 0
        assert pairs.dtype == np.uint32 and np.array_equal(pairs, ref_p)
        assert metric.dtype == F32 and metric.shape == (len(ref_p), 1) and np.array_equal(_bits(metric[:, 0]), _bits(ref_m))
        one = mex.call("matchradius", A, B, P2, Cn, np.array([[20.0]], F32))
        assert np.array_equal(one, ctx.match_in_radius(F1, F2, P2, Cn, 20.0))
        with pytest.raises(mexshim.MexError, match="vo:matchFeaturesInRadius:options"):
            mex.call("matchradius", A, B, P2, Cn, radius.reshape(-1, 1), "NoSuchOption", 1.0)
        with pytest.raises(mexshim.MexError, match="vo:badArgument"):
            mex.call("matchradius", A, B, P2, Cn, radius.reshape(-1, 1), "MatchThreshold", 30.0)
        with pytest.raises(mexshim.MexError, match="vo:badArgument"):
            mex.call("matchradius", A, B, P2, Cn, np.array([[-1.0]], F32))
    finally:
        mex.at_exit()
