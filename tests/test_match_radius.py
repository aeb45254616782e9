"""matchFeaturesInRadius on the CPU: the numpy restatement (tests/match_radius_ref.py) against
match_ref.match where the gate admits everything and against a per-row loop, the census of the
generated cases (every class the GPU test relies on is present, asserted on the reference alone),
the CPU build of vo_spec.h's gate and box bound against numpy, the box bound's conservativeness in
float32, and the MEX gateway's 'matchradius' command on the fake libvo."""
import numpy as np
import pytest

import match_radius_ref as rr
import match_ref as mr
import mexshim

F32 = np.float32
CASES = [(n1, n2, lay) for (n1, n2) in rr.SHAPES for lay in rr.LAYOUTS] + [(4100, 4100, "sorted")]


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("n1,n2", [(33, 129), (129, 33), (300, 257)])
def test_huge_radius_is_plain_matchfeatures(n1, n2):
    F1, F2, P2, Cn, _ = rr.case(n1, n2, "perrow")
    assert rr.gate(P2, Cn, np.full(n1, 1e6, F32)).all()
    for thr, ratio in mr.OPTIONS:
        for unique in (False, True):
            p, m = rr.match(F1, F2, P2, Cn, np.full(n1, 1e6, F32), thr, ratio, unique)
            q, k = mr.match(F1, F2, thr, ratio, unique)
            assert np.array_equal(p, q) and np.array_equal(_bits(m), _bits(k)), (thr, ratio, unique)
            p, m = rr.match(F1, F2, P2, Cn, np.array([1e6], F32), thr, ratio, unique)
            assert np.array_equal(p, q) and np.array_equal(_bits(m), _bits(k)), (thr, ratio, unique)


def _loop_match(F1, F2, P2, Cn, radius, thr, ratio, unique):
    """The spec row by row, scalar float32 arithmetic."""
    sv = mr.scores(F1, F2)
    n1, n2 = sv.shape
    r = np.broadcast_to(np.asarray(radius, F32).reshape(-1), (n1,)) if np.size(radius) == 1 else np.asarray(radius, F32)
    T = F32(thr) * F32(0.04)

    def inside(i, j):
        dx, dy = F32(P2[j, 0] - Cn[i, 0]), F32(P2[j, 1] - Cn[i, 1])
        return F32(F32(dx * dx) + F32(dy * dy)) <= F32(r[i] * r[i])

    out, met = [], []
    for i in range(n1):
        cand = [j for j in range(n2) if inside(i, j)]
        if not cand:
            continue
        order = sorted(cand, key=lambda j: (sv[i, j], j))
        best = sv[i, order[0]]
        second = sv[i, order[1]] if len(order) > 1 else F32(np.inf)
        with np.errstate(invalid="ignore", divide="ignore"):
            if not (best <= T and F32(best / second) <= F32(ratio)):
                continue
        j = order[0]
        if unique:
            rows = [a for a in range(n1) if inside(a, j)]
            if min(rows, key=lambda a: (sv[a, j], a)) != i:
                continue
        out.append((i + 1, j + 1))
        met.append(best)
    return np.array(out, np.uint32).reshape(-1, 2), np.array(met, F32)


@pytest.mark.parametrize("layout", rr.LAYOUTS)
def test_row_loop_equals_the_vectorised_restatement(layout):
    F1, F2, P2, Cn, radius = rr.case(33, 129, layout)
    for thr, ratio in mr.OPTIONS:
        for unique in (False, True):
            p, m = _loop_match(F1, F2, P2, Cn, radius, thr, ratio, unique)
            q, k = rr.reference(33, 129, layout, thr, ratio, unique)
            assert len(q) and np.array_equal(p, q) and np.array_equal(_bits(m), _bits(k)), (thr, ratio, unique)


@pytest.mark.parametrize("n1,n2,layout", CASES)
def test_census(n1, n2, layout):
    c = rr.census(n1, n2, layout)
    print(n1, n2, layout, c)
    for k in rr.census_required(n1, n2, layout):
        assert c[k] > 0, (k, c)


@pytest.mark.parametrize("n1,n2,layout", CASES)
def test_c_gate_and_box_bound_equal_numpy_and_the_bound_holds(n1, n2, layout):
    _, _, P2, Cn, radius = rr.case(n1, n2, layout)
    g = rr.gate(P2, Cn, radius)
    assert np.array_equal(rr.gate_c(P2, Cn, radius), g)
    for pts, other in ((P2, Cn), (Cn, P2)):              # forward: tiles of points; backward: tiles of centres
        boxes = rr.tile_boxes(pts)
        lb = rr.box_lb(boxes, other)
        assert np.array_equal(_bits(rr.box_lb_c(boxes, other)), _bits(lb))
        dx = pts[None, :, 0] - other[:, None, 0]
        dy = pts[None, :, 1] - other[:, None, 1]
        d2 = dx * dx + dy * dy
        assert d2.dtype == F32
        for t in range(len(boxes)):
            assert (lb[:, t:t + 1] <= d2[:, 32 * t:32 * t + 32]).all(), t


def _bound_holds(pts, other):
    """box_lb of the one box of pts against every point of other <= d2 with either operand order."""
    box = rr.tile_boxes(pts)[:1] if len(pts) <= 32 else np.array([[pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max()]], F32)
    with np.errstate(over="ignore", invalid="ignore"):
        lb = rr.box_lb_c(box, other)
        assert np.array_equal(_bits(lb), _bits(rr.box_lb(box, other)))
        for a, b in ((pts[None], other[:, None]), (other[:, None], pts[None])):
            dx, dy = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1]
            d2 = dx * dx + dy * dy
            assert d2.dtype == F32 and not np.isnan(lb).any()
            assert (lb <= d2).all()


def test_box_bound_on_random_and_extreme_tiles():
    rng = np.random.default_rng(5)
    for _ in range(2000):                                 # random tiles: arbitrary float32 values, not on a grid
        scale = F32(10.0 ** rng.integers(-3, 6))
        pts = (rng.normal(size=(32, 2)) * scale + rng.normal(size=2) * scale).astype(F32)
        other = (rng.normal(size=(32, 2)) * scale * 2).astype(F32)
        _bound_holds(pts, other)
    big = (rng.uniform(-1, 1, (32, 2)) * 1e30).astype(F32)
    _bound_holds(big, (rng.uniform(-1, 1, (64, 2)) * 1e30).astype(F32))            # d2 overflows to +inf on both sides
    _bound_holds(big, rng.uniform(-1, 1, (64, 2)).astype(F32))
    _bound_holds(-np.abs(big), np.abs(big))                                         # negative coordinates
    _bound_holds((rng.uniform(-2000, -1000, (32, 2))).astype(F32), rng.uniform(-3000, 0, (64, 2)).astype(F32))
    same = np.full((32, 2), F32(417.25))
    _bound_holds(same, rng.uniform(0, 1000, (64, 2)).astype(F32))                   # all equal: a degenerate box
    _bound_holds(same, same[:3])


@pytest.fixture(scope="module")
def mex():
    mexshim.build()
    m = mexshim.Mex(mexshim.FAKE)
    yield m
    m.at_exit()


def _mex_args(n1=5, n2=7):
    rng = np.random.default_rng(3)
    F1 = rng.integers(0, 256, (n1, 128)).astype(F32)
    F2 = rng.integers(0, 256, (n2, 128)).astype(F32)
    return F1, F2, rng.uniform(0, 100, (n2, 2)).astype(F32), rng.uniform(0, 100, (n1, 2)).astype(F32)


def test_mex_matchradius_unavailable_on_an_older_libvo(mex):
    F1, F2, P2, Cn = _mex_args()
    with pytest.raises(mexshim.MexError, match="vo:matchFeaturesInRadius:unavailable"):
        mex.call("matchradius", F1, F2, P2, Cn, np.array([[5.0]], F32))
    with pytest.raises(mexshim.MexError, match="vo:matchFeaturesInRadius:unavailable"):
        mex.call("matchradius", F1, F2, P2, Cn, np.full((5, 1), 5.0, F32), "Unique", True, nout=2)
    with pytest.raises(mexshim.MexError, match="vo:matchFeaturesInRadius:options"):
        mex.call("matchradius", F1, F2, P2, Cn, np.array([[5.0]], F32), "NoSuchOption", 1.0)
    assert mex.call("match", F1, F2).shape[1] == 2       # the other commands run as before


def test_mex_matchradius_refuses_wrong_shapes_before_libvo(mex):
    F1, F2, P2, Cn = _mex_args()
    r = np.array([[5.0]], F32)
    for args in ((F1, F2, P2[:6], Cn, r), (F1, F2, P2.T.copy(), Cn, r), (F1, F2, P2, Cn[:4], r),
                 (F1, F2, P2, Cn, np.full((2, 1), 5.0, F32)), (F1, F2, P2, Cn, np.full((5, 2), 5.0, F32)),
                 (F1, F2, P2.astype(np.float64), Cn, r), (F1[:, :64], F2, P2, Cn, r)):
        with pytest.raises(mexshim.MexError, match="vo:badArgument"):
            mex.call("matchradius", *args)
    with pytest.raises(mexshim.MexError, match="vo:nargin"):
        mex.call("matchradius", F1, F2, P2, Cn)
