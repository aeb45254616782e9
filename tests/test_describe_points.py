"""vo_check_points -- the host-side rules of vo_describe (include/vo.h) -- and the argument handling
of vo.extractFeatures(I, points) as far as it runs without a device.  Each refusal is rejected with
the right first_bad and its neighbour just inside is accepted; the scale bounds come from the CPU
reference's radius expression (tests/describe_ref), not from the library."""
import numpy as np
import pytest

import describe_ref

ROWS, COLS = 112, 168          # upsample 1: 7 octaves (o = 0..6, octave field -1..5); upsample 0: 5


def _pts(vo, n=4, **kw):
    q = np.zeros(n, vo.KP_DTYPE)
    q["x"], q["y"], q["scale"], q["angle"], q["layer"] = 50.0, 40.0, 2.0, 90.0, 1
    q["size"] = 4.0
    for k, v in kw.items():
        q[k] = v
    return q


def _params(vo, L=3, upsample=1):
    p = vo.default_sift_params()
    p.n_octave_layers, p.upsample = L, upsample
    return p


def _first_bad(vo, q, L=3, upsample=1, rows=ROWS, cols=COLS):
    return vo.check_points(q, rows, cols, _params(vo, L, upsample))


def _edge_scl(r):
    """The largest float32 scl whose window radius is r (bisection on the reference's expression)."""
    lo, hi = np.float32(0.0), np.float32(64.0)
    assert describe_ref.radius(lo) <= r < describe_ref.radius(hi)
    while np.nextafter(lo, hi) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if describe_ref.radius(mid) <= r:
            lo = mid
        else:
            hi = mid
    return lo, hi                                      # radius(lo) == r, radius(hi) == r + 1


def _with(vo, i, field, value, **row):
    """Plain points with row i's `field` (and any further fields of that row) replaced."""
    q = _pts(vo)
    q[field][i] = value
    for k, v in row.items():
        q[k][i] = v
    return q


def test_accepts_plain_points_and_an_empty_set(vo, oracle):
    assert _first_bad(vo, _pts(vo)) == -1
    assert _first_bad(vo, _pts(vo, 0)) == -1


@pytest.mark.parametrize("field", ["x", "y", "scale", "angle"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_read_fields_are_refused(vo, field, value):
    assert _first_bad(vo, _with(vo, 2, field, value)) == 2
    q = _with(vo, 2, field, value)
    q[field][1] = value
    assert _first_bad(vo, q) == 1                      # the first offending point


@pytest.mark.parametrize("field", ["size", "response"])
def test_nan_in_ignored_fields_is_accepted(vo, field):
    assert _first_bad(vo, _pts(vo, **{field: np.nan})) == -1


@pytest.mark.parametrize("field", ["x", "y"])
def test_position_bound(vo, field):
    inside = np.nextafter(np.float32(2 ** 20), np.float32(0))
    for sign in (1, -1):
        assert _first_bad(vo, _with(vo, 3, field, sign * np.float32(2 ** 20))) == 3
        assert _first_bad(vo, _with(vo, 3, field, sign * inside)) == -1
    assert _first_bad(vo, _with(vo, 0, field, -300.0)) == -1       # outside the image is legal


def test_angle_bounds(vo):
    assert _first_bad(vo, _with(vo, 1, "angle", 0.0)) == -1
    assert _first_bad(vo, _with(vo, 1, "angle", 360.0)) == -1
    assert _first_bad(vo, _with(vo, 1, "angle", np.float32(359.99))) == -1
    assert _first_bad(vo, _with(vo, 1, "angle", np.nextafter(np.float32(360), np.float32(400)))) == 1
    assert _first_bad(vo, _with(vo, 1, "angle", -np.nextafter(np.float32(0), np.float32(1)))) == 1
    assert _first_bad(vo, _with(vo, 1, "angle", -0.0)) == -1


@pytest.mark.parametrize("upsample", [1, 0])
def test_octave_bounds(vo, oracle, upsample):
    n_oct = oracle.lib().oracle_num_octaves(ROWS, COLS, upsample)
    assert n_oct == (7 if upsample else 5)             # cvRound(log2(min side of the base) - 2) + upsample
    lo, hi = -upsample, n_oct - 1 - upsample           # octave field of planes 0 and n_oct - 1
    scale = lambda o: 2.0 * 2.0 ** o                   # keep the octave-relative scale at 2
    for o in (lo, hi):
        assert _first_bad(vo, _with(vo, 2, "octave", o, scale=scale(o)), upsample=upsample) == -1
    assert _first_bad(vo, _with(vo, 2, "octave", lo - 1, scale=scale(lo)), upsample=upsample) == 2
    assert _first_bad(vo, _with(vo, 2, "octave", hi + 1, scale=scale(hi)), upsample=upsample) == 2
    assert _first_bad(vo, _with(vo, 0, "octave", -2, scale=1.0), upsample=1) == 0       # octave -2 with upsample
    assert _first_bad(vo, _with(vo, 0, "octave", -1, scale=1.0), upsample=0) == 0
    for o in (2 ** 31 - 1, -2 ** 31):
        assert _first_bad(vo, _with(vo, 1, "octave", o), upsample=upsample) == 1


@pytest.mark.parametrize("L", [1, 3, 5])
def test_layer_bounds(vo, L):
    for layer in range(0, L + 3):
        assert _first_bad(vo, _with(vo, 3, "layer", layer), L=L) == -1
    assert _first_bad(vo, _with(vo, 3, "layer", -1), L=L) == 3
    assert _first_bad(vo, _with(vo, 3, "layer", L + 3), L=L) == 3


@pytest.mark.parametrize("octave,upsample", [(-1, 1), (0, 1), (4, 1), (0, 0), (3, 0)])
def test_radius_bounds(vo, octave, upsample):
    """Radius 0 against 1 and 127 against 128, at the octave-relative scale: the keypoint's scale is
    scl * oscale, a power-of-two multiple, so the edge moves with the octave exactly."""
    oscale = np.float32(2.0 ** (octave + upsample) * (0.5 if upsample else 1.0))
    last0, first1 = _edge_scl(0)
    last127, first128 = _edge_scl(127)
    assert describe_ref.radius(first1) == 1 and describe_ref.radius(last127) == 127
    for scl, ok in ((last0, False), (first1, True), (last127, True), (first128, False)):
        q = _with(vo, 1, "scale", scl * oscale, octave=octave)
        assert _first_bad(vo, q, upsample=upsample) == (-1 if ok else 1), (scl, ok)
    for scl in (0.0, -2.0, np.float32(3e38)):
        assert _first_bad(vo, _with(vo, 1, "scale", scl, octave=octave), upsample=upsample) == 1


def test_bad_call_arguments(vo):
    import ctypes as C
    lib = vo.load_library()
    q = _pts(vo)
    kp = q.ctypes.data_as(C.POINTER(vo.Keypoint))
    p = _params(vo)
    bad = C.c_int(7)
    assert lib.vo_check_points(None, ROWS, COLS, kp, 4, C.byref(bad)) == vo.VO_ERR_ARG and bad.value == -1
    assert lib.vo_check_points(C.byref(p), ROWS, COLS, None, 4, C.byref(bad)) == vo.VO_ERR_ARG and bad.value == -1
    assert lib.vo_check_points(C.byref(p), ROWS, COLS, kp, -1, C.byref(bad)) == vo.VO_ERR_ARG and bad.value == -1
    assert lib.vo_check_points(C.byref(p), 0, COLS, kp, 4, C.byref(bad)) == vo.VO_ERR_ARG and bad.value == -1
    assert lib.vo_check_points(C.byref(p), ROWS, COLS, kp, 4, None) == vo.VO_OK          # first_bad may be NULL
    assert lib.vo_check_points(C.byref(p), ROWS, COLS, None, 0, C.byref(bad)) == vo.VO_OK
    with pytest.raises(vo.VOError):
        vo.check_points(q, 0, COLS)


# ---- vo.as_keypoints / vo.extractFeatures(I, points): what runs without a device ----

def test_as_keypoints_forms(vo):
    q = _pts(vo)
    assert vo.as_keypoints(q) is q or np.array_equal(vo.as_keypoints(q), q)
    cols = vo.as_keypoints({"x": [1.0, 2.0], "y": [3.0, 4.0], "scale": [2.0, 3.0]})
    assert cols.dtype == vo.KP_DTYPE and len(cols) == 2
    assert np.array_equal(cols["layer"], [0, 0]) and np.array_equal(cols["octave"], [0, 0])      # hand-built: level 0
    assert np.array_equal(cols["angle"], [0, 0]) and np.array_equal(cols["size"], [4.0, 6.0])
    sub = np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4"), ("scale", "<f4"), ("angle", "<f4")]))
    assert vo.as_keypoints(sub).dtype == vo.KP_DTYPE
    for bad in ([1, 2, 3], np.zeros((3, 2), np.float32), {"x": [1.0], "y": [1.0]}, {"x": [1.0], "y": [1.0], "scale": [1.0], "z": [0]},
                {"x": [1.0, 2.0], "y": [1.0], "scale": [1.0]}, np.zeros((2, 2), vo.KP_DTYPE)):
        with pytest.raises(vo.VOError) as e:
            vo.as_keypoints(bad)
        assert e.value.code == vo.VO_ERR_ARG


def test_extract_features_argument_handling_without_a_device(vo):
    I = np.zeros((64, 64), np.uint8)
    q = _pts(vo)
    for call in (lambda: vo.extractFeatures(I, q, Method="SURF"),
                 lambda: vo.extractFeatures(I, q, strongest=3),
                 lambda: vo.extractFeatures(I, [[1.0, 2.0]]),
                 lambda: vo.extractFeatures(np.zeros((4, 64, 64), np.uint8), q),
                 lambda: vo.extractFeatures(I.astype(np.float32), q)):
        with pytest.raises(vo.VOError) as e:
            call()
        assert e.value.code == vo.VO_ERR_ARG


def test_gateway_linked_without_vo_describe_says_so():
    """vo_mex('describe', ...) reaches libvo through a weak reference: a gateway linked with a libvo
    that lacks vo_describe (here the recording fake of tests/mex_shim) still loads, checks the
    argument count and classes, and raises vo:extractFeatures:unavailable."""
    import mexshim
    mexshim.build()
    m = mexshim.Mex(mexshim.FAKE)
    img = np.zeros((32, 48), np.uint8)
    col = lambda v, dt=np.float32: np.array(v, dt).reshape(-1, 1)
    with pytest.raises(mexshim.MexError) as e:
        m.call("describe", img, np.array([[5.0, 6.0]], np.float32), col([2.0]), col([0.1]), col([0], np.int32), col([1], np.int32))
    assert e.value.ident == "vo:extractFeatures:unavailable"
    with pytest.raises(mexshim.MexError) as e:
        m.call("describe", img, np.array([[5.0, 6.0]], np.float32))
    assert e.value.ident == "vo:nargin"
    m.at_exit()
