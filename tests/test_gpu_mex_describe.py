"""vo_mex('describe', I, loc, scale, ori, octave, layer) through the real gateway (matlab/vo_mex.c
built against tests/mex_shim's mx-API, linked to the real libvo): MATLAB column-major inputs, the
SIFTPoints properties as MATLAB holds them (Orientation in radians), against Context.describe on the
same points converted as the gateway converts them and against tests/describe_ref."""
import numpy as np
import pytest

import describe_ref
import mexshim

pytestmark = pytest.mark.gpu

ROWS, COLS = 112, 168


@pytest.fixture(scope="module")
def mex(vo):
    vo.load_library()                    # torch, then libvo: one HIP runtime in the process
    m = mexshim.Mex(mexshim.REAL)
    yield m
    m.at_exit()


def _mex_args(q):
    """SIFTPoints properties of keypoint rows: Location, Scale, Orientation (radians, single), Octave, Layer"""
    loc = np.stack([q["x"], q["y"]], 1).astype(np.float32)
    ori = (q["angle"].astype(np.float64) * (np.pi / 180)).astype(np.float32)
    return (loc, q["scale"].reshape(-1, 1), ori.reshape(-1, 1), q["octave"].astype(np.int32).reshape(-1, 1),
            q["layer"].astype(np.int32).reshape(-1, 1))


def _as_gateway_converts(q, ori):
    """the keypoint rows the gateway hands to vo_describe: degrees = (float)((double)ori * (180 / pi))"""
    g = q.copy()
    g["angle"] = (ori.reshape(-1).astype(np.float64) * (180.0 / np.pi)).astype(np.float32)
    return g


def test_mex_describe(mex, vo, oracle, syn):
    img = syn.stereo_pair(syn.SEED_BASE + 11, ROWS, COLS)[0]
    ctx = vo.Context(ROWS, COLS, 1)
    kps, _ = ctx.sift(img)
    rng = np.random.default_rng(3)
    q = np.concatenate([kps, kps])
    n = len(kps)
    q["x"][n:] += rng.uniform(-2, 2, n).astype(np.float32)
    q["y"][n:] += rng.uniform(-2, 2, n).astype(np.float32)
    q["scale"][n:] *= np.float32(1.5)
    q["angle"][n:] = rng.uniform(0, 359, n).astype(np.float32)
    q["layer"][n:] = rng.integers(0, 6, n)
    args = _mex_args(q)
    got = mex.call("describe", np.asfortranarray(img), *args)
    assert got.dtype == np.float32 and got.shape == (len(q), 128)
    g = _as_gateway_converts(q, args[2])
    assert ((g["angle"] >= 0) & (g["angle"] <= 360)).all()
    want = ctx.describe(img, g)
    assert np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(want, describe_ref.describe(img, g, oracle.sift_params()))
    # Scale / Orientation as double columns and Octave / Layer as double: the same rows
    dbl = mex.call("describe", img, args[0].astype(np.float64), args[1].astype(np.float64), args[2].astype(np.float64),
                   args[3].astype(np.float64), args[4].astype(np.float64))
    assert np.array_equal(dbl, got)
    empty = mex.call("describe", img, np.zeros((0, 2), np.float32), np.zeros((0, 1), np.float32), np.zeros((0, 1), np.float32),
                     np.zeros((0, 1), np.int32), np.zeros((0, 1), np.int32))
    assert empty.shape == (0, 128)
    ctx.close()


def test_mex_describe_refusals(mex, vo, syn):
    img = syn.stereo_pair(syn.SEED_BASE + 11, ROWS, COLS)[0]
    loc = np.array([[50.0, 40.0], [60.0, 45.0]], np.float32)
    col = lambda v, dt=np.float32: np.array(v, dt).reshape(-1, 1)
    good = (loc, col([2.0, 2.0]), col([0.5, 1.0]), col([0, 0], np.int32), col([1, 1], np.int32))
    assert mex.call("describe", img, *good).shape == (2, 128)
    for k, bad in ((1, col([2.0, 200.0])), (2, col([0.5, 7.0])), (3, col([0, 9], np.int32)), (4, col([1, 6], np.int32)),
                   (0, np.array([[50.0, 40.0], [np.nan, 45.0]], np.float32))):
        args = list(good)
        args[k] = bad
        with pytest.raises(mexshim.MexError) as e:
            mex.call("describe", img, *args)
        assert e.value.ident == "vo:badArgument" and "point 1" in str(e.value), str(e.value)
    with pytest.raises(mexshim.MexError) as e:
        mex.call("describe", img, loc, col([2.0]), good[2], good[3], good[4])
    assert e.value.ident == "vo:badArgument"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("describe", img, loc)
    assert e.value.ident == "vo:nargin"
