"""matchFeatures options (Unique, MatchThreshold, MaxRatio, matchMetric) on the CPU: the numpy
restatement of the spec (tests/match_ref.py) is pinned to the frozen oracle, the test inputs
are shown to exercise the Unique rule (pairs dropped, pairs kept, columns decided by index), the
crowded-column inputs separate the spec's operand order from the swapped one, and the MEX
gateway linked to a libvo without vo_match_f32_ex (the recording fake) refuses options cleanly.
tests/test_gpu_match_options.py checks libvo against the same restatement on the GPU."""
import ctypes as C

import numpy as np
import pytest

import match_ref as mr
import mexshim


@pytest.mark.parametrize("n1,n2", mr.SHAPES + mr.DEGENERATE)
def test_restatement_equals_the_oracle_without_unique(oracle, n1, n2):
    F1, F2 = mr.features(n1, n2)
    for thr, ratio in mr.OPTIONS:
        pairs, metric = mr.reference(n1, n2, thr, ratio, False)
        assert np.array_equal(pairs, oracle.match(F1, F2, oracle.MatchParams(thr, ratio))), (thr, ratio)
        assert metric.dtype == np.float32 and len(metric) == len(pairs)


@pytest.mark.parametrize("n1,n2", mr.SHAPES)
def test_inputs_exercise_the_unique_rule(n1, n2):
    """Conditions on the inputs, not measurements: Unique drops a pair, keeps a pair, and some
    column's winner is decided by the lowest index among equal scores."""
    for thr, ratio in mr.OPTIONS:
        fwd, _ = mr.reference(n1, n2, thr, ratio, False)
        uni, _ = mr.reference(n1, n2, thr, ratio, True)
        assert 1 <= len(uni) < len(fwd), (thr, ratio)
        assert set(map(tuple, uni)) <= set(map(tuple, fwd))
        assert np.all(np.diff(uni[:, 0].astype(np.int64)) > 0)            # ascending in F1
        assert len(np.unique(uni[:, 1])) == len(uni)                       # one pair per F2 row
        assert mr.index_decided_columns(*mr.features(n1, n2), thr, ratio) >= 1


def test_crowded_column_separates_the_operand_orders():
    """512 near-copies of one F2 row: scoring the backward pass as (dot * inv|F2|) * inv|F1|
    (the forward kernel with its sides exchanged) picks another winner than the spec's order."""
    F1, F2 = mr.crowded()
    spec, _ = mr.match(F1, F2, unique=True)
    swapped, _ = mr.match(F1, F2, unique=True, swapped_back=True)
    assert len(spec) == 1 and len(swapped) == 1 and spec[0, 1] == 18
    assert not np.array_equal(spec, swapped)
    c_spec, c_swap = mr.scores(F1, F2)[:, 17], mr.scores(F1, F2, swapped=True)[:, 17]
    assert 0.2 < np.mean(c_spec != c_swap) < 0.6                            # an ulp apart on about a third


def test_chunk_tie_inputs():
    F1, F2 = mr.chunk_tie_rows()
    assert mr.match(F1, F2)[0].tolist() == [[11, 6], [4100, 6]]
    assert mr.match(F1, F2, unique=True)[0].tolist() == [[11, 6]]
    F1, F2 = mr.chunk_tie_cols()
    fwd, uni = mr.match(F1, F2)[0], mr.match(F1, F2, unique=True)[0]
    assert fwd[:, 0].tolist() == [4, 41] and fwd[:, 1].tolist() == [4099, 4099] and len(uni) == 1


# ---- the MEX gateway against a libvo without vo_match_f32_ex (the recording fake) ----
@pytest.fixture(scope="module")
def mex():
    mexshim.build()
    m = mexshim.Mex(mexshim.FAKE)
    m.L.fake_int.argtypes = [C.c_char_p]
    yield m
    m.at_exit()


def test_gateway_plain_match_still_uses_vo_match_f32(mex):
    rng = np.random.default_rng(2)
    F1 = rng.integers(0, 256, (7, 128)).astype(np.float32)
    F2 = rng.integers(0, 256, (6, 128)).astype(np.float32)
    pairs = mex.call("match", F1, F2)
    assert (mex.L.fake_int(b"n1"), mex.L.fake_int(b"n2"), mex.L.fake_int(b"col_major")) == (7, 6, 1)
    assert np.array_equal(pairs, [[1, 6], [3, 4], [5, 2]])
    # options that only restate a default change nothing
    assert np.array_equal(mex.call("match", F1, F2, "Method", "Exhaustive", "metric", "ssd", "Prenormalized", False), pairs)


def test_gateway_refuses_options_without_the_entry_point(mex):
    F = np.zeros((3, 128), np.float32)
    for args, nout in ((("Unique", True), 1), ((), 2), (("NoSuchOption", 1.0), 1), (("MaxRatio", 0.8), 1),
                       (("MatchThreshold", np.float32(5)), 1), (("Method", "Approximate"), 1), (("Metric", "SAD"), 1),
                       (("Prenormalized", True), 1), (("Unique",), 1), (("MaxRatio", "x"), 1), (("Unique", True), 3)):
        with pytest.raises(mexshim.MexError, match="vo:matchFeatures:options"):
            mex.call("match", F, F, *args, nout=nout)
