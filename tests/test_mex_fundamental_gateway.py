"""The gateway's `fundamental` command on the CPU, against the recording fake libvo of tests/mex_shim:
the fake has no vo_est_fundamental, so the weak reference is null and the command must raise
vo:estimateFundamentalMatrix:unavailable while the argument-count and output-count checks still come
first.  The MATLAB shadow names every option it hands back to the toolbox."""
from pathlib import Path

import numpy as np
import pytest

import mexshim


@pytest.fixture(scope="module")
def mex():
    mexshim.build()
    m = mexshim.Mex(mexshim.FAKE)
    yield m
    m.at_exit()


def test_fundamental_is_unavailable_without_the_entry(mex):
    x = np.zeros((9, 2), np.float32)
    with pytest.raises(mexshim.MexError) as e:
        mex.call("fundamental", x, x, nout=3)
    assert e.value.ident == "vo:estimateFundamentalMatrix:unavailable"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("fundamental", x)
    assert e.value.ident == "vo:nargin"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("fundamental", x, x, nout=4)
    assert e.value.ident == "vo:badArgument"


def test_shadow_hands_unimplemented_options_back():
    src = (Path(__file__).resolve().parent.parent / "matlab" / "estimateFundamentalMatrix.m").read_text()
    assert "vo_mex('fundamental'" in src and "vo:estimateFundamentalMatrix:options" in src
    for word in ("RANSAC", "LMedS", "LTS", "Algebraic", "InlierPercentage", "toolbox''s estimateFundamentalMatrix"):
        assert word in src
