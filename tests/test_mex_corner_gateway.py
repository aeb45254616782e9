"""The gateway's `corners` command on the CPU, against the recording fake libvo of tests/mex_shim: the fake has no
vo_detect_corners, so the weak reference is null and the command must raise vo:cornerPoints:unavailable while
the argument-count, output-count and image checks still come first.  The MATLAB wrappers have the toolbox's
names and options and go through the command."""
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


def test_corners_refusals_without_the_entry(mex):
    I = np.zeros((64, 64), np.uint8, order="F")
    with pytest.raises(mexshim.MexError) as e:
        mex.call("corners", I, nout=2)
    assert e.value.ident == "vo:cornerPoints:unavailable"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("corners")
    assert e.value.ident == "vo:nargin"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("corners", I, np.zeros((1, 8)), np.zeros((1, 8)))
    assert e.value.ident == "vo:nargin"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("corners", I, nout=3)
    assert e.value.ident == "vo:badArgument"


@pytest.mark.parametrize("name,method", [("detectMinEigenFeatures", "opts = [0,"), ("detectHarrisFeatures", "opts = [1,")])
def test_wrappers_have_the_toolbox_shape(name, method):
    src = (Path(__file__).resolve().parent.parent / "matlab" / (name + ".m")).read_text()
    assert src.startswith(f"function points = {name}(I, varargin)") and "vo_mex('corners'" in src and method in src
    for word in ("MinQuality", "FilterSize", "ROI", 'cornerPoints(Location, "Metric", Metric)'):
        assert word in src
