"""The gateway's `trackpoints` command on the CPU, against the recording fake libvo of tests/mex_shim: the
fake has no vo_track_points, so the weak reference is null and the command must raise
vo:PointTracker:unavailable while the argument-count, output-count and image checks still come first.  The
MATLAB class has the toolbox's methods and goes through the command."""
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


def test_trackpoints_refusals_without_the_entry(mex):
    I = np.zeros((64, 64), np.uint8, order="F")
    x = np.zeros((9, 2), np.float32)
    with pytest.raises(mexshim.MexError) as e:
        mex.call("trackpoints", I, I, x, nout=3)
    assert e.value.ident == "vo:PointTracker:unavailable"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("trackpoints", I, I)
    assert e.value.ident == "vo:nargin"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("trackpoints", I, I, x, nout=4)
    assert e.value.ident == "vo:badArgument"


def test_class_has_the_toolbox_shape():
    src = (Path(__file__).resolve().parent.parent / "matlab" / "voPointTracker.m").read_text()
    assert "classdef voPointTracker < handle" in src and "vo_mex('trackpoints'" in src
    for word in ("function initialize(", "= step(", "function setPoints(", "function release(", "NumPyramidLevels", "BlockSize",
                 "MaxIterations", "MaxBidirectionalError"):
        assert word in src
