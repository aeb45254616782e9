"""The gateway's `disparitysgm` and `reconstructscene` commands on the CPU, against the recording fake libvo of
tests/mex_shim: the fake has neither entry, so the weak references are null and the commands must raise
vo:disparitySGM:unavailable -- after the argument-count, output-count and image checks, which still come first.
The MATLAB shadows have the toolbox's names and options and go through the commands."""
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


def _ident(mex, *args, nout=1):
    with pytest.raises(mexshim.MexError) as e:
        mex.call(*args, nout=nout)
    return e.value.ident


def test_disparitysgm_checks_come_before_unavailable(mex):
    I = np.zeros((32, 48), np.uint8, order="F")
    assert _ident(mex, "disparitysgm", I, I) == "vo:disparitySGM:unavailable"
    assert _ident(mex, "disparitysgm", I, I, np.array([[0.0, 64.0, 15.0]])) == "vo:disparitySGM:unavailable"
    assert _ident(mex, "disparitysgm", I, I, np.array([[0.0, 64.0, 15.0, 10.0, 120.0]])) == "vo:disparitySGM:unavailable"
    assert _ident(mex, "disparitysgm") == "vo:nargin"
    assert _ident(mex, "disparitysgm", I) == "vo:nargin"
    assert _ident(mex, "disparitysgm", I, I, np.zeros((1, 3)), np.zeros((1, 3))) == "vo:nargin"
    assert _ident(mex, "disparitysgm", I, I, nout=2) == "vo:badArgument"
    assert _ident(mex, "disparitysgm", I.astype(np.float64), I) == "vo:badArgument"
    assert _ident(mex, "disparitysgm", I, np.zeros((32, 47), np.uint8, order="F")) == "vo:badArgument"
    assert _ident(mex, "disparitysgm", I, I, np.zeros((1, 4))) == "vo:badArgument"
    assert _ident(mex, "disparitysgm", I, I, np.zeros((1, 3), np.float32)) == "vo:badArgument"


def test_reconstructscene_checks_come_before_unavailable(mex):
    D = np.zeros((32, 48), np.float32, order="F")
    Q = np.eye(4)
    assert _ident(mex, "reconstructscene", D, Q) == "vo:disparitySGM:unavailable"
    assert _ident(mex, "reconstructscene", D) == "vo:nargin"
    assert _ident(mex, "reconstructscene", D, Q, Q) == "vo:nargin"
    assert _ident(mex, "reconstructscene", D, Q, nout=2) == "vo:badArgument"
    assert _ident(mex, "reconstructscene", D.astype(np.float64), Q) == "vo:badArgument"
    assert _ident(mex, "reconstructscene", D, np.eye(3)) == "vo:badArgument"
    assert _ident(mex, "reconstructscene", D, Q.astype(np.float32)) == "vo:badArgument"


def test_shadows_have_the_toolbox_shape():
    matlab = Path(__file__).resolve().parent.parent / "matlab"
    src = (matlab / "disparitySGM.m").read_text()
    assert src.startswith("function disparityMap = disparitySGM(I1, I2, varargin)") and "vo_mex('disparitysgm'" in src
    for word in ("DisparityRange", "UniquenessThreshold", "inputParser", "[0 128]", "15"):
        assert word in src
    assert "KeepUnmatched" not in src                                    # inputParser refuses any other name by name
    src = (matlab / "reconstructScene.m").read_text()
    assert src.startswith("function xyzPoints = reconstructScene(disparityMap, reprojectionMatrix, varargin)")
    for word in ("vo_mex('reconstructscene'", "vo:reconstructScene:options", "reshape(xyz, size(disparityMap, 1), size(disparityMap, 2), 3)"):
        assert word in src
