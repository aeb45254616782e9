"""The gateway's `refinepose` command on the CPU, against the recording fake libvo of tests/mex_shim:
the fake has no vo_refine_pose, so the weak reference is null and the command must raise
vo:bundleAdjustmentMotion:unavailable while the argument-count and output-count checks still come first."""
import numpy as np
import pytest

import mexshim


@pytest.fixture(scope="module")
def mex():
    mexshim.build()
    m = mexshim.Mex(mexshim.FAKE)
    yield m
    m.at_exit()


def test_refinepose_is_unavailable_without_the_entry(mex):
    Xw, uv, A, K = np.zeros((5, 3)), np.zeros((5, 2)), np.eye(4), np.eye(3)
    with pytest.raises(mexshim.MexError) as e:
        mex.call("refinepose", Xw, uv, A, K, nout=2)
    assert e.value.ident == "vo:bundleAdjustmentMotion:unavailable"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("refinepose", Xw, uv, A)
    assert e.value.ident == "vo:nargin"
    with pytest.raises(mexshim.MexError) as e:
        mex.call("refinepose", Xw, uv, A, K, nout=3)
    assert e.value.ident == "vo:badArgument"
