"""The pin of vo_describe's spec (include/vo.h, "extractFeatures at caller-given points"): the CPU
reference tests/describe_ref -- the oracle's build_pyramid and descriptor behind the inverse of
oracle_sift's output mapping -- reproduces oracle.sift's descriptors from the public fields of
oracle.sift's own keypoints, with zero mismatching rows.  x, y and scale therefore carry enough to
rebuild descriptor()'s inputs (the equality could only break at a .5 rounding tie of xo or yo; the
images below hit none, so no seed had to be changed)."""
import re
from pathlib import Path

import numpy as np
import pytest

import describe_ref

ROOT = Path(__file__).resolve().parent.parent

# (rows, cols, n_octave_layers, upsample)
PIN_CASES = [(112, 168, 3, 1), (112, 168, 3, 0), (188, 621, 3, 1), (188, 621, 3, 0), (112, 168, 2, 1)]


def test_reference_is_built_with_the_oracle_flags():
    def cflags(p):
        return re.search(r"^CFLAGS \?= (.*)$", p.read_text(), flags=re.M).group(1).split()
    assert cflags(ROOT / "tests" / "describe_ref" / "Makefile") == cflags(ROOT / "oracle" / "Makefile")


@pytest.mark.parametrize("rows,cols,L,upsample", PIN_CASES)
def test_reference_reproduces_the_oracles_own_descriptors(oracle, syn, rows, cols, L, upsample):
    img, _ = syn.stereo_pair(syn.SEED_BASE + 11, rows, cols)
    p = oracle.sift_params()
    p.n_octave_layers, p.upsample = L, upsample
    kps, desc = oracle.sift(img, p)
    assert len(kps) >= 20                              # (not vacuous)
    got = describe_ref.describe(img, kps, p)
    bad = np.flatnonzero((got != desc).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} of {len(kps)} rows differ, first {bad[:5]}"


def test_reference_ignores_size_and_response(oracle, syn):
    img, _ = syn.stereo_pair(syn.SEED_BASE + 11, 112, 168)
    kps, desc = oracle.sift(img)
    q = kps.copy()
    q["size"] = np.nan
    q["response"] = -1.0
    assert np.array_equal(describe_ref.describe(img, q), desc)


def test_reference_window_without_a_sample_is_all_zero(oracle, syn):
    img, _ = syn.stereo_pair(syn.SEED_BASE + 11, 112, 168)
    q = np.zeros(2, oracle.KP_DTYPE)
    q["x"], q["y"], q["scale"], q["layer"] = [-500.0, 1000.0], [50.0, 900.0], 2.0, 1
    assert not describe_ref.describe(img, q).any()


def test_reference_radius_bounds():
    """The scale bounds of vo.h: radius 1 .. 127 is about 0.1 <= scl <= 11.9."""
    assert describe_ref.radius(0.1) == 1 and describe_ref.radius(0.04) == 0
    assert describe_ref.radius(11.9) == 126 and describe_ref.radius(12.0) == 127 and describe_ref.radius(12.1) == 128
