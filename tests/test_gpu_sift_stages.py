"""The feature kernels after the scale space -- k_ext_inner, k_seg_*, k_refine, k_orient, k_desc --
on the fixture images of tests/sift_edge_images.py, whose census (taken with the float64 reference
tests/sift_f64_ref.py, which tests/test_sift_f64_ref.py holds the oracle to) says which branches
they reach: candidates on the border rows and columns, every way a candidate dies, windows clipped
by every image side, histogram wrap, multi-peak keypoints, the descriptor radius cap.

One context per parameter set at 96 x 144; all fixture images go through one
sift_match_batch_dev call as the left and right images of consecutive frames, so every image sits
in another slot of the batch (image 2 f + side = its index in sift_edge_images.images()).

vo_fetch_candidate_counts is held to expected values here: its n_cand is the number of centres
that pass |val| > threshold and the extremum test within the DoG levels 1..L (include/vo.h), which
is what oracle_sift_trace lists and the reference's candidates() counts; n_acc the accepted ones.
The fixture images hold no candidate whose outcome float32 rounding could turn, so both are exact.
"""
import numpy as np
import pytest

import sift_edge_images as E

pytestmark = pytest.mark.gpu

KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "layer", "scale")


def _same_kps(a, b, what=""):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in KP_FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f)


@pytest.fixture(scope="module", params=E.PARAM_SETS, ids=lambda p: f"L{p[0]}-up{p[1]}")
def batch(request, vo, oracle):
    """(L, upsample, context after the batched call, oracle.sift per image, oracle trace per image)."""
    import torch
    L, up = request.param
    imgs = [im for _, im in E.images()]
    B = len(imgs) // 2
    ctx = vo.Context(E.ROWS, E.COLS, B, sift=E.sift_params(vo, L, up))
    dl = torch.from_numpy(np.ascontiguousarray(np.stack(imgs[0::2]))).cuda()
    dr = torch.from_numpy(np.ascontiguousarray(np.stack(imgs[1::2]))).cuda()
    torch.cuda.synchronize()
    ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), B, stats=False)
    p = E.sift_params(oracle, L, up)
    yield L, up, ctx, [oracle.sift(im, p) for im in imgs], [oracle.sift_trace(im, p) for im in imgs]
    ctx.close()


def test_keypoints_and_descriptors_bit_exact(batch):
    L, up, ctx, ref, _ = batch
    assert sum(len(k) for k, _ in ref) >= 50                      # (not vacuous)
    for i, (name, _) in enumerate(E.images()):
        k, d = ctx.fetch_keypoints(i)
        _same_kps(k, ref[i][0], name)
        assert np.array_equal(d, ref[i][1]), name


def test_candidate_counts_equal_the_trace_and_the_reference(batch):
    L, up, ctx, _, trace = batch
    for i, (name, _) in enumerate(E.images()):
        got = ctx.fetch_candidate_counts(i)
        assert got == (trace[i][1], trace[i][2]), (name, got, trace[i][1:])
        assert got == E.analyse(i, L, up).counts(), (name, got, E.analyse(i, L, up).counts())
    assert sum(t[1] for t in trace) >= 200 and sum(t[2] for t in trace) >= 40


def test_describe_at_its_own_keypoints_returns_the_batch_descriptors(batch):
    L, up, ctx, ref, _ = batch
    n = 0
    for i, (name, img) in enumerate(E.images()):
        k, d = ref[i]
        if len(k):
            assert np.array_equal(ctx.describe(img, k), d), name
            n += len(k)
    assert n >= 50


def test_single_image_entry_bit_exact(vo, oracle):
    name, img = E.images()[0]
    L, up = E.PARAM_SETS[0]
    ctx = vo.Context(E.ROWS, E.COLS, 1, sift=E.sift_params(vo, L, up))
    k, d = ctx.sift(img)
    rk, rd = oracle.sift(img, E.sift_params(oracle, L, up))
    assert len(rk) >= 20
    _same_kps(k, rk, name)
    assert np.array_equal(d, rd)
    ctx.close()


def test_census_has_no_empty_class():
    """A later edit of the images cannot hollow these tests out silently."""
    tot = E.census_total()
    empty = [k for k, v in tot.items() if v < E.CENSUS_MIN]
    assert not empty, empty
    for L, up in E.PARAM_SETS:
        for i in range(len(E.images())):
            assert not E.analyse(i, L, up).undecided_candidates() and not E.analyse(i, L, up).undecided_peaks()
