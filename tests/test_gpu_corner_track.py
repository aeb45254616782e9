"""GPU: detect_corners -> track_points on a shifted pair, the KLT front end without SIFT: both results are equal
by bytes to corner_ref -> klt_ref, the CPU builds of the same include/vo_spec.h functions."""
import numpy as np
import pytest

import corner_ref as R
import klt_ref as K

pytestmark = pytest.mark.gpu


def test_detect_then_track_equals_the_references_by_bytes(vo):
    img0, img1 = K.images("a:s0")                        # 97 x 121 and its copy shifted by (3.25, -2.5) px
    rows, cols = img0.shape
    exp_c = R.detect(img0, strongest=150)
    exp_t = K.track(img0, img1, exp_c["loc"])
    ctx = vo.Context(rows, cols, 1, sift=vo.default_sift_params(512))
    try:
        loc, met = ctx.detect_corners(img0, vo.default_corner_params(strongest=150))
        assert len(loc) == 150 and loc.tobytes() == exp_c["loc"].tobytes() and met.tobytes() == exp_c["metric"].tobytes()
        pts1, valid, scores, info = ctx.track_points(img0, img1, loc)
        assert pts1.tobytes() == exp_t["pts1"].tobytes() and np.array_equal(valid, exp_t["valid"])
        assert scores.tobytes() == exp_t["scores"].tobytes() and info.tobytes() == exp_t["info"].tobytes()
        err = np.sqrt(((pts1 - loc - np.float32(K.SHIFT)) ** 2).sum(1))[valid]
        assert valid.mean() > 0.9 and np.median(err) < 0.05
    finally:
        ctx.close()
