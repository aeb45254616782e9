"""GPU: a context's whole life through libvo.so, for the layer that owns its device resources and
scopes its profiler.  No call here fails: the failure paths of the resource pool are driven on the
CPU (test_dev_pool.py).  Every context is 64 x 64, max_batch 2, max_keypoints 256; the frames are a
64 x 64 window of the 150 x 497 synthetic sequence (the calibration's principal point moves with
the window), where the oracle detects about a hundred keypoints per image."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Y0, X0, SCALE = 40, 336, 0.4


@pytest.fixture(scope="module")
def seq(syn):
    L, R, _ = syn.sequence(4, rows=150, cols=497, scale=SCALE)
    crop = lambda F: np.ascontiguousarray(F[:, Y0:Y0 + 64, X0:X0 + 64])
    shift = np.array([[1.0, 0.0, -X0], [0.0, 1.0, -Y0], [0.0, 0.0, 1.0]])
    A, B = syn.calib(SCALE)
    return crop(L), crop(R), shift @ A, shift @ B


def _context(vo, seq):
    return vo.Context(64, 64, 2, calib=vo.calib_from(seq[2], seq[3]), sift=vo.default_sift_params(256))


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays if a is not None)


def _cycle(vo, seq):
    """Create, touch every lazily allocated buffer once, close.  -> the results' bytes, in order.
    A call that does not return VO_OK raises (Context._check)."""
    import torch
    L, R, A, B = seq
    rng = np.random.default_rng(0x11FE)
    out = []
    c = _context(vo, seq)
    try:
        c.set_strongest(72)                                           # selectStrongest's keys, both sets
        c.set_pose_refinement(vo.default_refine_params())             # refinement stats, both sets
        d = vo.distortion_from(A[:, :3], radial=(-0.05, 0.01, 0.002), tangential=(1e-3, -5e-4))
        c.set_distortion(d, d)                                        # the rectified frames
        F1 = rng.integers(0, 256, (200, 128), dtype=np.uint8)
        F2 = np.concatenate([F1[::-1][:150], rng.integers(0, 256, (50, 128), dtype=np.uint8)])
        out.append(_bytes(*c.match(F1, F2, unique=True, return_metric=True)))          # vo_match_ex's buffers
        G1 = rng.random((120, 128), dtype=np.float32)
        G2 = np.concatenate([G1[40:], rng.random((30, 128), dtype=np.float32)])
        out.append(_bytes(c.match_f32(G1, G2)))                                         # the general-float path's
        x1 = rng.uniform(5.0, 60.0, (300, 2)).astype(np.float32)                       # two chunks of 256
        x2 = x1 - np.array([rng.uniform(1.0, 8.0, 300), np.zeros(300)], np.float32).T
        out.append(_bytes(*c.triangulate(x1, x2, A, B, quality=True)))                  # the quality buffers
        out.append(_bytes(*c.sift(np.asfortranarray(L[0]))))                            # column-major staging
        c.set_landmark_frame(True)
        steps = np.concatenate([c.step_batch(L[:2], R[:2]), c.step_batch(L[2:], R[2:])])
        out.append(_bytes(steps))
        X, keep = c.get_landmark_rows()                                                 # the device landmark store
        out.append(_bytes(X, keep))
        out.append(_bytes(*c.fetch_track_quality(1), c.fetch_pose_refinement(1)))
        world = torch.zeros((max(len(X), 1), 3), dtype=torch.float32, device="cuda")
        n = c.landmarks_world_dev(steps["pose"], world.data_ptr(), len(X))             # its pose / offset staging
        out.append(_bytes(world[:n].cpu().numpy()))
        print(f"cycle: {steps['n_left'].tolist()} keypoints, {steps['n_tracked'].tolist()} tracked, {len(X)} landmark rows")
        assert len(X) > 0 and steps["n_tracked"].max() > 0               # the store and the geometry were in use
    finally:
        c.close()
    return out


def test_three_cycles_same_bytes(vo, seq):
    """Create / use / close three times in one process: every call returns VO_OK and cycles 2 and 3
    return the bytes of cycle 1."""
    first = _cycle(vo, seq)
    assert all(len(b) > 0 for b in first)
    for k in (2, 3):
        again = _cycle(vo, seq)
        assert [a == b for a, b in zip(again, first)] == [True] * len(first), f"cycle {k}"


def test_two_contexts_profiler_and_close(vo, seq):
    """A profiles, B does not.  B's launches after A's call are not counted by A's profiler (B's stays
    empty), and B works as before once A is closed: vo_fetch_track_quality launches outside any
    profiled call."""
    L, R, A, B = seq
    rng = np.random.default_rng(0x2C7)
    x1 = rng.uniform(5.0, 60.0, (100, 2)).astype(np.float32)
    x2 = x1 - np.array([rng.uniform(1.0, 8.0, 100), np.zeros(100)], np.float32).T
    a, b = _context(vo, seq), _context(vo, seq)
    try:
        a.set_profiling(True)
        a.triangulate(x1, x2, A, B)                      # A's call: one k_tri_list
        kb, db = b.sift(L[0])                            # B's call: the SIFT kernels
        assert len(kb) > 0
        ta = a.kernel_times()
        assert set(ta) == {"k_tri_list"} and ta["k_tri_list"][1] == 1, ta
        assert b.kernel_times() == {}

        def step_and_quality():
            b.reset()
            return _bytes(b.step_batch(L[:2], R[:2]), *b.fetch_track_quality(1))
        before = step_and_quality()
        a.close()
        assert step_and_quality() == before
        assert b.kernel_times() == {}
    finally:
        a.close()
        b.close()
