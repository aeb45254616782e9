"""The octave-0 base of a plane too short for its own band height: 32 x 2048 images in a batch of
72 stereo frames (144 planes of 64 x 4096).  The wave target asks for 72-row bands of the base, the
plane has 64 rows, so the launch plan (csrc/blur_plan.h) does not stream the base from the u8
image: k_base_src<true> stages the upsampled float plane and the tiled blur reads that.  (Before
the plan decided it in one place, the caller passed no source plane at all here.)  Everything
computed equals the CPU oracle bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS, COLS, FRAMES = 32, 2048, 72


def test_short_wide_base_in_a_large_batch_is_staged(vo, oracle, syn):
    import torch
    L, R = syn.stereo_pair(syn.SEED_BASE + 70, ROWS, COLS)
    (kl, dl_ref), (kr, dr_ref) = oracle.sift(L), oracle.sift(R)
    pairs = oracle.match(dl_ref, dr_ref)
    assert len(kl) >= 30 and len(kr) >= 30 and len(pairs) >= 10   # (not vacuous)

    dl = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(L, (FRAMES, ROWS, COLS)))).cuda()
    dr = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(R, (FRAMES, ROWS, COLS)))).cuda()
    torch.cuda.synchronize()
    ctx = vo.Context(ROWS, COLS, FRAMES)
    ctx.set_profiling(True)
    ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), FRAMES)
    kt = {k: v[1] for k, v in ctx.kernel_times().items()}
    ctx.set_profiling(False)
    assert kt.get("k_base_src<true>") == 1 and "k_blur_base" not in kt, kt

    for img, src in ((0, L), (2 * FRAMES - 1, R)):
        flat = oracle.pyramid(src)
        r, c = 2 * ROWS, 2 * COLS
        for level in (0, 1):                                      # octave 0's first planes lead oracle.pyramid
            ref = flat[level * r * c: (level + 1) * r * c].reshape(r, c)
            got = ctx.fetch_gaussian(img, 0, level)
            assert got.shape == ref.shape
            bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
            assert bad.size == 0, f"image {img} level {level}: {len(bad)} mismatches, first {bad[:4].tolist()}"
    for img in (0, 1, 2 * FRAMES - 2, 2 * FRAMES - 1):
        k, d = ctx.fetch_keypoints(img)
        rk, rd = (kl, dl_ref) if img % 2 == 0 else (kr, dr_ref)
        assert len(k) == len(rk) and np.array_equal(k, rk), img
        assert np.array_equal(d, rd), img
    for f in (0, FRAMES - 1):
        assert np.array_equal(ctx.fetch_stereo_pairs(f), pairs), f
    ctx.close()
