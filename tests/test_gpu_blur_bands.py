"""The streamed blurs at the band heights large batches give them: every Gaussian plane, keypoint,
descriptor and stereo pair of sampled images of one batched call per case of
tests/test_blur_census.py's table equals the CPU oracle bit for bit, and the profiled launch counts
per site equal what the census of scale-space launches (tests/blur_census.py) lists for the case --
which holds that census to the dispatch in sift_enqueue_pyramid.

A call's frames are two distinct synthetic pairs repeated, so the oracle runs once per distinct
image; the images compared are 0, 1, one in the middle, two fixed pseudo-random ones and the last
two of the call.  Every comparison is exact.

Wall time per case on an MI355X, first run (context, upload, call, oracle, comparisons), seconds, in
the order of the table: 1.65 (the first call of the process), 0.03, 0.22, 0.30, 3.89, 0.34, 0.48,
0.51, 0.44, 0.53, 0.19, 0.43, 0.75, 0.58, 1.84, 0.69, 0.05, 0.08, 0.02, 0.11, 0.99, 1.78, 0.08, 0.06,
0.13, 0.13, 0.33, 0.23, 0.06; the file 17.5 s.  None is near 10 s, so none was replaced."""
import functools
import time

import numpy as np
import pytest

import blur_census as bc
from test_blur_census import CASES

pytestmark = pytest.mark.gpu

PX_PER_CELL = 5.0
MAX_KEYPOINTS = 4096                # the same cap on both sides; the arenas of 1026 images stay small
KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "layer", "scale")


@functools.lru_cache(maxsize=None)
def _pairs(rows, cols):
    from r7020e_visual_odometry_amd import synthetic as syn
    return syn.independent_pairs(2, rows, cols, first=500, px_per_cell=PX_PER_CELL)


@functools.lru_cache(maxsize=None)
def _plan_lib():
    import oracle
    oracle.build()
    return bc.load_plan_lib(oracle)


def _planes(oracle, img, p):
    """oracle.pyramid -> {(octave, level): Gaussian plane}"""
    flat = oracle.pyramid(img, p)
    L = p.n_octave_layers
    r, c = (2 * img.shape[0], 2 * img.shape[1]) if p.upsample else img.shape
    out, off, o = {}, 0, 0
    while off < flat.size:
        if o:
            r, c = r // 2, c // 2
        for i in range(L + 3):
            out[(o, i)] = flat[off: off + r * c].reshape(r, c)
            off += r * c
        off += (L + 2) * r * c
        o += 1
    assert off == flat.size and o == oracle.lib().oracle_num_octaves(img.shape[0], img.shape[1], p.upsample)
    return out


def _sampled_images(n_img):
    """0, 1, the middle, two fixed pseudo-random indices, and the last two"""
    rng = np.random.default_rng(0xB1A5 + n_img)
    return sorted({0, 1, n_img // 2, int(rng.integers(2, n_img)), int(rng.integers(2, n_img)), n_img - 2, n_img - 1})


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}-f{c[2]}-up{c[3]}-off{c[4]}")
def test_planes_features_and_launches_at_batch_band_heights(vo, oracle, case):
    import torch
    t0 = time.perf_counter()
    rows, cols, B, up, offset, why = case
    _, classes, counts = bc.census(_plan_lib(), oracle, rows, cols, B, up, offset=offset)
    assert set(why) <= {":".join(c) for c in classes}
    Ls, Rs = _pairs(rows, cols)
    n = rows * cols
    idx = np.arange(B) % 2
    bufs = []
    for side in (Ls, Rs):
        buf = torch.zeros(B * n + 16, dtype=torch.uint8, device="cuda")
        buf[offset: offset + B * n] = torch.from_numpy(np.ascontiguousarray(side[idx]).reshape(-1)).cuda()
        bufs.append(buf)
    torch.cuda.synchronize()
    ctx = vo.Context(rows, cols, B, sift=vo.SiftParams(3, 1.6, 0.04, 10.0, up, MAX_KEYPOINTS))
    try:
        ctx.set_profiling(True)
        ctx.sift_match_batch_dev(bufs[0].data_ptr() + offset, bufs[1].data_ptr() + offset, B)
        kt = {k: v[1] for k, v in ctx.kernel_times().items()}
        ctx.set_profiling(False)
        assert {s: kt.get(s, 0) for s in bc.SITES} == {s: counts.get(s, 0) for s in bc.SITES}, (kt, counts)

        p = oracle.SiftParams(3, 1.6, 0.04, 10.0, up, MAX_KEYPOINTS)
        ref = {}
        for pair in (0, 1):
            for side, src in enumerate((Ls[pair], Rs[pair])):
                ref[(pair, side)] = (_planes(oracle, src, p),) + oracle.sift(src, p)
        pairs_ref = {pair: oracle.match(ref[(pair, 0)][2], ref[(pair, 1)][2]) for pair in (0, 1)}
        # (not vacuous: from 8000 pixels on every distinct image has keypoints)
        n_kp = [len(v[1]) for v in ref.values()]
        assert rows * cols < 8000 or min(n_kp) >= 1, n_kp
        n_planes = 0
        for img in _sampled_images(2 * B):
            planes, rk, rd = ref[((img // 2) % 2, img % 2)]
            for (o, i), plane in planes.items():
                got = ctx.fetch_gaussian(img, o, i)
                assert got.shape == plane.shape, (img, o, i, got.shape, plane.shape)
                bad = np.argwhere(got.view(np.uint32) != plane.view(np.uint32))
                assert bad.size == 0, f"image {img} octave {o} level {i}: {len(bad)} mismatches, first {bad[:4].tolist()}"
                n_planes += 1
            k, d = ctx.fetch_keypoints(img)
            assert len(k) == len(rk), (img, len(k), len(rk))
            for f in KP_FIELDS:
                assert np.array_equal(k[f], rk[f]), (img, f)
            assert np.array_equal(d, rd), img
            assert np.array_equal(ctx.fetch_stereo_pairs(img // 2), pairs_ref[(img // 2) % 2]), img // 2
        assert n_planes >= min(7, 2 * B) * 6 * 2
    finally:
        ctx.close()
    print(f"case {rows}x{cols} f{B} up{up}: {time.perf_counter() - t0:.1f} s, keypoints {n_kp}, pairs "
          f"{[len(v) for v in pairs_ref.values()]}, launches {counts}")
