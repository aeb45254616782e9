"""The scale space as two chains: octaves 0 and 1 on the scale-space stream, the
large octaves 2.. and k_small_pyr on the down stream, forked after octave 1's level L (after octave
0's when octave 1 is not a large one; one or more octaves later only where a batch is large enough
for octave 2's blurs to run at full bands, which the 256- and 512-pair cases of
test_gpu_sift_match.py reach and the shapes here do not), beside octave 1's levels L+1, L+2.  No
kernel's arithmetic
changed, so every comparison is bit for bit: with the CPU oracle, or with the same inputs run one
call at a time behind a host synchronise.

Which launches a shape gets (2 stereo pairs, so the band height is 4 rows): a level blur streams
when its plane has more rows than radius + 6 -- more than 19 rows at the defaults' largest radius
13 -- and an octave belongs to k_small_pyr when its plane has at most 9216 pixels.  A streamed
octave 1 therefore needs a frame of more than 9216 pixels and more than 19 rows; the smallest is
22 x 419 (9218 = 2 * 11 * 419 has no other factorisation with both sides above 19): octave 0
44 x 838 and octave 1 22 x 419 stream, octaves 2, 3 (11 x 209, 5 x 104) are k_small_pyr's, which is
then all of the down chain.  Twice that, 44 x 838, is the smallest frame with a streamed octave on
the down chain.  The call-order tests use 100 x 380 (octave 2: 50 x 190 = 9500 pixels, streamed on
the down chain; keypoints from k_small_pyr's octaves too)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "layer", "scale")
SMALLEST = (22, 419)
CALLS = (100, 380)
PX_PER_CELL = 5.0                  # texture fine enough for ~200 keypoints per image at these sizes


@functools.lru_cache(maxsize=None)
def _pairs(rows, cols, n, first):
    from r7020e_visual_odometry_amd import synthetic as syn
    return syn.independent_pairs(n, rows, cols, first=first, px_per_cell=PX_PER_CELL)


def _dev(L, R):
    import torch
    dl, dr = torch.from_numpy(np.ascontiguousarray(L)).cuda(), torch.from_numpy(np.ascontiguousarray(R)).cuda()
    torch.cuda.synchronize()
    return dl, dr


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


def _same_kps(a, b, what=""):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in KP_FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f)


def _results(ctx, B, levels=None):
    """everything a caller can fetch of the last batched call"""
    out = {"kp": [ctx.fetch_keypoints(i) for i in range(2 * B)], "pairs": [ctx.fetch_stereo_pairs(f) for f in range(B)]}
    if levels:
        n_oct, n_lev = levels
        out["g"] = {(i, o, l): ctx.fetch_gaussian(i, o, l) for i in range(2 * B) for o in range(n_oct) for l in range(n_lev)}
    return out


def _same_results(a, b, what=""):
    for i, ((ka, da), (kb, db)) in enumerate(zip(a["kp"], b["kp"])):
        _same_kps(ka, kb, f"{what} image {i}")
        assert np.array_equal(da, db), (what, i)
    for f, (pa, pb) in enumerate(zip(a["pairs"], b["pairs"])):
        assert np.array_equal(pa, pb), (what, f)
    for k, g in a.get("g", {}).items():
        assert np.array_equal(g.view(np.uint32), b["g"][k].view(np.uint32)), (what, k)


def _against_oracle(ctx, oracle, Ls, Rs, p, what=""):
    """Gaussian levels, keypoints, descriptors and stereo pairs of the last batched call of the frames
    Ls, Rs against the oracle with parameter block p."""
    B = len(Ls)
    desc = []
    for img in range(2 * B):
        src = (Ls, Rs)[img % 2][img // 2]
        for (o, i), plane in _planes(oracle, src, p).items():
            got = ctx.fetch_gaussian(img, o, i)
            assert got.shape == plane.shape, (what, img, o, i)
            bad = np.argwhere(got.view(np.uint32) != plane.view(np.uint32))
            assert bad.size == 0, f"{what} image {img} octave {o} level {i}: {len(bad)} mismatches, first {bad[:4].tolist()}"
        rk, rd = oracle.sift(src, p)
        k, d = ctx.fetch_keypoints(img)
        _same_kps(k, rk, f"{what} image {img}")
        assert np.array_equal(d, rd), (what, img)
        desc.append(rd)
    n_pairs = 0
    for f in range(B):
        ref = oracle.match(desc[2 * f], desc[2 * f + 1])
        assert np.array_equal(ctx.fetch_stereo_pairs(f), ref), (what, f)
        n_pairs += len(ref)
    return sum(len(d) for d in desc), n_pairs


def _profiled_async_call(ctx, dl, dr, B):
    """launch counts {name: calls} of one asynchronous (forked) call"""
    ctx.set_profiling(True)
    ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), B, stats=False)
    kt = {k: v[1] for k, v in ctx.kernel_times().items()}
    ctx.set_profiling(False)
    return kt


# ------------------------------------------------------------------ smallest shapes with all three parts
@pytest.mark.parametrize("rows,cols,n_large", [(22, 419, 2), (44, 838, 3)])
def test_smallest_shapes_with_streamed_octaves_and_small(vo, oracle, rows, cols, n_large):
    Ls, Rs = _pairs(rows, cols, 2, 40)
    dl, dr = _dev(Ls, Rs)
    ctx = vo.Context(rows, cols, 2)
    kt = _profiled_async_call(ctx, dl, dr, 2)
    # 5 level blurs per large octave (a generic base would count as one more k_blur_fused: at 22 x 419
    # octave 0's 44 rows are below the fused-upsample base's 64, so k_base_src and the streamed
    # float-source base); no k_down: every level L streamed and stored the next base; the other
    # octaves in k_small_pyr
    assert kt.get("k_blur_fused") == 5 * n_large and kt.get("k_blur_base") == 1 and kt.get("k_blur_small") == 1 and \
        "k_down" not in kt, kt
    n_kp, n_pairs = _against_oracle(ctx, oracle, Ls, Rs, oracle.SiftParams(3, 1.6, 0.04, 10.0, 1, 16384), "async")
    assert n_kp >= 400 and n_pairs >= 20, (n_kp, n_pairs)
    ctx.close()
    if n_large == 2:
        # one row fewer: octave 1 (21 x 419 = 8799 pixels) moves into k_small_pyr
        ctx = vo.Context(rows - 1, cols, 2)
        d1 = _dev(*_pairs(rows - 1, cols, 2, 40))
        kt = _profiled_async_call(ctx, d1[0], d1[1], 2)
        assert kt.get("k_blur_fused") == 5 and kt.get("k_blur_small") == 1, kt
        ctx.close()


# ------------------------------------------------------------------ back-to-back calls
def test_back_to_back_calls_equal_one_at_a_time(vo, oracle):
    """Calls 1..k back to back without a host synchronise, for k = 1..4 (only the last call's results
    can be fetched: call n+2 overwrites call n's set): call k's Gaussian levels, keypoints,
    descriptors and pairs equal the same inputs run alone behind a synchronise -- and those the oracle."""
    rows, cols = CALLS
    B = 2
    inputs = [_pairs(rows, cols, B, 50 + 10 * j) for j in range(4)]
    dev = [_dev(L, R) for L, R in inputs]
    ctx = vo.Context(rows, cols, B)
    n_oct = oracle.lib().oracle_num_octaves(rows, cols, 1)
    alone = []
    for j, (dl, dr) in enumerate(dev):
        ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), B)            # stats: synchronises
        alone.append(_results(ctx, B, (n_oct, 6)))
    p = oracle.SiftParams(3, 1.6, 0.04, 10.0, 1, 16384)
    n_kp, n_pairs = _against_oracle(ctx, oracle, inputs[3][0], inputs[3][1], p, "alone")
    assert n_kp >= 400 and n_pairs >= 10, (n_kp, n_pairs)
    assert not np.array_equal(alone[0]["g"][(0, 3, 2)], alone[1]["g"][(0, 3, 2)])       # the inputs do differ
    for k in range(1, 5):
        for dl, dr in dev[:k]:
            ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), B, stats=False)
        _same_results(_results(ctx, B, (n_oct, 6)), alone[k - 1], f"after {k} calls")
    # and with the order reversed, so every input is once the one behind three others
    for dl, dr in reversed(dev):
        ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), B, stats=False)
    _same_results(_results(ctx, B, (n_oct, 6)), alone[0], "reversed")
    ctx.close()


# ------------------------------------------------------------------ concurrency split
def test_concurrency_split_equals_one_part(vo, oracle):
    rows, cols = CALLS
    B = 6
    Ls, Rs = _pairs(rows, cols, B, 100)
    dl, dr = _dev(Ls, Rs)
    ctx = vo.Context(rows, cols, B)
    n_oct = oracle.lib().oracle_num_octaves(rows, cols, 1)
    res = {}
    for n in (1, 2, 3):
        ctx.set_concurrency(n)
        for _ in range(2):                                      # both buffer sets, no synchronise between
            ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), B, stats=False)
        res[n] = _results(ctx, B, (n_oct, 6))
    _same_results(res[2], res[1], "2 parts")
    _same_results(res[3], res[1], "3 parts")
    assert sum(len(k) for k, _ in res[1]["kp"]) >= 1200
    ctx.close()


# ------------------------------------------------------------------ submit / collect
def test_three_batches_in_flight_on_the_golden_sequence(vo):
    """112 x 373: octaves 0, 1, 2 streamed (56 x 186 = 10416 pixels), the rest in k_small_pyr.  The
    loop body keeps the scale space one chain (its geometry and copy streams leave no queue for a
    fifth stream), behind the same ev_top / ev_join waits as the forked calls."""
    from pathlib import Path
    z = np.load(Path(__file__).resolve().parent / "golden" / "sequence.npz")
    L, R = z["L"], z["R"]
    assert len(L) == 3
    ctx = vo.Context(L.shape[1], L.shape[2], 1, calib=vo.calib_from(z["P1"], z["P2"]))
    sync = np.concatenate([ctx.step_batch(L[i:i + 1], R[i:i + 1]) for i in range(3)])
    sync_lm = ctx.get_landmarks()
    ctx.reset()
    dl, dr = _dev(L, R)
    fs = L[0].size
    for i in range(3):
        ctx.step_submit_dev(dl.data_ptr() + i * fs, dr.data_ptr() + i * fs, 1)
    assert ctx.steps_pending() == 3
    outs = []
    while ctx.steps_pending():
        outs.append(ctx.step_collect())
    outs = np.concatenate(outs)
    for k in outs.dtype.names:
        assert np.array_equal(outs[k], sync[k]), k
        if k != "flags":
            assert np.array_equal(outs[k], z["out_" + k]), k
    assert np.array_equal(ctx.get_landmarks(), sync_lm) and np.array_equal(sync_lm, z["landmarks"])
    ctx.close()


# ------------------------------------------------------------------ non-default parameters
# Octaves 0, 1, 2 large, level L generic: octave 1's base by k_down on the scale-space stream,
# octave 2's by k_down at the head of the down chain.  (rows, cols, L, sigma, upsample, route)
PARAM_CASES = [
    (150, 260, 1, 1.2, 1, "radii 9, 17, 34: every blur generic"),
    (150, 260, 5, 1.6, 1, "8 levels; level L (radius 7) generic"),
    (300, 520, 4, 1.6, 0, "no upsample; octave 2 75 x 130 above k_small_pyr's 9216 pixels, level L (radius 7) generic"),
]


@pytest.mark.parametrize("case", PARAM_CASES, ids=lambda c: f"{c[0]}x{c[1]}-L{c[2]}-s{c[3]}-up{c[4]}")
def test_non_default_parameters_with_k_down_on_the_down_chain(vo, oracle, case):
    rows, cols, L, sigma, up, _ = case
    Ls, Rs = _pairs(rows, cols, 2, 200)
    dl, dr = _dev(Ls, Rs)
    ctx = vo.Context(rows, cols, 2, sift=vo.SiftParams(L, sigma, 0.04, 10.0, up, 16384))
    kt = _profiled_async_call(ctx, dl, dr, 2)
    assert kt.get("k_down") == 2 and kt.get("k_blur_small") == 1, kt
    ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), 2, stats=False)      # the other set, behind the first
    n_kp, _ = _against_oracle(ctx, oracle, Ls, Rs, oracle.SiftParams(L, sigma, 0.04, 10.0, up, 16384), case[5])
    assert n_kp >= 100, n_kp
    ctx.close()


# ------------------------------------------------------------------ tiny images: an empty side of the fork
@pytest.mark.parametrize("rows,cols,up", [(16, 16, 1), (16, 20, 0)])
def test_tiny_image_and_context_churn(vo, oracle, rows, cols, up):
    """Every octave below 0 is k_small_pyr's: the fork follows octave 0's level L and the down chain
    holds that one launch (vo_create refuses sides under 16, so there always is an octave 1).  20 contexts created, used and
    destroyed, then one more: streams and events are the context's own and go with it."""
    Ls, Rs = _pairs(rows, cols, 2, 300)
    dl, dr = _dev(Ls, Rs)
    sp = vo.SiftParams(3, 1.6, 0.04, 10.0, up, 16384)
    rp = oracle.SiftParams(3, 1.6, 0.04, 10.0, up, 16384)
    for i in range(21):
        ctx = vo.Context(rows, cols, 2, sift=sp)
        if i in (0, 20):
            kt = _profiled_async_call(ctx, dl, dr, 2)
            assert kt.get("k_blur_small") == 1 and "k_down" not in kt, kt
            ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), 2, stats=False)
            _against_oracle(ctx, oracle, Ls, Rs, rp, f"context {i}")
        else:
            ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), 2, stats=False)
        ctx.close()
