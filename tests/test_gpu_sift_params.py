"""GPU parity away from the default vo_sift_params: layer counts 1..5, sigma up to the blur-radius
cap, no upsample, other contrast / edge thresholds.  Every comparison is bit for bit against the CPU
oracle called with the same parameter block.

Other parameters run other kernels than the defaults' (radii 5, 6, 8, 10, 13 streamed): every other
radius takes the generic k_blur_fused<0> and k_small_pyr's runtime-radius loop; a generic level L is
followed by k_down, a streamed one stores the next base itself; without the upsample the base is
k_base_src<false> plus a streamed (float source) or generic blur; k_ext_inner<L>, k_refine's layer
tests, the extremum threshold floor(0.5 ct / L * 255) and k_desc's window tables depend on L and
sigma.  Each case's `route` says which of these it is there for, and after "ran:" what one profiled
batch call (vo_set_profiling / vo_kernel_times) launched.  The profile names the launch sites, not
the instantiations: "k_blur_base" is the streamed base alone (with the upsample fused when no
k_base_src runs before it); "k_blur_fused" counts every level blur, streamed or generic, plus a
generic base; k_down runs exactly where level L of a large octave was generic; every case also runs
k_blur_small (k_small_pyr) and the feature kernels.  The refusals beyond the cap are in
tests/test_abi.py (no GPU needed)."""
import functools

import numpy as np
import pytest

import strongest_ref as sr

pytestmark = pytest.mark.gpu

KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "layer", "scale")
SEED = 900

# (rows, cols, n_octave_layers, sigma, upsample, contrast_threshold, edge_threshold, route)
CASES = [
    (150, 200, 1, 1.2, 1, 0.04, 10.0, "radii 9,17,34 base 3: all generic, k_ext_inner<1>, k_down"
     " | ran: k_base_src<true>, no k_blur_base, k_blur_fused x7, k_down, k_ext_inner<1>"),
    (150, 200, 1, 1.4, 0, 0.04, 10.0, "radii 10,20,39 next to the cap, no upsample, L = 1"
     " | ran: k_base_src<false>, k_blur_base, k_blur_fused x3, k_ext_inner<1>"),
    (150, 200, 2, 1.6, 1, 0.04, 10.0, "radii 7,9,13,18: fused-upsample base, one streamed level, level L generic -> k_down"
     " | ran: k_blur_base alone, k_blur_fused x8, k_down, k_ext_inner<2>"),
    (150, 200, 2, 1.6, 0, 0.04, 10.0, "base radius 6: k_base_src<false> + streamed float-source base"
     " | ran: k_base_src<false>, k_blur_base, k_blur_fused x4, k_ext_inner<2>"),
    (150, 200, 3, 1.6, 0, 0.04, 10.0, "the defaults' radii, no upsample: k_expand offsets, octave numbers"
     " | ran: k_base_src<false>, k_blur_base, k_blur_fused x5, k_ext_inner<3>"),
    (150, 200, 4, 1.6, 1, 0.04, 10.0, "radii 4,5,6,7,8,10: streamed and generic interleaved, level L = 7 generic"
     " | ran: k_blur_base alone, k_blur_fused x12, k_down, k_ext_inner<4>"),
    (150, 200, 5, 1.6, 1, 0.04, 10.0, "radii 4,4,5,6,7,7,9: 8 levels, k_ext_inner<5>"
     " | ran: k_blur_base alone, k_blur_fused x14, k_down, k_ext_inner<5>"),
    (150, 200, 5, 1.6, 0, 0.04, 10.0, "8 levels, no upsample"
     " | ran: k_base_src<false>, k_blur_base, k_blur_fused x7, k_ext_inner<5>"),
    (150, 200, 3, 1.2, 1, 0.04, 10.0, "radii 4,5,6,8,10 base 3: streamed level L stores the next base after a generic level"
     " | ran: k_base_src<true>, no k_blur_base, k_blur_fused x11, no k_down"),
    (150, 200, 3, 2.0, 1, 0.04, 10.0, "radii 6,8,10,13,16 base 7: level L streamed, top level and base generic"
     " | ran: k_base_src<true>, no k_blur_base, k_blur_fused x11, no k_down"),
    (150, 200, 3, 2.0, 0, 0.04, 10.0, "radii 6,8,10,13,16 base 8: streamed float-source base"
     " | ran: k_base_src<false>, k_blur_base, k_blur_fused x5"),
    (150, 200, 3, 5.0, 1, 0.04, 10.0, "radii 16..39 base 20: generic kernel above 64 KB of LDS, large descriptor tables"
     " | ran: k_base_src<true>, no k_blur_base, k_blur_fused x11, k_down"),
    (150, 200, 2, 3.4, 0, 0.04, 10.0, "radii 14,19,27,39: next to the cap at L = 2, few large keypoints"
     " | ran: k_base_src<false>, no k_blur_base, k_blur_fused x5"),
    (97, 131, 5, 1.6, 1, 0.04, 10.0, "odd sizes, ragged strips"),
    (97, 131, 2, 1.6, 0, 0.04, 10.0, "odd sizes, ragged strips, no upsample"),
    (24, 420, 3, 5.0, 0, 0.04, 10.0, "radius 39 > 24 rows: iterated reflect-101 in the generic tiled kernel; octave 0 outside k_small_pyr"
     " | ran: k_base_src<false>, no k_blur_base, k_blur_fused x6"),
    (40, 1450, 2, 1.6, 1, 0.04, 10.0, "octave 0 wider than 1400 columns: 4 columns per lane for the streamed radius 13"
     " | ran: k_blur_base alone, k_blur_fused x12, k_down x2"),
    (70, 1500, 4, 1.6, 0, 0.04, 10.0, "wider than 1400 columns, no upsample"
     " | ran: k_base_src<false>, k_blur_base, k_blur_fused x12, k_down"),
    (150, 200, 3, 1.6, 1, 0.0, 10.0, "extremum threshold 0 (contrast 0)"),
    (150, 200, 3, 1.6, 1, 0.01, 10.0, "extremum threshold floor(0.425) = 0, contrast test 0.01"),
    (150, 200, 1, 1.2, 1, 0.09, 10.0, "extremum threshold floor(11.475) = 11 at L = 1"),
    (150, 200, 3, 1.6, 1, 0.04, 2.0, "edge threshold 2"),
    (150, 200, 3, 1.6, 1, 0.04, 50.0, "edge threshold 50"),
]


def _id(c):
    rows, cols, L, sigma, up, ct, et, _ = c
    return f"{rows}x{cols}-L{L}-s{sigma}-up{up}-ct{ct}-et{et}"


def _params(mod, L, sigma, up, ct=0.04, et=10.0, cap=16384):
    return mod.SiftParams(L, sigma, ct, et, up, cap)


@functools.lru_cache(maxsize=None)
def _frames(rows, cols):
    """The stereo pair and its mirror image: lefts [2, rows, cols], rights [2, rows, cols]."""
    from r7020e_visual_odometry_amd import synthetic as syn
    L, R = syn.stereo_pair(syn.SEED_BASE + SEED, rows, cols)
    return (np.ascontiguousarray(np.stack([L, L[:, ::-1]])), np.ascontiguousarray(np.stack([R, R[:, ::-1]])))


@functools.lru_cache(maxsize=None)
def _ref_features(rows, cols, L, sigma, up, ct, et):
    """oracle.sift of the four images (image 2 f + side), computed once per parameter block."""
    import oracle
    Ls, Rs = _frames(rows, cols)
    p = _params(oracle, L, sigma, up, ct, et)
    return [oracle.sift((Ls, Rs)[i % 2][i // 2], p) for i in range(4)]


def _planes(oracle, img, p):
    """oracle.pyramid -> {(octave, level): Gaussian plane}, for any layer count / upsample."""
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


def _multi_peak(k):
    """keypoints that share location, scale and layer with another (several orientation peaks)"""
    key = np.stack([k["x"], k["y"], k["scale"]], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return int((cnt[inv.reshape(-1)] > 1).sum())


def _batch(vo, ctx, rows, cols, concurrency=None):
    import torch
    Ls, Rs = _frames(rows, cols)
    dl, dr = torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda()
    torch.cuda.synchronize()
    if concurrency:
        ctx.set_concurrency(concurrency)
    return ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), 2)


# ------------------------------------------------------------------ (a) the scale space
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gaussian_levels_bit_exact(vo, oracle, case):
    rows, cols, L, sigma, up, ct, et, _ = case
    Ls, Rs = _frames(rows, cols)
    ctx = vo.Context(rows, cols, 2, sift=_params(vo, L, sigma, up, ct, et))
    _batch(vo, ctx, rows, cols)
    rp = _params(oracle, L, sigma, up, ct, et)
    for img in (0, 3):
        ref = _planes(oracle, (Ls, Rs)[img % 2][img // 2], rp)
        assert len(ref) % (L + 3) == 0
        for (o, i), plane in ref.items():
            got = ctx.fetch_gaussian(img, o, i)
            assert got.shape == plane.shape, (o, i, got.shape, plane.shape)
            bad = np.argwhere(got.view(np.uint32) != plane.view(np.uint32))
            assert bad.size == 0, f"image {img} octave {o} level {i}: {len(bad)} mismatches, first {bad[:4].tolist()}"
    ctx.close()


# ------------------------------------------------------------------ (b) keypoints, descriptors, matches
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_features_and_matches_bit_exact(vo, oracle, case):
    rows, cols, L, sigma, up, ct, et, _ = case
    Ls, Rs = _frames(rows, cols)
    ref = _ref_features(rows, cols, L, sigma, up, ct, et)
    rk, rd = ref[0]
    rpairs = [oracle.match(ref[2 * f][1], ref[2 * f + 1][1]) for f in range(2)]
    print(f"{_id(case)}: left keypoints {len(rk)}, multi-peak {_multi_peak(rk)}, stereo matches {len(rpairs[0])}")
    # the oracle's own output is not vacuous
    if rows != 24:
        assert len(rk) >= 30, len(rk)
    if (rows, cols) == (150, 200):
        assert _multi_peak(rk) >= 8, _multi_peak(rk)
        assert len(rpairs[0]) >= (5 if (L, sigma, up) == (2, 3.4, 0) else 10), len(rpairs[0])
    ctx = vo.Context(rows, cols, 2, sift=_params(vo, L, sigma, up, ct, et))
    k, d = ctx.sift(Ls[0])
    _same_kps(k, rk, "vo_sift")
    assert np.array_equal(d, rd)
    _batch(vo, ctx, rows, cols, concurrency=2)
    for img in range(4):
        kk, dd = ctx.fetch_keypoints(img)
        _same_kps(kk, ref[img][0], f"image {img}")
        assert np.array_equal(dd, ref[img][1]), img
    for f in range(2):
        assert np.array_equal(ctx.fetch_stereo_pairs(f), rpairs[f]), f
    ctx.close()


# ------------------------------------------------------------------ (c) the loop body
@pytest.mark.parametrize("L,sigma,up", [(2, 1.6, 0), (4, 1.6, 1)])
def test_loop_body_bit_exact(vo, oracle, syn, L, sigma, up):
    """VO.m's loop over 4 frames: step_batch and the pipelined step_submit_dev / step_collect
    (two batches of 2) against oracle.run_sequence with the same parameter block."""
    import torch
    s = 0.4
    rows, cols = 150, 497
    A, B = syn.calib(s)
    SL, SR, _ = syn.sequence(4, rows=rows, cols=cols, scale=s)
    routs, rlm = oracle.run_sequence(SL, SR, A, B, sp=_params(oracle, L, sigma, up))
    assert routs["status"].tolist() == [0, 0, 0, 0] and routs["n_tracked"][1:].min() >= 8, routs
    ctx = vo.Context(rows, cols, 2, calib=vo.calib_from(A, B), sift=_params(vo, L, sigma, up))

    def compare(outs, lm):
        for f in range(4):
            for k in ("status", "n_left", "n_right", "n_stereo", "n_tracked", "n_inliers", "n_landmarks"):
                assert outs[f][k] == routs[f][k], (f, k, outs[f][k], routs[f][k])
            assert np.array_equal(outs[f]["rel_pose"], routs[f]["rel_pose"]), f
            assert np.array_equal(outs[f]["pose"], routs[f]["pose"]), f
        assert np.array_equal(lm, rlm)

    compare(np.concatenate([ctx.step_batch(SL[0:2], SR[0:2]), ctx.step_batch(SL[2:4], SR[2:4])]), ctx.get_landmarks())
    ctx.reset()
    dl, dr = torch.from_numpy(np.ascontiguousarray(SL)).cuda(), torch.from_numpy(np.ascontiguousarray(SR)).cuda()
    torch.cuda.synchronize()
    fs = SL[0].size
    for a in (0, 2):
        ctx.step_submit_dev(dl.data_ptr() + a * fs, dr.data_ptr() + a * fs, 2)
    outs = []
    while ctx.steps_pending():
        outs.append(ctx.step_collect())
    compare(np.concatenate(outs), ctx.get_landmarks())
    ctx.close()


# ------------------------------------------------------------------ (d) selectStrongest
def test_select_strongest_at_five_layers(vo, oracle):
    """selectStrongest(points, 40) at (5, 1.6, no upsample) == tests/strongest_ref.py on the
    oracle's detections (the rank kernels see another layer count and octave numbering)."""
    rows, cols, N = 150, 200, 40
    Ls, _ = _frames(rows, cols)
    rk, rd = _ref_features(rows, cols, 5, 1.6, 0, 0.04, 10.0)[0]
    assert len(rk) > N
    sk, sd = sr.select(rk, rd, N)
    ctx = vo.Context(rows, cols, 1, sift=_params(vo, 5, 1.6, 0))
    ctx.set_strongest(N)
    k, d = ctx.sift(Ls[0])
    _same_kps(k, sk, "selectStrongest")
    assert np.array_equal(d, sd)
    ctx.close()


# ------------------------------------------------------------------ (e) the accepted side of the bounds
@pytest.mark.parametrize("L,sigma", [(1, 1.4), (2, 3.4), (3, 5.0), (3, 5.2)])
def test_sigma_next_to_the_radius_cap_is_accepted_and_exact(vo, oracle, L, sigma):
    """Top-level radius 39, and at (3, 5.2) 40 = VO_SIFT_MAX_RADIUS itself (the refused side, 45 /
    46 / 47 and 41, is tests/test_abi.py): the context is created, detects, and equals the oracle."""
    rows, cols = 150, 200
    Ls, _ = _frames(rows, cols)
    rk, rd = oracle.sift(Ls[0], _params(oracle, L, sigma, 1))
    assert len(rk) >= 30, len(rk)
    ctx = vo.Context(rows, cols, 1, sift=_params(vo, L, sigma, 1))
    k, d = ctx.sift(Ls[0])
    _same_kps(k, rk)
    assert np.array_equal(d, rd)
    ctx.close()
