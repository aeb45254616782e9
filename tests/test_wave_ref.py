"""Holds the NumPy restatements of tests/wave_probe.py (what tests/test_gpu_wave.py compares the device's
collectives with) to independent references, so that the GPU suite does not compare the device with an
unchecked restatement: the float64 tree against vo_spec.h's vo_tree_sum by bytes, the integer tree, scans and
rank against np.sum / plain Python loops, the two top-2 merges against a brute-force loop over all pairs, and
-- for each floating-point family the GPU suite sums -- that the tree's result differs in bits from the
left-to-right sum and from the tree with its levels reversed, so the order is pinned and not merely met."""
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

import wave_probe as wp

ROOT = Path(__file__).resolve().parent.parent
M32 = 1 << 32


def test_probe_is_built_with_the_kernels_flags():
    """tests/wave_probe/Makefile's HIPFLAGS are csrc/Makefile's but for the include directories"""
    def flags(path):
        text = path.read_text().replace("\\\n", " ")
        return [f for f in re.search(r"^HIPFLAGS\s*=(.*)$", text, re.M).group(1).split() if not f.startswith("-I")]
    ours = flags(ROOT / "tests" / "wave_probe" / "Makefile")
    theirs = flags(ROOT / "r7020e-visual-odometry_amd" / "csrc" / "Makefile")
    assert ours == theirs
    assert {"-ffp-contract=off", "-fno-fast-math", "-O3", "--offload-arch=$(ARCH)"} <= set(ours)


def test_float64_tree_equals_vo_tree_sum_by_bytes(oracle):
    x = wp.per_wave(wp.wave_family(np.float64)).reshape(-1, 64)                    # [8 waves][64]
    assert oracle.tree_sum(np.ascontiguousarray(x.T), x.shape[0]).tobytes() == wp.tree_sum(x).tobytes()
    y = wp.xor28_family().reshape(8, 64, 28)
    for w in range(8):
        got = oracle.tree_sum(np.ascontiguousarray(y[w]), 28)
        assert got.tobytes() == wp.tree_sum(y[w].T).tobytes()
    assert wp.wave_sum_n(wp.xor28_family()).reshape(8, 64, 28)[3, 17].tobytes() == oracle.tree_sum(np.ascontiguousarray(y[3]), 28).tobytes()


@pytest.mark.parametrize("dtype", [np.int32, np.uint32, np.int64])
def test_integer_tree_is_the_sum(dtype):
    rng = np.random.default_rng(11)
    info = np.iinfo(dtype)
    x = rng.integers(info.min, info.max, (40, 64), dtype=dtype, endpoint=True)       # sums wrap
    mod = 1 << (8 * np.dtype(dtype).itemsize)
    got = wp.tree_sum(x)
    assert got.dtype == np.dtype(dtype)
    for w in range(40):
        assert (int(got[w]) - sum(int(v) for v in x[w])) % mod == 0
    assert np.array_equal(got, np.sum(x, axis=-1, dtype=dtype))
    assert np.array_equal(wp.wave_sum(x.reshape(10, 1, 256)).reshape(40, 64), np.repeat(got[:, None], 64, 1))


@pytest.mark.parametrize("dtype", [np.int32, np.uint32])
def test_scans_and_rank_equal_python_loops(dtype):
    rng = np.random.default_rng(12)
    info = np.iinfo(dtype)
    x = rng.integers(info.min, info.max, (3, 2, 192), dtype=dtype, endpoint=True)
    inc = wp.wave_incl_scan(x)
    ex, tot = wp.block_excl_scan(x.view(np.uint32))
    assert inc.dtype == np.dtype(dtype) and ex.dtype == np.uint32
    for b, r in itertools.product(range(3), range(2)):
        run = 0
        for t in range(192):
            if t % 64 == 0:
                wave = 0
            assert int(ex[b, r, t]) == run % M32
            wave += int(x[b, r, t])
            run += int(x.view(np.uint32)[b, r, t])
            assert (int(inc[b, r, t]) - wave) % M32 == 0
        assert (tot[b, r] == run % M32).all()
    pred = (x & 1).astype(np.int32)
    rank, count = wp.wave_rank(pred)
    for b, r, t in itertools.product(range(3), range(2), range(192)):
        w0 = t - t % 64
        assert rank[b, r, t] == sum(int(p) for p in pred[b, r, w0:t])
        assert count[b, r, t] == sum(int(p) for p in pred[b, r, w0:w0 + 64])


def test_rank_patterns_hold_what_they_are_named_for():
    m = wp.rank_masks()
    assert m.shape == (76, 64) and m[0].sum() == 0 and m[1].sum() == 64
    assert (m[2] + m[3] == 1).all() and m[2, 0] == 1
    for r in range(4):
        assert m[4 + r].sum() == 16 and m[4 + r, 16 * r:16 * r + 16].all()
    assert np.array_equal(m[12:], np.eye(64, dtype=np.int32))


def test_integer_block_sum_and_match_place_equal_python_loops():
    rng = np.random.default_rng(13)
    x = rng.integers(0, M32, (2, 2, 192), dtype=np.uint32)
    got = wp.block_sum(x)
    for b, r in itertools.product(range(2), range(2)):
        assert (got[b, r] == sum(int(v) for v in x[b, r]) % M32).all()
    ok = (rng.random((3, 3, 256)) < 0.4).astype(np.int32)
    ok[1, 1] = 0
    ok[2, 0] = 1
    pos, base = wp.match_place(ok)
    for b in range(3):
        placed = 0
        for r in range(3):
            for t in range(256):
                assert pos[b, r, t] == placed
                placed += int(ok[b, r, t])
            assert (base[b, r] == placed).all()


def _beats_c(f, e):
    return f[0] > e[0] or (f[0] == e[0] and f[1] < e[1])


def _beats_s(f, e):
    return f[0] < e[0] or (f[0] == e[0] and f[1] < e[1])


def _brute(cands, beats, held, pick, other, empty):
    """the best triple is the one no other triple beats (all pairs); the second value is the extreme over all
    pairs of distinct multiset members of the pair's worse one"""
    h = [c for c in cands if held(c)]
    best = [e for e in h if not any(beats(f, e) for f in h if f is not e)]
    vals = [v for c in cands for v in (c[0], c[2])]
    second = pick(other(vals[a], vals[b]) for a in range(len(vals)) for b in range(len(vals)) if a != b)
    assert len(best) <= 1
    return (best[0][0], best[0][1], second) if best else (empty, -1, second)


def test_top2_merges_equal_brute_force_over_all_pairs():
    rng = np.random.default_rng(14)
    vals = [0.25, 0.5, 0.75, 1.0]
    ties_c = ties_s = second_is_best = empties = 0
    for _ in range(600):
        n = int(rng.integers(2, 7))
        idx = rng.permutation(50)[:n]
        cc, cs = [], []
        for k in range(n):
            b = vals[int(rng.integers(4))]
            lower = [v for v in vals if v <= b] + [-np.inf]
            upper = [v for v in vals if v >= b] + [np.inf]
            cc.append((b, int(idx[k]), lower[int(rng.integers(len(lower)))]))
            cs.append((np.inf, -1, np.inf) if rng.random() < 0.3 else (b, int(idx[k]), upper[int(rng.integers(len(upper)))]))
        if rng.random() < 0.1:
            cs = [(np.inf, -1, np.inf)] * n
        got_c, got_s = wp.top2c_union(cc), wp.top2s_union(cs)
        assert got_c == _brute(cc, _beats_c, lambda c: True, max, min, -np.inf)
        assert got_s == _brute(cs, _beats_s, lambda c: c[1] >= 0, min, max, np.inf)
        ties_c += sum(c[0] == got_c[0] for c in cc) > 1
        ties_s += sum(c[0] == got_s[0] and c[1] >= 0 for c in cs) > 1
        second_is_best += got_c[2] == got_c[0]
        empties += got_s[1] < 0
    assert min(ties_c, ties_s, second_is_best, empties) > 20       # the forced ties and the empty sets did occur


def test_fill_of_partnerless_lanes_never_reaches_lane_0():
    """wave_tree's ZERO flag chooses what a lane without a partner at a level is given (0, or its own value).
    Lane-level model of the no-LDS tree with that fill replaced by arbitrary values: lane l has a partner
    l + off at the permlane levels if l % (2 off) < off, at a row_shl level if l % 16 + off < 16.  Lane 0's
    chain only ever reads lanes that had one, so the broadcast result is the tree's p[0] whatever the fill
    is: no input tells wave_sum built with ZERO = false, or wave_max with ZERO = true, from the header's."""
    rng = np.random.default_rng(15)
    x = wp.mixed(np.float32, (16, 64), 7)
    lane = np.arange(64)
    for trial in range(8):
        v = x.copy()
        for off in wp.OFFS:
            has = (lane % (2 * off) < off) if off >= 16 else (lane % 16 + off < 16)
            other = np.where(has, v[:, (lane + off) % 64], rng.standard_normal((16, 64)).astype(np.float32) * 1e6)
            v = v + other
        assert v[:, 0].tobytes() == wp.tree_sum(x).tobytes()
        assert (v[:, 1:] != v[:, :1]).any()                                   # the other lanes do depend on it


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wave_family_pins_the_tree_order(dtype):
    x = wp.per_wave(wp.wave_family(dtype))
    assert x.dtype == np.dtype(dtype) and (x > 0).any() and (x < 0).any()
    t = wp.tree_sum(x)
    assert (t != wp.seq_sum(x)).all() and (t != wp.rev_tree_sum(x)).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nwaves", wp.BLOCK_NWAVES)
def test_block_family_pins_the_tree_order(dtype, nwaves):
    x = wp.block_family(dtype, nwaves)
    t = wp.block_sum(x)
    assert (t == t[..., :1]).all()
    assert (t[..., 0] != wp.block_seq_sum(x)).all() and (t[..., 0] != wp.block_rev_sum(x)).all()


def test_xor28_family_pins_the_tree_order():
    x = wp.xor28_family()
    w = np.moveaxis(x.reshape(8, 64, 28), -1, -2)                                  # [8 waves][28][64]
    t = wp.tree_sum(w)
    assert ((t != wp.seq_sum(w)).sum(-1) >= 14).all() and ((t != wp.rev_tree_sum(w)).sum(-1) >= 14).all()
