"""The contracts of csrc/wave.h and csrc/match_merge.h, function by function, on the MI355X: the device probe
(tests/wave_probe) calls one collective per thread and stores every thread's return value; each is compared
bit for bit with tests/wave_probe.py's NumPy restatement (held to independent references by
tests/test_wave_ref.py), in every lane and thread, in at least two blocks, and for the wave functions in the
waves 1 .. 3 of a 256-thread block as well as in wave 0.  The inputs sit where a wrong row mask, a dropped tree
level, a signed compare or another summation order shows; NaN results are compared as NaN, not by payload."""
import numpy as np
import pytest

import wave_probe as wp

pytestmark = pytest.mark.gpu

F32, F64, I32, U32, I64 = np.float32, np.float64, np.int32, np.uint32, np.int64
LANE = np.arange(64)


def bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, ref, what, nan_as_nan=False):
    """every element equal in bits (where ref is NaN and nan_as_nan: got is NaN)"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    bad = bits(got) != bits(ref)
    if nan_as_nan:
        bad &= ~(np.isnan(ref) & np.isnan(got))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {at}: got {got[at]!r}, want {ref[at]!r}")


def blocks(waves, nwaves=4):
    """[n][64] (or [n][64][N]) waves -> [n / nwaves][1][nwaves * 64]: consecutive waves share a block"""
    waves = np.asarray(waves)
    n = waves.shape[0]
    assert n % nwaves == 0 and n // nwaves >= 2
    return np.ascontiguousarray(waves.reshape((n // nwaves, 1, nwaves * 64) + waves.shape[2:]))


def one_hot(dtype, value=1):
    """64 waves: `value` in lane k of wave k, zeros elsewhere"""
    return np.eye(64, dtype=dtype) * np.dtype(dtype).type(value)


def spread(base, value):
    """64 waves: the base wave with the special value in lane k, for every k"""
    x = np.tile(base, (64, 1))
    x[LANE, LANE] = value
    return x


# ---------------------------------------------------------------- wave_sum, wave_sum_xor
def sum_waves(dtype, rng):
    """finite inputs of wave_sum<dtype>: [n][64], n a multiple of 4"""
    dt = np.dtype(dtype)
    w = [one_hot(dtype)]
    if dt.kind == "f":
        w += [wp.per_wave(wp.wave_family(dtype)).reshape(-1, 64)]
        w += [np.full((4, 64), -0.0, dtype)]                                   # the sum carries the sign bit
        w += [one_hot(dtype, -1.5)]
    elif dt == np.dtype(U32):
        w += [rng.integers(0, 1 << 32, (8, 64), dtype=U32), np.full((4, 64), 0xFFFFFFFF, U32)]     # wrap past 2^32
    elif dt == np.dtype(I32):
        w += [rng.integers(-(1 << 24), 1 << 24, (8, 64), dtype=I32), -rng.integers(1, 1 << 24, (4, 64), dtype=I32)]
    else:
        w += [rng.integers(-(1 << 56), 1 << 56, (8, 64), dtype=I64), rng.integers(1 << 53, 1 << 56, (4, 64), dtype=I64)]
        w += [one_hot(I64, (1 << 53) + 1)]
    return np.concatenate(w)


@pytest.mark.parametrize("dtype", [I32, U32, F32, I64, F64])
@pytest.mark.parametrize("fn", ["wave_sum", "wave_sum_xor"])
def test_wave_sum(fn, dtype):
    x = sum_waves(dtype, np.random.default_rng(21))
    if np.dtype(dtype).kind == "f":
        t = wp.tree_sum(x[64:72])
        assert (t != wp.seq_sum(x[64:72])).all() and (bits(wp.tree_sum(x[72:76])) >> (8 * x.itemsize - 1) == 1).all()
    for nwaves in (4, 1):
        xb = blocks(x, nwaves)
        got, = wp.run(fn, xb, nwaves=nwaves)
        same(got, wp.wave_sum(xb), f"{fn}<{np.dtype(dtype)}> in blocks of {nwaves} waves")


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("fn", ["wave_sum", "wave_sum_xor"])
def test_wave_sum_of_non_finite_values(fn, dtype):
    rng = np.random.default_rng(22)
    x = rng.standard_normal((8, 64)).astype(dtype)
    x[0, 5] = np.nan                       # one NaN lane: NaN
    x[1, 63] = np.nan
    x[2, 0], x[2, 40] = np.inf, -np.inf    # +inf with -inf: NaN
    x[3, 17], x[3, 33] = -np.inf, np.inf
    x[4, 9] = np.inf                       # +inf alone: +inf
    x[5, 31], x[5, 32] = -np.inf, -np.inf
    x[6, 16] = np.nan
    x[6, 47] = np.inf
    ref = wp.wave_sum(blocks(x))
    assert np.isnan(ref[0, 0, :192]).all() and np.isnan(ref[1, 0, 128:192]).all() and np.isinf(ref[1, 0, :128]).all()
    got, = wp.run(fn, blocks(x), nwaves=4)
    same(got, ref, f"{fn}<{np.dtype(dtype)}>", nan_as_nan=True)


def test_wave_sum_xor_n():
    rng = np.random.default_rng(23)
    x = rng.integers(-(1 << 24), 1 << 24, (8, 64, 3), dtype=I32)
    hot = np.zeros((64, 64, 3), I32)
    hot[LANE, LANE, LANE % 3] = 1 + LANE % 3
    x = blocks(np.concatenate([x, hot]))
    got, = wp.run("wave_sum_xor_n", x, nwaves=4)
    same(got, wp.wave_sum_n(x), "wave_sum_xor<3>(int*)")
    y = wp.xor28_family()
    got, = wp.run("wave_sum_xor_n", y, nwaves=4)
    same(got, wp.wave_sum_n(y), "wave_sum_xor<28>(double*)")


# ---------------------------------------------------------------- wave_max, wave_min
def extreme_waves(fn, dtype, rng):
    """(finite [n][64], with NaN lanes [m][64]) for wave_max / wave_min: no wave mixes +0 and -0 (none holds a zero
    but uint32's)"""
    mx = fn == "wave_max"
    if dtype == F32:
        sign = F32(-1.0 if mx else 1.0)
        # all negative under max, all positive under min: a zero fill would win; the extreme in lane k for every k
        w = [spread(sign * rng.uniform(1.0, 100.0, 64).astype(F32), sign * F32(0.5))]
        w += [(sign * rng.uniform(1.0, 100.0, (4, 64))).astype(F32)]
        w += [spread(rng.standard_normal(64).astype(F32), -sign * F32(50.0))]                       # mixed signs
        inf = rng.standard_normal((4, 64)).astype(F32)
        inf[0, 7], inf[0, 50] = np.inf, -np.inf
        inf[1, 63], inf[2, 0] = -sign * np.inf, -sign * np.inf
        inf[3] = sign * np.inf                                                                           # every lane the identity
        inf[3, 21] = sign * F32(3.0)
        nan = (sign * rng.uniform(1.0, 100.0, (8, 64))).astype(F32)
        nan[0, 0] = nan[1, 63] = nan[2, 15] = nan[3, 16] = nan[4, 32] = np.nan                           # the others' extreme
        nan[5, :63] = np.nan                                                                             # one lane left
        nan[6] = nan[7] = np.nan                                                                         # all NaN: NaN
        return np.concatenate(w + [inf]), nan
    big = rng.integers(1 << 31, (1 << 32) - 64, 64, dtype=U32)
    small = rng.integers(64, 1 << 31, 64, dtype=U32)
    if mx:
        w = [spread(small, U32((1 << 31) + 5))]        # one value with the top bit set: a signed compare loses it
        w += [spread(big, U32(0xFFFFFFFF))]
        w += [spread(np.zeros(64, U32), U32(1))]
    else:
        w = [spread(big, U32((1 << 31) - 5))]          # a signed compare prefers the large ones
        w += [spread(big, U32(1 << 31))]               # all large under min: a zero fill would win
        w += [spread(np.full(64, 0xFFFFFFFF, U32), U32(0xFFFFFFFE))]
    w += [rng.integers(0, 1 << 32, (8, 64), dtype=U32)]
    return np.concatenate(w), None


@pytest.mark.parametrize("dtype", [F32, U32])
@pytest.mark.parametrize("fn", ["wave_max", "wave_min"])
def test_wave_max_min(fn, dtype):
    x, nan = extreme_waves(fn, dtype, np.random.default_rng(24))
    ref_fn = getattr(wp, fn)
    for nwaves in (4, 1):
        xb = blocks(x, nwaves)
        got, = wp.run(fn, xb, nwaves=nwaves)
        same(got, ref_fn(xb), f"{fn}<{np.dtype(dtype)}> in blocks of {nwaves} waves")
    if nan is not None:
        ref = ref_fn(blocks(nan))
        assert not np.isnan(ref[0]).any() and not np.isnan(ref[1, 0, :128]).any() and np.isnan(ref[1, 0, 128:]).all()
        got, = wp.run(fn, blocks(nan), nwaves=4)
        same(got, ref, f"{fn}<float> with NaN lanes", nan_as_nan=True)


# ---------------------------------------------------------------- wave_incl_scan
@pytest.mark.parametrize("dtype", [I32, U32])
def test_wave_incl_scan(dtype):
    rng = np.random.default_rng(25)
    w = [one_hot(dtype), one_hot(dtype, 7)]                                     # the step function at every lane
    if dtype == I32:
        w += [rng.integers(-(1 << 24), 1 << 24, (8, 64), dtype=I32), -rng.integers(1, 1 << 24, (4, 64), dtype=I32)]
        w += [-one_hot(I32)]
    else:
        w += [rng.integers(0, 1 << 32, (8, 64), dtype=U32), np.full((4, 64), 0xFFFFFFFF, U32)]           # wraps
        w += [rng.integers(0, 1 << 20, (8, 64), dtype=U32)]
    x = np.concatenate(w)
    step = wp.wave_incl_scan(x[:64])
    assert all((step[k, :k] == 0).all() and (step[k, k:] == 1).all() for k in range(64))
    for nwaves in (4, 1):
        xb = blocks(x, nwaves)
        got, = wp.run("wave_incl_scan", xb, nwaves=nwaves)
        same(got, wp.wave_incl_scan(xb), f"wave_incl_scan<{np.dtype(dtype)}> in blocks of {nwaves} waves")
        same(wp.per_wave(got)[..., 63], wp.tree_sum(wp.per_wave(xb)), "lane 63 holds the wave's total")


# ---------------------------------------------------------------- wave_rank, match_place
def rank_blocks():
    """[76][1][256]: block j holds the masks j .. j + 3 (cyclic), so every mask runs in each of the four waves"""
    m = wp.rank_masks()
    n = len(m)
    return np.ascontiguousarray(np.stack([np.concatenate([m[(j + w) % n] for w in range(4)]) for j in range(n)])[:, None, :])


def test_wave_rank():
    x = rank_blocks()
    rank, count = wp.run("wave_rank", x, nwaves=4)
    ref_rank, ref_count = wp.wave_rank(x)
    same(rank, ref_rank, "wave_rank")
    same(count, ref_count, "wave_rank's *count")
    one = wp.rank_masks()[:, None, :]
    rank, count = wp.run("wave_rank", one, nwaves=1)
    same(rank, wp.wave_rank(one)[0], "wave_rank in one-wave blocks")
    same(count, wp.wave_rank(one)[1], "wave_rank's *count in one-wave blocks")


def test_match_place():
    m = wp.rank_masks()
    n = len(m)
    x = np.stack([np.stack([np.concatenate([m[(j + 4 * r + w) % n] for w in range(4)]) for r in range(3)]) for j in range(n)])
    rng = np.random.default_rng(26)
    edge = np.zeros((2, 3, 256), I32)
    edge[0, 1] = 1                                                              # no accepted row, all 256, a random tile
    edge[0, 2] = rng.random(256) < 0.5
    edge[1, 0] = edge[1, 2] = 1                                                 # all, none, all
    x = np.ascontiguousarray(np.concatenate([x, edge]).astype(I32))
    pos, base = wp.run("match_place", x, nwaves=4)
    ref_pos, ref_base = wp.match_place(x)
    assert ref_base[n, 0, 0] == 0 and ref_base[n, 1, 0] == 256 and ref_base[n + 1, 2, 255] == 512
    same(pos, ref_pos, "match_place")
    same(base, ref_base, "match_place's base")


# ---------------------------------------------------------------- block_excl_scan and the ladder scans
def scan_blocks(nwaves):
    """[8][3][nwaves * 64] uint32: two blocks each of 0/1 flags, values up to 2^20, a single 1 at a seam (thread 0,
    63, 64, the last; three rounds over different seams) and totals that wrap; every round and block differs"""
    rng = np.random.default_rng(27 + nwaves)
    B = nwaves * 64
    x = np.zeros((8, 3, B), U32)
    x[0:2] = rng.random((2, 3, B)) < 0.5
    x[2:4] = rng.integers(0, (1 << 20) + 1, (2, 3, B), dtype=U32)
    seams = [0, 63, min(64, B - 1), B - 1, B - 1, 0]
    for q, t in enumerate(seams):
        x[4 + q // 3, q % 3, t] = 1
    x[6:8] = rng.integers(0, 1 << 32, (2, 3, B), dtype=U32)
    return x


@pytest.mark.parametrize("nwaves", [1, 2, 3, 4, 8, 15, 16])
def test_block_excl_scan(nwaves):
    x = scan_blocks(nwaves)
    scan, total = wp.run("block_excl_scan", x, nwaves=nwaves)
    ref_scan, ref_total = wp.block_excl_scan(x)
    assert (ref_total[6:8, :, 0].astype(np.uint64) < x[6:8].sum(-1, dtype=np.uint64)).all()              # they did wrap
    same(scan, ref_scan, f"block_excl_scan<{nwaves}>")
    same(total, ref_total, f"block_excl_scan<{nwaves}>'s *total")


def test_block_exscan_1024_is_block_excl_scan_16():
    x = scan_blocks(16)
    scan, total = wp.run("block_exscan_1024", x, nwaves=16)
    ref_scan, ref_total = wp.block_excl_scan(x)
    same(scan, ref_scan, "block_exscan_1024")
    same(total, ref_total, "block_exscan_1024's *total")
    dev_scan, dev_total = wp.run("block_excl_scan", x, nwaves=16)
    same(scan, dev_scan, "block_exscan_1024 against block_excl_scan<16>")
    same(total, dev_total, "block_exscan_1024's *total against block_excl_scan<16>'s")


def test_block_exscan_256_is_block_excl_scan_4():
    x = scan_blocks(4)
    scan, = wp.run("block_exscan_256", x, nwaves=4)
    same(scan, wp.block_excl_scan(x)[0], "block_exscan_256")
    same(scan, wp.run("block_excl_scan", x, nwaves=4)[0], "block_exscan_256 against block_excl_scan<4>")


# ---------------------------------------------------------------- block_sum
@pytest.mark.parametrize("dtype", [I32, U32, F32, F64])
@pytest.mark.parametrize("nwaves", wp.BLOCK_NWAVES)
def test_block_sum(nwaves, dtype):
    """[2][2][nwaves * 64]: two blocks, called twice with the caller's barrier between"""
    rng = np.random.default_rng(28)
    if np.dtype(dtype).kind == "f":
        x = wp.block_family(dtype, nwaves)                                      # order-sensitive (test_wave_ref.py)
    elif dtype == I32:
        x = rng.integers(-(1 << 20), 1 << 20, (2, 2, nwaves * 64), dtype=I32)
    else:
        x = rng.integers(0, 1 << 32, (2, 2, nwaves * 64), dtype=U32)
    got, = wp.run("block_sum", x, nwaves=nwaves)
    same(got, wp.block_sum(x), f"block_sum<{nwaves}, {np.dtype(dtype)}>")


# ---------------------------------------------------------------- the two top-2 merges
def test_top2c_merge_lanes():
    """Values from a set of four, so that the two lanes of a pair hold equal bests with different indices and a
    second equal to a best; the start state (-inf, -1, -inf); and the one input on which `i2 < i` and `i2 <= i`
    differ: equal (value, index) in both lanes with the bits +0 and -0, where a lane keeps its own."""
    rng = np.random.default_rng(29)
    vals = np.array([0.25, 0.5, 0.75, 1.0], F32)
    n = 32
    k = rng.integers(0, 4, (n, 64))
    b = vals[k]
    i = np.stack([rng.permutation(4096)[:64] for _ in range(n)]).astype(I32)
    ks = k - rng.integers(0, 3, (n, 64))                                        # second <= best; below the set: -inf
    s = np.where(ks >= 0, vals[np.maximum(ks, 0)], F32(-np.inf)).astype(F32)
    empty = rng.random((n, 64)) < 0.1
    b[empty], s[empty], i[empty] = -np.inf, -np.inf, -1
    b[n - 1, :32], b[n - 1, 32:] = 0.0, -0.0
    s[n - 1] = -np.inf
    i[n - 1] = np.tile(np.arange(32, dtype=I32), 2)
    b[n - 2, :32], b[n - 2, 32:] = -0.0, 0.0
    s[n - 2], i[n - 2] = s[n - 1], i[n - 1]
    live = ~empty[:, :32] & ~empty[:, 32:]
    assert (live & (b[:, :32] == b[:, 32:]))[:n - 2].sum() > 50 and (live & (s[:, :32] == b[:, 32:]))[:n - 2].sum() > 50
    ins = [blocks(a) for a in (b, i, s)]
    got = wp.run("top2c_merge_lanes", *ins, nwaves=4)
    ref = wp.top2c_merge_lanes(*ins)
    assert (bits(ref[0][-1, 0, 128:]) == bits(ins[0][-1, 0, 128:])).all()                               # a lane keeps its own zero
    for g, r, what in zip(got, ref, ("best", "index", "second")):
        if what == "second":             # min(+0, -0) of the two zero waves is either zero (wave.h: order-free)
            g, r = (np.where(a == 0, F32(0.0), a) for a in (g, r))
        same(g, r, f"top2c_merge_lanes(off = 32): {what}")


def test_top2s_merge_wave():
    """every lane empty; one holder at lane k for every k; 1 .. 63 holders; equal bests at different indices (the
    lowest index wins); the best value twice (second = best); a holder whose best is inf still wins over the
    lanes that hold none.  The result is the same in all 64 lanes."""
    rng = np.random.default_rng(30)
    vals = np.array([0.25, 0.5, 0.75, 1.0, np.inf], F32)
    n = 4 + 64 + 64 + 64 + 4
    b = np.full((n, 64), np.inf, F32)
    s = np.full((n, 64), np.inf, F32)
    i = np.full((n, 64), -1, I32)

    def hold(w, lanes, kb, ks):
        b[w, lanes], s[w, lanes] = vals[kb], vals[ks]
        i[w, lanes] = rng.permutation(5000)[:len(lanes)]

    for k in range(64):                                                          # waves 4 .. 67: one holder at lane k
        hold(4 + k, np.array([k]), rng.integers(0, 4, 1), [4])
    for k in range(64):                                                          # waves 68 .. 131: k holders (0: none)
        lanes = rng.permutation(64)[:k]
        kb = rng.integers(0, 4, k)
        hold(68 + k, lanes, kb, np.minimum(kb + rng.integers(0, 3, k), 4))
    for k in range(64):                                                          # waves 132 .. 195: all hold, few values
        kb = rng.integers(k % 4, 4, 64)
        hold(132 + k, LANE, kb, np.minimum(kb + rng.integers(0, 3, 64), 4))
    for k in range(4):                                                           # waves 196 .. 199: the holder's best is inf
        hold(196 + k, np.array([5 + 17 * k]), [4], [4])
    ins = [blocks(a) for a in (b, i, s)]
    ref = wp.top2s_merge_wave(*ins)
    rb, ri, rs = (wp.per_wave(r).reshape(n, 64)[:, 0] for r in ref)
    assert (ri[:4] == -1).all() and np.isinf(rb[:4]).all() and np.isinf(rs[:4]).all()
    assert (ri[4:68] >= 0).all() and (ri[196:] >= 0).all() and np.isinf(rb[196:]).all()
    assert (rs[132:196] == rb[132:196]).sum() > 40                               # the best value duplicated
    assert ((b[132:196] == rb[132:196, None]).sum(1) > 1).all()                  # ties on the best: lowest index
    got = wp.run("top2s_merge_wave", *ins, nwaves=4)
    for g, r, what in zip(got, ref, ("best", "index", "second")):
        same(g, r, f"top2s_merge_wave: {what}")
        assert (bits(wp.per_wave(g)) == bits(wp.per_wave(g)[..., :1])).all(), f"{what} is not the same in every lane"
