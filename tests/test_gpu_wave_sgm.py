"""GPU: the 64-lane shifts of csrc/wave.h (wave_shift_up, wave_shift_down), which k_sgm_paths takes the k +- 1
neighbours of its recurrence with, through the thin kernels of tests/wave_sgm_probe: every lane of every wave equal,
bit for bit, to the NumPy restatements of tests/wave_sgm_probe.py (held to plain loops in test_wave_sgm_ref.py).
Blocks of 1, 2 and 4 waves: a shift must not cross from one wave of a block into the next."""
import numpy as np
import pytest

import wave_sgm_probe as W

pytestmark = pytest.mark.gpu


def _values(dt, nblocks, nwaves, seed):
    rng = np.random.default_rng(seed)
    if dt == np.uint32:
        return rng.integers(0, 1 << 32, (nblocks, nwaves * 64), dtype=np.uint64).astype(np.uint32)
    x = rng.standard_normal((nblocks, nwaves * 64)).astype(np.float32)
    x[0, :4] = [np.inf, -0.0, np.nan, 1e-42]                                   # carried as bits: nothing is computed
    return x


@pytest.mark.parametrize("nwaves", [1, 2, 4])
@pytest.mark.parametrize("dt", [np.uint32, np.float32], ids=["uint32", "float32"])
@pytest.mark.parametrize("fn", ["shift_up", "shift_down"])
def test_shifts_equal_the_restatement(fn, dt, nwaves):
    x = _values(dt, 3, nwaves, 7 + nwaves)
    fill = dt(0x3FFF) if dt == np.uint32 else np.float32(-2.5)
    got = W.run(fn, x, fill, nwaves)
    exp = getattr(W, fn)(x, fill)
    assert got.tobytes() == exp.tobytes()
    # a distinct value in every lane: each lane's source is told apart
    lanes = np.arange(3 * nwaves * 64, dtype=np.uint32).reshape(3, -1).astype(dt)
    assert W.run(fn, lanes, fill, nwaves).tobytes() == getattr(W, fn)(lanes, fill).tobytes()


@pytest.mark.parametrize("nwaves", [1, 4])
def test_the_three_collectives_of_a_path_step(nwaves):
    """wave_min, wave_shift_up and wave_shift_down on one register, as a path step issues them; values in the
    range of L_r with VO_SGM_ABSENT in the idle lanes of a D = 24 walk."""
    rng = np.random.default_rng(3)
    x = rng.integers(0, 318, (5, nwaves * 64)).astype(np.uint32)
    x.reshape(5, nwaves, 64)[:, :, 24:] = 0x3FFF
    m, lo, hi = W.run("min_and_neighbours", x, np.uint32(0x3FFF), nwaves)
    assert m.tobytes() == W.wave_min(x).tobytes()
    assert lo.tobytes() == W.shift_up(x, np.uint32(0x3FFF)).tobytes()
    assert hi.tobytes() == W.shift_down(x, np.uint32(0x3FFF)).tobytes()
