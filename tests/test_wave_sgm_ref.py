"""CPU: the NumPy restatements of tests/wave_sgm_probe.py against plain loops, and the probe's compiler flags against
csrc/Makefile's, so the probe compiles wave.h as libvo.so does."""
import re
from pathlib import Path

import numpy as np

import wave_sgm_probe as W

ROOT = Path(__file__).resolve().parent.parent


def test_restatements_equal_plain_loops():
    x = np.random.default_rng(1).integers(0, 1000, (2, 128)).astype(np.uint32)
    up, down, mn = W.shift_up(x, 77), W.shift_down(x, 77), W.wave_min(x)
    for b in range(2):
        for t in range(128):
            lane, w0 = t % 64, t - t % 64
            assert up[b, t] == (77 if lane == 0 else x[b, t - 1])
            assert down[b, t] == (77 if lane == 63 else x[b, t + 1])
            assert mn[b, t] == min(x[b, w0:w0 + 64])


def test_probe_is_compiled_with_the_librarys_flags():
    def flags(p):
        text = p.read_text().replace("\\\n", " ")
        return re.search(r"^HIPFLAGS\s*=\s*(.*)$", text, flags=re.M).group(1).split()
    lib = [f for f in flags(ROOT / "r7020e-visual-odometry_amd" / "csrc" / "Makefile") if not f.startswith("-I")]
    probe = [f for f in flags(ROOT / "tests" / "wave_sgm_probe" / "Makefile") if not f.startswith("-I")]
    assert lib == probe
