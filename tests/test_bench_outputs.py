"""bench.py's inputs and --dump-outputs (CPU parts; the run itself: test_gpu_bench_plain_run).

The step's inputs are rendered by worker processes and must equal synthetic.independent_pairs
frame for frame; --dump-outputs writes float .npy files of what a caller fetches after the
last timed call, the same sample of frames in every run."""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("vo_bench", ROOT / "bench.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules["vo_bench"] = m                                # render_pairs' workers look their function up by module
    spec.loader.exec_module(m)
    return m


def test_render_pairs_equals_independent_pairs(bench, syn, monkeypatch):
    monkeypatch.setattr(bench, "ROWS", 48)
    monkeypatch.setattr(bench, "COLS", 96)
    L, R = bench.render_pairs(5, 7, 3)                         # chunks of 1, 2, 2 frames
    rL, rR = syn.independent_pairs(5, 48, 96, first=7, px_per_cell=syn.BENCH_PX_PER_CELL)
    assert L.dtype == np.uint8 and L.shape == (5, 48, 96)
    assert np.array_equal(L, rL) and np.array_equal(R, rR)
    L1, R1 = bench.render_pairs(5, 7, 1)
    assert np.array_equal(L1, rL) and np.array_equal(R1, rR)


class _FakeContext:
    """fetch_keypoints / fetch_stereo_pairs of a finished call with seeded contents."""

    def __init__(self, vo, B, n_kp):
        self.vo, self.B, self.n_kp = vo, B, n_kp

    def fetch_keypoints(self, image, descriptors=True):
        rng = np.random.default_rng(image)
        n = self.n_kp + image % 3
        k = np.zeros(n, self.vo.KP_DTYPE)
        for name in k.dtype.names:
            k[name] = rng.integers(0, 100, n)
        return k, (rng.integers(0, 256, (n, 128)).astype(np.uint8) if descriptors else None)

    def fetch_stereo_pairs(self, frame):
        n = 5 + frame % 4
        return np.random.default_rng(1000 + frame).integers(0, self.n_kp, (n, 2)).astype(np.uint32)


def test_dump_outputs_files(bench, vo, tmp_path):
    B = 20
    ctx = _FakeContext(vo, B, 11)
    bench.dump_outputs(ctx, B, tmp_path / "a")
    bench.dump_outputs(ctx, B, tmp_path / "b")
    names = sorted(p.name for p in (tmp_path / "a").glob("*.npy"))
    assert names == ["counts.npy", "descriptors.npy", "keypoints.npy", "sample_frames.npy", "stereo_pairs.npy"]
    d = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert d[n[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(d[n[:-4]], np.load(tmp_path / "b" / n))          # the same sample every time
    assert sum(a.nbytes for a in d.values()) <= bench.DUMP_MAX_BYTES
    sample = d["sample_frames"].astype(int)
    assert len(sample) == bench.DUMP_FRAMES and len(set(sample)) == len(sample) and sample.max() < B
    # counts cover every frame; the sampled frames' rows are there in full, in fetch order
    for f in range(B):
        assert d["counts"][f].tolist() == [11 + (2 * f) % 3, 11 + (2 * f + 1) % 3, 5 + f % 4]
    f = sample[1]
    rows = d["keypoints"][(d["keypoints"][:, 0] == f) & (d["keypoints"][:, 1] == 1)]
    k, desc = ctx.fetch_keypoints(2 * f + 1)
    assert np.array_equal(rows[:, 2:], np.column_stack([k[n].astype(np.float32) for n in k.dtype.names]))
    first = np.flatnonzero((d["keypoints"][:, 0] == f) & (d["keypoints"][:, 1] == 1))[0]
    assert np.array_equal(d["descriptors"][first:first + len(k)], desc.astype(np.float32))
    pr = d["stereo_pairs"][d["stereo_pairs"][:, 0] == f]
    assert np.array_equal(pr[:, 1:], ctx.fetch_stereo_pairs(f).astype(np.float32))
    assert len(d["keypoints"]) == len(d["descriptors"]) == int(d["counts"][sample, :2].sum())


def test_dump_outputs_stays_below_the_size_limit(bench, vo, tmp_path, monkeypatch):
    B = 12
    ctx = _FakeContext(vo, B, 40)
    one_frame = 2 * 41 * (10 + 128) * 4                       # bytes of one frame's keypoints + descriptors, about
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 3 * one_frame)
    bench.dump_outputs(ctx, B, tmp_path)
    total = sum(p.stat().st_size for p in tmp_path.glob("*.npy"))
    assert total <= 3 * one_frame
    assert 1 <= len(np.load(tmp_path / "sample_frames.npy")) < bench.DUMP_FRAMES


@pytest.mark.gpu
def test_gpu_bench_plain_run(tmp_path):
    """A plain run (2 frames per step): exactly --steps timed steps, the contract fields, none of
    the --full figures, and the dump of the last step."""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "2", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["steps"] == 2 and d["timed_runs"]["n"] == 1 and d["timed_runs"]["steps_per_run"] == 2
    assert d["value"] == pytest.approx(2 * 1e3 / d["ms_per_step"])
    for k in ("roofline", "cpu_baseline", "full_path", "large", "h2d"):
        assert k not in d
    counts = np.load(tmp_path / "counts.npy")
    kp = np.load(tmp_path / "keypoints.npy")
    assert counts.shape == (2, 3) and (counts > 0).all()
    assert len(kp) == counts[:, :2].sum() == len(np.load(tmp_path / "descriptors.npy"))
    assert len(np.load(tmp_path / "stereo_pairs.npy")) == counts[:, 2].sum()
    assert d["config"]["mean_stereo_matches"] == pytest.approx(counts[:, 2].mean())
