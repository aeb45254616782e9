"""Time of vo_triangulate_ex with both quality outputs beside vo_triangulate on the same points
-> profiles/tri_quality_times.txt.
usage: tri_quality_times.py [--out FILE] [--n 2000] [--reps 15]

n KITTI-calibrated pairs (tests/geom_ref's kitti_low_disparity fixture, repeated if n > 2000) in a
context of the default capacity, so the call is one chunk.  Wall clock around the synchronous calls
(host buffers: the call stages the quads and copies the results back), and the GPU side from
vo_kernel_times of profiled calls: k_tri_list alone against k_tri_list + k_tri_quality."""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vo_amd  # noqa: E402,F401
from r7020e_visual_odometry_amd import vo  # noqa: E402
import geom_ref as G  # noqa: E402


def timed(f, reps, warm=3):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def kernels(ctx, f, reps):
    """per-call kernel milliseconds of `reps` profiled calls: name -> median"""
    runs = []
    for _ in range(reps):
        ctx.set_profiling(True)
        f()
        runs.append({n: v[0] for n, v in ctx.kernel_times().items()})
        ctx.set_profiling(False)
    return {n: statistics.median(r.get(n, 0.0) for r in runs) for n in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tri_quality_times.txt"))
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tri_quality_times.py measures on the GPU"
    x1, x2, P1, P2 = G.tri_fixtures()["kitti_low_disparity"]
    rep = (a.n + len(x1) - 1) // len(x1)
    x1, x2 = np.concatenate([x1] * rep)[: a.n], np.concatenate([x2] * rep)[: a.n]
    ctx = vo.Context(64, 64, 1)
    X = ctx.triangulate(x1, x2, P1, P2)
    Xq, err, valid = ctx.triangulate(x1, x2, P1, P2, quality=True)
    assert Xq.tobytes() == X.tobytes() and valid.all() and np.isfinite(err).all()
    plain = lambda: ctx.triangulate(x1, x2, P1, P2)
    ex = lambda: ctx.triangulate(x1, x2, P1, P2, quality=True)
    t0, t1 = timed(plain, a.reps), timed(ex, a.reps)
    k0, k1 = kernels(ctx, plain, a.reps), kernels(ctx, ex, a.reps)
    ctx.close()
    fmt = lambda t: f"{t[0]:8.4f} ms  (min {t[1]:.4f}, max {t[2]:.4f})"
    lines = [
        f"vo_triangulate_ex with reprojection errors and validity beside vo_triangulate, MI355X, n = {a.n} pairs, one chunk",
        f"median of {a.reps} synchronous calls after 3 warm-up calls; kernels: vo_kernel_times of {a.reps} profiled calls, median",
        "",
        f"wall clock  vo_triangulate                    {fmt(t0)}",
        f"            vo_triangulate_ex (err + valid)   {fmt(t1)}",
        f"            ratio {t1[0] / t0[0]:.3f}",
        "GPU side    vo_triangulate     " + ", ".join(f"{n} {v * 1e3:.2f} us" for n, v in sorted(k0.items())),
        "            vo_triangulate_ex  " + ", ".join(f"{n} {v * 1e3:.2f} us" for n, v in sorted(k1.items())),
        f"            kernel sums {sum(k0.values()) * 1e3:.2f} us against {sum(k1.values()) * 1e3:.2f} us",
    ]
    print("\n".join(lines), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
