"""Time per call of estimateFundamentalMatrix (vo_est_fundamental / vo_est_fundamental_batch) beside the
CPU reference on the same inputs -> profiles/fund_times.txt (the method is 9g's).
usage: fund_times.py [--out FILE] [--sizes 300,2000] [--batches 1,256] [--outliers 0,0.4] [--reps 3]

Inputs: tests/fund_ref.py's generator (general motion, 0.1 px noise, DistanceThreshold 0.1 px^2, the
other parameters at their defaults); problem f of a batch is the generator's seed f.  The kernel figure
is k_fund_msac's HIP-event time from vo_kernel_times of one profiled call, the call figure the host's
wall clock around the same call (staging copies and synchronisation included); --reps calls, the first
dropped, the kept ones printed.  The CPU figure is the wall clock of tests/fund_ref (one thread, the
same spec functions, without the kernel's chunking: it stops at the slot where the loop stops) over
the batch's problems, one after the other.  The numbers are recorded, not gated."""
import argparse
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
import fund_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fund_times.txt"))
    ap.add_argument("--sizes", default="300,2000")
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--outliers", default="0,0.4")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fund_times.py measures on the GPU"
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    sizes = [int(s) for s in a.sizes.split(",")]
    batches = [int(s) for s in a.batches.split(",")]
    ctx = vo.Context(64, 64, max(batches), sift=vo.default_sift_params(max(max(sizes), 16)))
    say("estimateFundamentalMatrix, MI355X: ms per call; kernel = k_fund_msac (HIP events, vo_kernel_times), call = host wall "
        f"clock of the same call, cpu = tests/fund_ref over the same problems on one host thread; {a.reps} calls with the first "
        "dropped, the kept ones side by side")
    for method, mname in ((R.MSAC, "MSAC"), (R.NORM8, "Norm8Point")):
        for n in sizes:
            for frac in [float(s) for s in a.outliers.split(",")]:
                for B in batches:
                    x1 = np.zeros((B, n, 2), np.float32)
                    x2 = np.zeros((B, n, 2), np.float32)
                    for f in range(B):
                        x1[f], x2[f], _ = R.case(n, "general", 0.1, frac, f)
                    p = vo.default_fund_params(method=method, distance_threshold=0.1)
                    kern, wall, res = [], [], None
                    for k in range(a.reps):
                        ctx.set_profiling(True)
                        t0 = time.perf_counter()
                        res = ctx.est_fundamental_batch(x1, x2, [n] * B, p, key0=0)
                        t1 = time.perf_counter()
                        t = ctx.kernel_times()
                        ctx.set_profiling(False)
                        if k:
                            kern.append(t["k_fund_msac"][0])
                            wall.append((t1 - t0) * 1e3)
                    t0 = time.perf_counter()
                    slots = []
                    for f in range(B):
                        r = R.estimate(x1[f], x2[f], f, method=method, distance_threshold=0.1)
                        slots.append(r["census"]["slots"])
                        assert r["F"].tobytes() == res[1][f].tobytes() and r["status"] == res[0][f]
                    cpu = (time.perf_counter() - t0) * 1e3
                    say(f"  {mname:<10} n {n:>4}  outliers {frac:>4.0%}  B {B:>3}: kernel {'/'.join(f'{x:.3f}' for x in kern)}  "
                        f"call {'/'.join(f'{x:.3f}' for x in wall)}  cpu {cpu:.2f}  (slots replayed: median {int(np.median(slots))}, "
                        f"max {max(slots)}; inliers of problem 0: {int(res[3][0])})")
    ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
