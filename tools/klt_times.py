"""Time per call of the point tracker (vo_track_points / vo_track_points_batch) beside the CPU reference on
the same inputs -> profiles/klt_times.txt (the method is 9g's).
usage: klt_times.py [--out FILE] [--sizes 300,2000] [--windows 11,31] [--batches 1,64] [--reps 3] [--cpu-pairs 2]

Inputs: tests/klt_ref.py's generator at KITTI's image size (375 x 1242 band-limited noise, the second
image shifted by (3.25, -2.5) px with noise of sd 8; 8 distinct pairs, cycled over a batch), random
interior points, 3 levels, MaxBidirectionalError off and 1 px.  The kernel figures are the HIP-event
times of k_klt_pyr (all launches of the call) and k_klt_track from vo_kernel_times of one profiled call,
the call figure the host's wall clock around the same call (staging copies and synchronisation included);
--reps calls, the first dropped, the kept ones printed.  The CPU figure is the wall clock per pair of
tests/klt_ref (one thread, the same spec functions, pyramid included) over the first --cpu-pairs pairs of
the batch, whose results are checked by bytes against the device's.  Recorded, not gated."""
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
import klt_ref as R  # noqa: E402

ROWS, COLS, DISTINCT = 375, 1242, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "klt_times.txt"))
    ap.add_argument("--sizes", default="300,2000")
    ap.add_argument("--windows", default="11,31")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-pairs", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "klt_times.py measures on the GPU"
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    sizes = [int(s) for s in a.sizes.split(",")]
    batches = [int(s) for s in a.batches.split(",")]
    f = R.field(ROWS, COLS, 31)
    img0 = R.render(f)
    seconds = [R.render(f, R.SHIFT[0], R.SHIFT[1], 8.0, seed=k) for k in range(DISTINCT)]
    ctx = vo.Context(ROWS, COLS, max(batches), sift=vo.default_sift_params(max(max(sizes), 16)))
    say("vision.PointTracker, MI355X, 375 x 1242, 3 levels: ms per call; pyr = k_klt_pyr (both launches), track = k_klt_track "
        "(HIP events, vo_kernel_times), call = host wall clock of the same call, cpu = tests/klt_ref per pair on one host thread "
        f"(results equal by bytes); {a.reps} calls with the first dropped, the kept ones side by side")
    for n in sizes:
        for win in [int(s) for s in a.windows.split(",")]:
            for bidir in (float("inf"), 1.0):
                for B in batches:
                    imgs0 = np.stack([img0] * B)
                    imgs1 = np.stack([seconds[k % DISTINCT] for k in range(B)])
                    sets = [R.interior_points(ROWS, COLS, n, 50 + k, 20.0) for k in range(B)]
                    p = vo.default_klt_params(block_size=(win, win), max_bidirectional_error=bidir)
                    pyr, trk, wall, res = [], [], [], None
                    for k in range(a.reps):
                        ctx.set_profiling(True)
                        t0 = time.perf_counter()
                        res = ctx.track_points_batch(imgs0, imgs1, sets, None, p)
                        t1 = time.perf_counter()
                        t = ctx.kernel_times()
                        ctx.set_profiling(False)
                        if k:
                            pyr.append(t["k_klt_pyr"][0])
                            trk.append(t["k_klt_track"][0])
                            wall.append((t1 - t0) * 1e3)
                    m = min(B, a.cpu_pairs)
                    t0 = time.perf_counter()
                    for k in range(m):
                        r = R.track(imgs0[k], imgs1[k], sets[k], None, levels=3, block=(win, win), max_it=30, max_bidir=bidir)
                        assert r["pts1"].tobytes() == res[k][0].tobytes() and r["info"].tobytes() == res[k][3].tobytes()
                        assert r["scores"].tobytes() == res[k][2].tobytes() and np.array_equal(r["valid"], res[k][1])
                    cpu = (time.perf_counter() - t0) * 1e3 / m
                    it = np.concatenate([x[3]["iterations"] for x in res])
                    valid = np.concatenate([x[1] for x in res])
                    say(f"  n {n:>4}  window {win:>2}  bidir {'off' if bidir == float('inf') else 'on ':<3}  B {B:>2}: "
                        f"pyr {'/'.join(f'{x:.3f}' for x in pyr)}  track {'/'.join(f'{x:.3f}' for x in trk)}  "
                        f"call {'/'.join(f'{x:.3f}' for x in wall)}  cpu per pair {cpu:.1f}  "
                        f"(valid {valid.mean():.1%}, level-0 iterations mean {it.mean():.1f}, max {it.max()})")
    ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
