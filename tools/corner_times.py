"""Time per call of the corner detector (vo_detect_corners_batch) beside the CPU reference on the same inputs ->
profiles/corner_times.txt (the method is 9g's).
usage: corner_times.py [--out FILE] [--filters 5,15] [--batches 1,64] [--strongest 0,1000] [--reps 3] [--cpu-images 1]

Inputs: band-limited noise at KITTI's image size (375 x 1242; 8 distinct images, cycled over a batch), both
methods, MinQuality 0.01, the whole image.  The kernel figures are the HIP-event times of k_corner_metric,
k_corner_count + k_corner_emit and k_corner_rank from vo_kernel_times of one profiled call, the call figure the
host's wall clock around the same call (staging copies, synchronisation and the copies back included); --reps
calls, the first dropped, the kept ones printed.  The CPU figure is the wall clock per image of tests/corner_ref
(one thread, the same spec functions) over the first --cpu-images images of the batch, whose results are checked
by bytes against the device's.  Recorded, not gated."""
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
import corner_ref as R  # noqa: E402

ROWS, COLS, DISTINCT, MAX_KEYPOINTS = 375, 1242, 8, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "corner_times.txt"))
    ap.add_argument("--filters", default="5,15")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--strongest", default="0,1000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-images", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "corner_times.py measures on the GPU"
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    batches = [int(s) for s in a.batches.split(",")]
    distinct = []
    for k in range(DISTINCT):
        g = R._blur(np.random.default_rng(40 + k).standard_normal((ROWS, COLS)), 1.5)
        distinct.append(np.clip(np.rint(128.0 + 40.0 * g / g.std()), 0, 255).astype(np.uint8))
    ctx = vo.Context(ROWS, COLS, (max(batches) + 1) // 2, sift=vo.default_sift_params(MAX_KEYPOINTS))
    say("detectMinEigenFeatures / detectHarrisFeatures, MI355X, 375 x 1242, MinQuality 0.01: ms per call; metric = k_corner_metric, "
        "select = k_corner_count + k_corner_emit, rank = k_corner_rank (HIP events, vo_kernel_times), call = host wall clock of the "
        "same call, cpu = tests/corner_ref per image on one host thread (results equal by bytes); "
        f"{a.reps} calls with the first dropped, the kept ones side by side")
    for method, name in ((vo.VO_CORNER_MINEIG, "MinEigen"), (vo.VO_CORNER_HARRIS, "Harris  ")):
        for f in [int(s) for s in a.filters.split(",")]:
            for strongest in [int(s) for s in a.strongest.split(",")]:
                for B in batches:
                    imgs = np.stack([distinct[k % DISTINCT] for k in range(B)])
                    p = vo.default_corner_params(method=method, filter_size=f, strongest=strongest)
                    met, sel, rank, wall, res = [], [], [], [], None
                    for k in range(a.reps):
                        ctx.set_profiling(True)
                        t0 = time.perf_counter()
                        res = ctx.detect_corners_batch(imgs, p)
                        t1 = time.perf_counter()
                        t = ctx.kernel_times()
                        ctx.set_profiling(False)
                        if k:
                            met.append(t["k_corner_metric"][0])
                            sel.append(t["k_corner_count"][0] + t["k_corner_emit"][0])
                            rank.append(t["k_corner_rank"][0] if strongest else 0.0)
                            wall.append((t1 - t0) * 1e3)
                    m = min(B, a.cpu_images)
                    t0 = time.perf_counter()
                    for k in range(m):
                        r = R.detect(imgs[k], method=method, f=f, strongest=strongest, max_keypoints=MAX_KEYPOINTS)
                        assert res[k][2] == vo.VO_OK and r["loc"].tobytes() == res[k][0].tobytes() and r["metric"].tobytes() == res[k][1].tobytes()
                    cpu = (time.perf_counter() - t0) * 1e3 / m
                    say(f"  {name}  f {f:>2}  strongest {strongest:>4}  B {B:>2}: metric {'/'.join(f'{x:.3f}' for x in met)}  "
                        f"select {'/'.join(f'{x:.3f}' for x in sel)}  rank {'/'.join(f'{x:.3f}' for x in rank)}  "
                        f"call {'/'.join(f'{x:.3f}' for x in wall)}  cpu per image {cpu:.1f}  (corners per image {res[0][3]})")
    ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
