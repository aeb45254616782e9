"""Times and accuracy of the pose refinement (vo_set_pose_refinement; k_refine_pose) on the full
per-frame path over the street world rendered along the KITTI-00 trajectory -> profiles/refine_times.txt.
usage: refine_times.py [--out FILE] [--frames 4541] [--batch 256] [--reps 3] [--profile-batches 4]

 1. full-path stereo frames/s (vo_step_submit_dev / vo_step_collect, three batches in flight, 2048
    MSAC hypotheses, frames resident in HBM) with the refinement off and on, alternating, same
    context and build; median of --reps;
 2. per kernel, from vo_kernel_times of a profiled pass over the first --profile-batches batches
    with the refinement on: k_refine_pose beside k_msac, ms per batch;
 3. the refinement's own stats over the sequence (status counts, passes, accepted steps, cost drop);
 4. ATE and PlotOnMap.m's lagged xz error against the rendered trajectory, off and on.
Nothing is tuned to 4: the parameters are vo_default_refine_params."""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vo_amd  # noqa: E402,F401
from r7020e_visual_odometry_amd import vo, street, kitti  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "refine_times.txt"))
    ap.add_argument("--frames", type=int, default=4541)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile-batches", type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "refine_times.py measures on the GPU"
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    dev = torch.device("cuda", 0)
    gt = street.kitti00_gt()
    n = min(a.frames, len(gt))
    P0, P1 = street.kitti00_calib()
    t0 = time.perf_counter()
    wld = street.kitti00_world(device="cuda:0", poses=gt)
    dL = torch.empty((n, street.KITTI_ROWS, street.KITTI_COLS), dtype=torch.uint8, device=dev)
    dR = torch.empty_like(dL)
    street.render_frames(wld, gt, range(n), P0, P1, out=(dL, dR))
    del wld
    torch.cuda.synchronize()
    say(f"pose refinement on the full per-frame path, MI355X, street world along KITTI-00, {n} frames at "
        f"{street.KITTI_ROWS}x{street.KITTI_COLS} (rendered in {time.perf_counter() - t0:.1f} s, not timed), "
        f"{a.batch} frames per submit, 2048 MSAC hypotheses, vo_default_refine_params")
    rp = vo.default_ransac_params()
    rp.max_num_trials = 2048
    ctx = vo.Context(street.KITTI_ROWS, street.KITTI_COLS, a.batch, device=0, calib=vo.calib_from(P0, P1), ransac=rp)
    params = vo.default_refine_params()

    def loop(refine, stop=n, hook=None):
        ctx.reset()
        ctx.set_pose_refinement(params if refine else None)
        torch.cuda.synchronize()
        t = time.perf_counter()
        outs = kitti._pipelined(ctx, kitti.device_batches(dL, dR, a.batch, 0, stop), dev, hook)
        return time.perf_counter() - t, np.concatenate(outs)

    loop(False, min(n, 2 * a.batch))                         # warm-up
    loop(True, min(n, 2 * a.batch))
    ts = {False: [], True: []}
    outs = {}
    for _ in range(a.reps):
        for refine in (False, True):
            t, o = loop(refine)
            ts[refine].append(t)
            outs[refine] = o
    say()
    say(f"1. full path, wall clock of the pipelined loop, median of {a.reps} alternating runs")
    for refine in (False, True):
        med = statistics.median(ts[refine])
        say(f"   refinement {'on ' if refine else 'off'}: {n / med:8.1f} stereo frames/s  ({med * 1e3:.1f} ms; runs "
            + ", ".join(f"{n / t:.0f}" for t in ts[refine]) + ")")
    say(f"   on / off = {statistics.median(ts[False]) / statistics.median(ts[True]):.4f}")

    PB = max(1, min(a.profile_batches, n // a.batch))
    ctx.set_profiling(True)
    loop(True, PB * a.batch)
    kt = ctx.kernel_times()
    ctx.set_profiling(False)
    say()
    say(f"2. kernels of a profiled pass over the first {PB} batches, refinement on (vo_kernel_times; profiling "
        "synchronises every stream at each collect, so these are the kernels' own durations)")
    for name in ("k_refine_pose", "k_msac"):
        ms, calls = kt.get(name, (0.0, 0))
        say(f"   {name:14s} {ms / PB:8.4f} ms per {a.batch}-frame batch  ({calls} launches)")
    say(f"   sum of all kernels {sum(v[0] for v in kt.values()) / PB:.3f} ms per batch")

    stats = []

    def hook(b0, L, done):
        for f in range(len(done[-1])):
            stats.append(ctx.fetch_pose_refinement(f))
    _, o_on = loop(True, n, hook)                            # two batches in flight: the fetch needs the set intact
    assert o_on.tobytes() == outs[True].tobytes(), "the refined run is not reproducible"
    st = np.array(stats)
    ran = st[st["passes"] > 0]
    say()
    say(f"3. the refinement over the sequence: {len(ran)} of {len(st)} frames refined (the others: frame 1, or MSAC failed)")
    names = {0: "CONVERGED", 1: "MAX_ITER", 2: "DAMPING", -1: "DEGENERATE", -3: "TOO_FEW"}
    say("   status: " + ", ".join(f"{names[int(s)]} {int((ran['status'] == s).sum())}" for s in np.unique(ran["status"])))
    say(f"   passes mean {ran['passes'].mean():.2f} max {ran['passes'].max()}, accepted mean {ran['accepted'].mean():.2f}, "
        f"points used mean {ran['n_used'].mean():.0f}")
    say(f"   cost per used point (px^2): initial median {np.median(ran['cost_initial'] / ran['n_used']):.4f}, "
        f"final median {np.median(ran['cost_final'] / ran['n_used']):.4f}")
    say()
    say("4. accuracy against the rendered trajectory (kitti.ate_rmse; kitti.lagged_xz_error, PlotOnMap.m:8-20)")
    for refine in (False, True):
        poses = np.stack([o["pose"] for o in outs[refine]])
        err = kitti.lagged_xz_error(poses, gt[:n])
        say(f"   refinement {'on ' if refine else 'off'}: ATE {kitti.ate_rmse(poses, gt[:n]):.3f} m, lagged xz error mean {err.mean():.3f} m, "
            f"max {err.max():.3f} m, final {err[-1]:.3f} m; frames with status != 0: {int((outs[refine]['status'] != 0).sum())}")
    ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
