"""Time per call of disparitySGM (vo_disparity_sgm_batch_dev) and reconstructScene beside the CPU reference on the same
inputs -> profiles/sgm_times.txt (the method is 9g's).
usage: sgm_times.py [--out FILE] [--ranges 64,128] [--batches 1,8] [--reps 3] [--cpu-pairs 1]

Inputs: synthetic's rendered stereo pairs at 376 x 1241 (4 distinct pairs, cycled over a batch), the default
parameters but DisparityRange [0 D].  The kernel figures are the HIP-event times of k_sgm_census, the four
k_sgm_paths launches and k_sgm_select from vo_kernel_times of one profiled call through vo_disparity_sgm_batch_dev
(device images in, device map out), the call figure the host's wall clock around the same call and its
synchronisation; --reps calls, the first dropped, the kept ones printed.  The floor is the traffic of S alone:
one store, three read-modify-writes and one read of 2 * rows * cols * D bytes a pair (8 passes), at the
device's 8 TB/s peak (the rate every fraction of DESIGN.md is taken of); the fraction is floor / the sum of the paths and select kernels.  The
CPU figure is the wall clock per pair of tests/sgm_ref (one thread, the same spec functions) over the first
--cpu-pairs pairs, whose maps are checked by bytes against the device's.  Recorded, not gated."""
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
from r7020e_visual_odometry_amd import vo, synthetic as syn  # noqa: E402
import sgm_ref as R  # noqa: E402

ROWS, COLS, DISTINCT = 376, 1241, 4
HBM_TBS = 8.0
PATHS = ("k_sgm_paths_rows", "k_sgm_paths_cols", "k_sgm_paths_diag", "k_sgm_paths_anti")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sgm_times.txt"))
    ap.add_argument("--ranges", default="64,128")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-pairs", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sgm_times.py measures on the GPU"
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    batches = [int(s) for s in a.batches.split(",")]
    Ls, Rs = syn.independent_pairs(DISTINCT, ROWS, COLS)
    ctx = vo.Context(ROWS, COLS, 1, sift=vo.default_sift_params(64))
    Q = vo.reprojection_matrix(*syn.calib(1.0))
    say(f"disparitySGM / reconstructScene, MI355X, {ROWS} x {COLS}, DisparityRange [0 D], defaults otherwise: ms per call of "
        "vo_disparity_sgm_batch_dev; census = k_sgm_census, rows / cols / diag / anti = the four k_sgm_paths launches (each walks its "
        "paths both ways), select = k_sgm_select (HIP events, vo_kernel_times), call = host wall clock of the same call with its "
        "synchronisation, floor = 8 passes over S (2 * rows * cols * D bytes a pair) at " f"{HBM_TBS} TB/s, fraction = floor / (paths + "
        "select), cpu = tests/sgm_ref per pair on one host thread (maps equal by bytes); "
        f"{a.reps} calls with the first dropped, the kept ones side by side")
    for D in [int(s) for s in a.ranges.split(",")]:
        p = vo.default_sgm_params(disparity_range=(0, D))
        for B in batches:
            L = np.stack([Ls[k % DISTINCT] for k in range(B)])
            Rt = np.stack([Rs[k % DISTINCT] for k in range(B)])
            dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(Rt).cuda()
            dd = torch.zeros((B, ROWS, COLS), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            cols = {k: [] for k in ("census",) + PATHS + ("select", "call")}
            for k in range(a.reps):
                ctx.set_profiling(True)
                t0 = time.perf_counter()
                ctx.disparity_sgm_batch_dev(dl.data_ptr(), dr.data_ptr(), B, dd.data_ptr(), p)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                t = ctx.kernel_times()
                ctx.set_profiling(False)
                if k:
                    cols["census"].append(t["k_sgm_census"][0])
                    for name in PATHS:
                        cols[name].append(t[name][0])
                    cols["select"].append(t["k_sgm_select"][0])
                    cols["call"].append((t1 - t0) * 1e3)
            got = dd.cpu().numpy()
            m = min(B, a.cpu_pairs)
            t0 = time.perf_counter()
            for k in range(m):
                assert R.disparity(L[k], Rt[k], 0, D)["disp"].tobytes() == got[k].tobytes()
            cpu = (time.perf_counter() - t0) * 1e3 / max(m, 1)
            floor_ms = 8 * 2.0 * ROWS * COLS * D * B / (HBM_TBS * 1e12) * 1e3
            bound = [sum(cols[n][i] for n in PATHS) + cols["select"][i] for i in range(len(cols["call"]))]
            fmt = lambda v: "/".join(f"{x:.3f}" for x in v)
            say(f"  D {D:>3}  B {B}: census {fmt(cols['census'])}  rows {fmt(cols[PATHS[0]])}  cols {fmt(cols[PATHS[1]])}  "
                f"diag {fmt(cols[PATHS[2]])}  anti {fmt(cols[PATHS[3]])}  select {fmt(cols['select'])}  call {fmt(cols['call'])}  "
                f"floor {floor_ms:.3f}  fraction {fmt([floor_ms / b for b in bound])}  cpu per pair {cpu:.0f}  "
                f"(reliable {np.isfinite(got[0]).mean():.3f})")
    # reconstructScene: the host entry (copies in and out included) and its kernel
    disp = ctx.disparity_sgm(Ls[0], Rs[0], vo.default_sgm_params(disparity_range=(0, 128)))
    wall, kern = [], []
    for k in range(a.reps):
        ctx.set_profiling(True)
        t0 = time.perf_counter()
        xyz = ctx.reconstruct_scene(disp, Q)
        t1 = time.perf_counter()
        t = ctx.kernel_times()
        ctx.set_profiling(False)
        if k:
            wall.append((t1 - t0) * 1e3)
            kern.append(t["k_reconstruct"][0])
    t0 = time.perf_counter()
    assert R.reconstruct(disp, Q).tobytes() == xyz.tobytes()
    cpu = (time.perf_counter() - t0) * 1e3
    say(f"  reconstructScene, one map: k_reconstruct {'/'.join(f'{x:.3f}' for x in kern)}  call (host map in, host xyz out) "
        f"{'/'.join(f'{x:.3f}' for x in wall)}  cpu {cpu:.1f}")
    ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
