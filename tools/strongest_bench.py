#!/usr/bin/env python3
"""strongest_bench.py — what selectStrongest (vo_set_strongest) costs and saves on the batched path.

Workload: `--batch` stereo frames (default 256 at 1242x375; --large: 1920x1080, ~8k keypoints per
image) resident in HBM through vo_sift_match_batch_dev, as bench.py times it (calls back to
back, one synchronise at the end).  For every N of --n (0 = off; give 0 twice for the run-to-run
spread) it prints one JSON line with the step time, the mean detected / selected keypoint and
stereo-match counts, and the per-kernel HIP-event times of a separate profiled pass
(vo_set_profiling; isolated: every call synchronised) of the selection kernels, the keypoint
scan / expansion, k_desc and the match kernels.

`--unique` frames are rendered and repeated to fill the batch (rendering 256 pairs on the host
takes longer than the measurement)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[0, 0, 500, 1000])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--unique", type=int, default=32)
    ap.add_argument("--large", action="store_true", help="1920x1080 pairs (synthetic.large_pairs)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile-steps", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()

    import torch
    import vo_amd  # noqa: F401
    from r7020e_visual_odometry_amd import vo, synthetic as syn
    assert torch.cuda.is_available(), "strongest_bench.py measures on the GPU"
    B, U = args.batch, min(args.unique, args.batch)
    L, R = syn.large_pairs(U, threads=args.threads) if args.large else syn.independent_pairs(U, threads=args.threads)
    rep = -(-B // U)
    d_l = torch.from_numpy(np.concatenate([L] * rep)[:B]).cuda()
    d_r = torch.from_numpy(np.concatenate([R] * rep)[:B]).cuda()
    torch.cuda.synchronize()
    rows, cols = L.shape[1:]
    ctx = vo.Context(rows, cols, B)

    def call(stats):
        return ctx.sift_match_batch_dev(d_l.data_ptr(), d_r.data_ptr(), B, stats=stats)

    for N in args.n:
        ctx.set_strongest(N)
        st = call(True)
        det = np.mean([ctx.fetch_detected_count(i) for i in range(0, 2 * B, max(1, 2 * B // 16))])
        for _ in range(args.warmup):
            call(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call(False)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        ctx.set_profiling(True)
        for _ in range(args.profile_steps):
            call(True)
        kt = ctx.kernel_times()
        ctx.set_profiling(False)
        pick = {k: round(v[0] / args.profile_steps, 4) for k, v in sorted(kt.items())
                if k.startswith(("k_sel", "k_scan_cands", "k_expand", "k_desc", "k_match", "k_orient"))}
        print(json.dumps({"strongest": N, "rows": rows, "cols": cols, "batch": B, "unique_frames": U,
                          "ms_per_step": round(ms, 4), "stereo_frames_per_s": round(B / ms * 1e3, 1),
                          "mean_detected_sampled": float(det),
                          "mean_selected": float(np.mean([s[0] + s[1] for s in st]) / 2),
                          "mean_stereo_matches": float(np.mean([s[2] for s in st])),
                          "flags": int(max(s[3] for s in st)),
                          "isolated_kernel_ms_per_step": pick,
                          "isolated_all_kernels_ms_per_step": round(sum(v[0] for v in kt.values()) / args.profile_steps, 4)}),
              flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
