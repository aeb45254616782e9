"""Times of the describe path (vo_describe / vo_describe_batch) beside the detecting entries on the
same inputs -> profiles/describe_times.txt.
usage: describe_times.py [--out FILE] [--batch 256] [--distinct 32] [--reps 7] [--parent-lib libvo.so]

 1. one 375x1242 image: vo_sift_ex against vo_describe at the image's own detections (host buffers,
    wall clock around the synchronous call);
 2. a --batch-pair batch: vo_sift_match_batch_dev (device-resident frames, stats requested, so the
    call synchronises) against vo_describe_batch of the 2 x batch images at their own detections
    (host buffers: the call stages the images, the points and the descriptors);
 3. per kernel, from vo_kernel_times of profiled calls: the descriptor launch at table capacity 127
    (k_desc_pts) against the detecting launch at the pyramid's dcap (k_desc) on the same keypoints,
    and the kernel sums of both paths.
--parent-lib names a libvo.so of the parent commit; its vo_sift_ex and vo_sift_match_batch_dev are
timed in the same process, alternating with this tree's.  The batch's frames are --distinct rendered
pairs repeated (rendering 256 pairs takes longer than every measurement here)."""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vo_amd  # noqa: E402,F401
from r7020e_visual_odometry_amd import vo, synthetic as syn  # noqa: E402

ROWS, COLS = 375, 1242
DETECT = ("k_ext_", "k_seg_", "k_refine", "k_orient", "k_scan_cands", "k_sel_", "k_expand")


def timed(f, reps, warm=2):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return f"{t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f})"


def profiled(ctx, f):
    ctx.set_profiling(True)
    f()
    k = ctx.kernel_times()
    ctx.set_profiling(False)
    return {n: v[0] for n, v in k.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "describe_times.txt"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "describe_times.py measures on the GPU"
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    B, D = a.batch, min(a.distinct, a.batch)
    L, R = syn.independent_pairs(D, px_per_cell=syn.BENCH_PX_PER_CELL, threads=16)
    rep = (B + D - 1) // D
    L, R = np.concatenate([L] * rep)[:B], np.concatenate([R] * rep)[:B]
    parent = vo.load_library(a.parent_lib) if a.parent_lib else None
    say(f"describe path against the detecting entries, MI355X, {ROWS}x{COLS}, default SIFT parameters")
    say(f"wall clock around synchronous calls, median of {a.reps} after 2 warm-up calls"
        + (f"; parent = {Path(a.parent_lib).name} of the parent commit, timed in this process" if parent else ""))
    say()

    # ---- 1. one image ----
    img = L[0]
    ctx = vo.Context(ROWS, COLS, 1)
    kps, desc = ctx.sift(img)
    n = len(kps)
    got = ctx.describe(img, kps)
    assert np.array_equal(got, desc), "describe at the image's own detections differs from sift"
    say(f"1. one image, {n} detections")
    t_sift1 = timed(lambda: ctx.sift(img), a.reps)
    t_desc1 = timed(lambda: ctx.describe(img, kps), a.reps)
    say(f"   vo_sift_ex  (detect + describe)        {fmt(t_sift1)}")
    say(f"   vo_describe (its {n} detections)     {fmt(t_desc1)}")
    if parent:
        pctx = vo.Context(ROWS, COLS, 1, lib=parent)
        say(f"   vo_sift_ex  (parent)                   {fmt(timed(lambda: pctx.sift(img), a.reps))}")
        pctx.close()
    say(f"   ratio vo_describe / vo_sift_ex = {t_desc1[0] / t_sift1[0]:.3f}")
    k_sift = profiled(ctx, lambda: ctx.sift(img))
    k_desc = profiled(ctx, lambda: ctx.describe(img, kps))
    say(f"   kernels (profiled call, ms): sift sum {sum(k_sift.values()):.3f} of which detection stages "
        f"{sum(v for k, v in k_sift.items() if k.startswith(DETECT)):.3f}, k_desc {k_sift.get('k_desc', 0):.3f}; "
        f"describe sum {sum(k_desc.values()):.3f}, k_points {k_desc.get('k_points', 0):.3f}, k_desc_pts {k_desc.get('k_desc_pts', 0):.3f}")
    ctx.close()
    say()

    # ---- 2. a batch ----
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    torch.cuda.synchronize()
    ctx = vo.Context(ROWS, COLS, B)
    ctx.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), B)
    sets = [ctx.fetch_keypoints(i) for i in range(2 * B)]
    counts = np.array([len(s[0]) for s in sets], np.int32)
    stride = int(counts.max())
    pts = np.zeros((2 * B, stride), vo.KP_DTYPE)
    for i, (k, _) in enumerate(sets):
        pts[i, : len(k)] = k
    imgs = np.ascontiguousarray(np.stack([L, R], 1).reshape(2 * B, ROWS, COLS))      # image 2 f + side
    dsc = np.zeros((2 * B, stride, 128), np.uint8)

    def describe_batch():
        ctx._check(ctx.lib.vo_describe_batch(ctx.h, imgs.ctypes.data_as(C.POINTER(C.c_uint8)), COLS, 0, 2 * B,
                                             pts.ctypes.data_as(C.POINTER(vo.Keypoint)), counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                             stride, dsc.ctypes.data_as(C.POINTER(C.c_uint8))))

    def sift_batch(c=ctx):
        c.sift_match_batch_dev(dl.data_ptr(), dr.data_ptr(), B)

    describe_batch()
    for i in (0, 1, 2 * B - 1):
        assert np.array_equal(dsc[i, : counts[i]], sets[i][1]), "describe_batch differs from the batch's own descriptors"
    say(f"2. {B} pairs ({2 * B} images, {int(counts.sum())} keypoints, {int(counts.mean())} per image)")
    t_sb = timed(sift_batch, a.reps)
    t_db = timed(describe_batch, a.reps)
    say(f"   vo_sift_match_batch_dev (device frames, synchronous)   {fmt(t_sb)}")
    say(f"   vo_describe_batch       (host images, points, rows)    {fmt(t_db)}")
    if parent:
        pctx = vo.Context(ROWS, COLS, B, lib=parent)
        say(f"   vo_sift_match_batch_dev (parent)                       {fmt(timed(lambda: sift_batch(pctx), a.reps))}")
        say(f"   vo_sift_match_batch_dev (this tree, again)             {fmt(timed(sift_batch, a.reps))}")
        pctx.close()
    say(f"   ratio vo_describe_batch / vo_sift_match_batch_dev = {t_db[0] / t_sb[0]:.3f}")
    nbytes = imgs.nbytes + int(counts.sum()) * 128 + pts.nbytes
    say(f"   (vo_describe_batch moves {nbytes / 1e6:.0f} MB between pageable host memory and the device inside the call: "
        f"{imgs.nbytes / 1e6:.0f} MB of images in, {int(counts.sum()) * 128 / 1e6:.0f} MB of descriptors out, image by image "
        "where the counts differ; the detecting entry reads frames already on the device and returns counts)")
    k_sift = profiled(ctx, sift_batch)
    k_desc = profiled(ctx, describe_batch)
    say()
    say("3. kernels of one profiled call of each (vo_kernel_times, ms; a profiled synchronous batch runs as one chain)")
    det = sum(v for k, v in k_sift.items() if k.startswith(DETECT))
    say(f"   detecting path: sum {sum(k_sift.values()):.3f}; detection stages {det:.3f}; k_desc (LDS tables at dcap) {k_sift.get('k_desc', 0):.3f}; "
        f"k_match* {sum(v for k, v in k_sift.items() if 'match' in k):.3f}")
    say(f"   describe path : sum {sum(k_desc.values()):.3f}; k_points {k_desc.get('k_points', 0):.3f}; "
        f"k_desc_pts (LDS tables at 127) {k_desc.get('k_desc_pts', 0):.3f}")
    if k_sift.get("k_desc"):
        say(f"   ratio k_desc_pts / k_desc on the same {int(counts.sum())} keypoints = {k_desc.get('k_desc_pts', 0) / k_sift['k_desc']:.3f}")
    for name, k in (("detecting", k_sift), ("describe", k_desc)):
        say(f"   {name}: " + ", ".join(f"{n} {v:.3f}" for n, v in sorted(k.items(), key=lambda x: -x[1])))
    ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
