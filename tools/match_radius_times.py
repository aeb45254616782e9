"""Per-kernel times of matchFeaturesInRadius (vo_match_radius) beside vo_match_ex on the same
descriptors -> profiles/match_radius_times.txt (the method is 9g's).
usage: match_radius_times.py [--out FILE] [--sizes 2048,9472] [--reps 3] [--parent-lib libvo.so] [--noprereject-lib libvo.so]

Inputs: tests/match_radius_ref.py's generator (layout "scalar") at n1 = n2 = n, as generated
("scattered"), with F2 and points2 reordered by (y, x) ("sorted", the order SIFT emits within a
layer), and with F1 and the centres reordered by (y, x) as well ("both sorted": both sets in SIFT
order).  Calls: vo_match_ex and vo_match_radius at r = 20 and r = 1e6, unique 0 and 1.  Every figure
is a kernel's HIP-event time from vo_kernel_times of one profiled call; --reps calls, the first
dropped, the kept ones printed.  --parent-lib: a libvo.so of the parent commit, whose vo_match_ex is
the baseline; --noprereject-lib: this tree built with -DVO_RADIUS_PREREJECT=0."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vo_amd  # noqa: E402,F401
from r7020e_visual_odometry_amd import vo  # noqa: E402
import match_radius_ref as rr  # noqa: E402

F32 = np.float32


def layouts(n):
    F1, F2, P2, Cn, _ = rr.case(n, n, "scalar")
    o2 = np.lexsort((P2[:, 0], P2[:, 1]))
    o1 = np.lexsort((Cn[:, 0], Cn[:, 1]))
    return {"scattered": (F1, F2, P2, Cn), "sorted": (F1, F2[o2], P2[o2], Cn), "both sorted": (F1[o1], F2[o2], P2[o2], Cn[o1])}


def kernel_ms(ctx, f, reps):
    """-> {kernel: [ms of each kept call]}, the call's result"""
    kept, res = {}, None
    for k in range(reps):
        ctx.set_profiling(True)
        res = f()
        t = ctx.kernel_times()
        ctx.set_profiling(False)
        if k:
            for name, v in t.items():
                kept.setdefault(name, []).append(v[0])
    return kept, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "match_radius_times.txt"))
    ap.add_argument("--sizes", default="2048,9472")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--noprereject-lib", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "match_radius_times.py measures on the GPU"
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    builds = [("this tree", vo.Context(64, 64, 1))]
    if a.noprereject_lib:
        builds.append(("no pre-reject", vo.Context(64, 64, 1, lib=vo.load_library(a.noprereject_lib))))
    parent = vo.Context(64, 64, 1, lib=vo.load_library(a.parent_lib)) if a.parent_lib else None
    say("matchFeaturesInRadius beside matchFeatures, MI355X: kernel times in ms (HIP events, vo_kernel_times), one profiled "
        f"call each, {a.reps} calls with the first dropped; the kept calls are printed side by side")
    for n in [int(s) for s in a.sizes.split(",")]:
        for lname, (F1, F2, P2, Cn) in layouts(n).items():
            say()
            say(f"n1 = n2 = {n}, layout {lname}")
            for unique in (0, 1):
                def line(tag, kept, pairs):
                    total = [sum(v[k] for v in kept.values()) for k in range(a.reps - 1)]
                    say(f"  {tag:<44} unique {unique}: " + ", ".join(f"{nm} {'/'.join(f'{x:.4f}' for x in v)}" for nm, v in sorted(kept.items()))
                        + f"; sum {'/'.join(f'{x:.4f}' for x in total)}; {pairs} pairs")
                if parent and lname == "scattered":
                    kept, p = kernel_ms(parent, lambda: parent.match(F1, F2, unique=bool(unique), return_metric=True)[0], a.reps)
                    line("vo_match_ex (parent build)", kept, len(p))
                if lname == "scattered":
                    ctx = builds[0][1]
                    kept, p = kernel_ms(ctx, lambda: ctx.match(F1, F2, unique=bool(unique), return_metric=True)[0], a.reps)
                    line("vo_match_ex (this tree)", kept, len(p))
                for r in (20.0, 1e6):
                    for bname, ctx in builds:
                        kept, p = kernel_ms(ctx, lambda: ctx.match_in_radius(F1, F2, P2, Cn, r, unique=bool(unique)), a.reps)
                        line(f"vo_match_radius r = {r:g} ({bname})", kept, len(p))
            if lname == "sorted":
                pre = rr.prereject(P2, Cn, np.array([20.0], F32))
                say(f"  (r = 20: the forward pass skips {int(pre.sum())} of {pre.size} (32-row block, tile) combinations)")
            if lname == "both sorted":
                pre = rr.prereject(P2, Cn, np.array([20.0], F32))
                say(f"  (r = 20: the forward pass skips {int(pre.sum())} of {pre.size} (32-row block, tile) combinations)")
    for _, c in builds:
        c.close()
    if parent:
        parent.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
