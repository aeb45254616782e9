#!/usr/bin/env python3
"""Scale-space launches of the pipelined SIFT loop from a rocprofv3 kernel trace of bench.py or
tools/prof_run.py: for every launch of a call (identified by kernel name and grid size) its mean
in-situ duration and its mean start after the call's octave-0 base kernel, over the back-to-back
calls (the first two and the last are left out) -- where each chain of the scale space stands in
time, and what its launches cost beside the other streams' (DESIGN.md §9j).
    python3 tools/launch_sequence.py <kernel_trace.csv>"""
import collections
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
qcol = next(c for c in ("Stream_Id", "Queue_Id") if c in rows[0])
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
             r["Kernel_Name"].split("(")[0].replace("void ", "").replace("vo::", ""), r[qcol], int(r["Grid_Size_X"]))
            for r in rows if "vo::" in r["Kernel_Name"])
ss = [e for e in ev if e[2].startswith("k_blur_stream") or e[2].startswith("k_small_pyr")]
occ = collections.defaultdict(list)
for e in ss:
    occ[(e[2], e[4])].append(e)
n = min(len(v) for v in occ.values())
bases = occ[next(k for k in occ if k[0].startswith("k_blur_stream<5, 5"))]
print(f"calls {n}, mean over {n - 3}")
for (name, grid), v in sorted(occ.items(), key=lambda kv: kv[1][3][0] if len(kv[1]) > 3 else 0):
    v = v[2:n - 1]
    dur = sum(e[1] - e[0] for e in v) / len(v) / 1e3
    offs = [(e[0] - max(b[0] for b in bases if b[0] <= e[0])) / 1e3 for e in v]
    print(f"{name:28s} grid {grid:8d} q{v[0][3]} dur {dur:8.1f} us  start+{sum(offs) / len(offs):9.1f}")
