"""dev tool: the kernels of ONE replayed step of a rocprofv3 kernel trace of bench.py in start order -- start within the step, queue id,
duration, name -- to see which call site a row of tools/kernel_hist.py belongs to.  A step begins at its `seed_advance` launch (the
first kernel of every replayed step, as in kernel_hist.py); the step shown is the last complete one, or the k-th before it.
usage: step_order.py TRACE.csv [k]"""
import csv
import re
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
k = int(sys.argv[2]) if len(sys.argv) > 2 else 0
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "")) for r in rows)
marks = [s for s, e, name, q in ev if "seed_advance" in name]
t0, t1 = marks[-2 - k], marks[-1 - k]
for s, e, name, q in ev:
    if t0 <= s < t1:
        name = name.replace("void (anonymous namespace)::", "").replace("(anonymous namespace)::", "").replace("void ", "")
        name = re.sub(r"^_ZN12_GLOBAL__N_1\d\d", "", name)
        print(f"{(s - t0) / 1e3:9.1f} us  q{q:>3}  {(e - s) / 1e3:7.1f} us  {name[:90]}")
