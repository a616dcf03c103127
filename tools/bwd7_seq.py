"""bwd7_seq.py TRACE.csv [nsteps]: the bwd7_kernel / film_silu_bwd launches of a replayed step in start order, mean duration per position."""
import csv, sys, collections, re
rows = list(csv.DictReader(open(sys.argv[1])))
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Grid_Size", r.get("Grid_Size_X", "?")), r.get("Queue_Id", "?")) for r in rows)
marks = [s for s, e, k, g, q in ev if "seed_advance" in k][-n - 1:]
steps = []
for a, b in zip(marks[:-1], marks[1:]):
    seq = [(re.sub(r"\(.*", "", k.replace("void (anonymous namespace)::", ""))[:40], e - s, g, q) for s, e, k, g, q in ev
           if a <= s < b and ("bwd7_kernel" in k or "film_silu_bwd" in k)]
    steps.append(seq)
names = [tuple((k, g) for k, d, g, q in s) for s in steps]
print(f"{len(steps)} steps, {len(steps[0])} launches each; same sequence in every step: {all(x == names[0] for x in names)}")
for i in range(len(steps[0])):
    ds = [s[i][1] for s in steps if len(s) > i and s[i][0] == steps[0][i][0]]
    print(f"{i:3d}  {steps[0][i][0]:40s} grid {steps[0][i][2]:>8s} q {steps[0][i][3]:>3s}  mean {sum(ds) / len(ds) / 1e3:7.1f} us  min {min(ds) / 1e3:7.1f}  max {max(ds) / 1e3:7.1f}")
