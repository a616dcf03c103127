"""dev tool: bench.py --dump-outputs directories of several runs of two builds, all pairs, every difference relative to the array's own
maximum.  Prints the arrays whose name holds one of the given substrings, then every array that separates the builds (its SMALLEST
parent-this difference exceeds its LARGEST same-build difference).  usage: dump_spread.py SUBSTR,SUBSTR,... PARENT_DIRS THIS_DIRS (comma lists)"""
import itertools
import os
import sys

import numpy as np

pat, pdirs, tdirs = (a.split(",") for a in sys.argv[1:4])
names = sorted(f for f in os.listdir(pdirs[0]) if f.endswith(".npy"))


def rel(a, b, s):
    return float(np.abs(a - b).max()) / s


def line(f, pp, tt, pt):
    return (f"{f[:-4]:60s} parent-parent max {max(pp):.2e} median {np.median(pp):.2e} | this-this max {max(tt):.2e} median {np.median(tt):.2e} | "
            f"parent-this max {max(pt):.2e} median {np.median(pt):.2e} min {min(pt):.2e}")


apart = []
for f in names:
    P = [np.load(os.path.join(d, f)).astype(np.float64).ravel() for d in pdirs]
    T = [np.load(os.path.join(d, f)).astype(np.float64).ravel() for d in tdirs]
    s = max(float(np.abs(P[0]).max()), 1e-300)
    pp = [rel(a, b, s) for a, b in itertools.combinations(P, 2)]
    tt = [rel(a, b, s) for a, b in itertools.combinations(T, 2)]
    pt = [rel(a, b, s) for a in P for b in T]
    if any(k in f for k in pat):
        print(line(f, pp, tt, pt))
    if min(pt) > max(pp + tt):
        apart.append(line(f, pp, tt, pt) + f" | elements {P[0].size}")
print(f"--- arrays that separate the builds over {len(pdirs)} + {len(tdirs)} runs (smallest parent-this > largest same-build difference): {len(apart)} of {len(names)}")
for l in apart:
    print(l)
