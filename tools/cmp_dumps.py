"""cmp_dumps.py PARENT_A PARENT_B THIS_A THIS_B: bench.py --dump-outputs directories, every array relative to its own maximum."""
import os, sys
import numpy as np
pa, pb, ta, tb = sys.argv[1:5]
names = sorted(f for f in os.listdir(pa) if f.endswith(".npy"))
assert names == sorted(f for f in os.listdir(ta) if f.endswith(".npy")), "array sets differ"
rows = []
for f in names:
    a, b, c, d = (np.load(os.path.join(p, f)).astype(np.float64).ravel() for p in (pa, pb, ta, tb))
    s = max(float(np.abs(a).max()), 1e-300)
    rows.append((f[:-4], float(np.abs(a - b).max()) / s, float(np.abs(a - c).max()) / s, float(np.abs(b - c).max()) / s,
                 float(np.abs(c - d).max()) / s, s, bool(np.isfinite(c).all())))
print(f"{len(rows)} arrays; all finite in this tree: {all(r[6] for r in rows)}")
for n, pp, pt, pt2, tt, s, _ in rows:
    if n == "loss":
        print(f"LOSS {n}: parent_a {np.load(os.path.join(pa, n + '.npy')).ravel()[:4]} parent_b {np.load(os.path.join(pb, n + '.npy')).ravel()[:4]} "
              f"this_a {np.load(os.path.join(ta, n + '.npy')).ravel()[:4]} this_b {np.load(os.path.join(tb, n + '.npy')).ravel()[:4]}")
g = [r for r in rows if r[0] != "loss"]
print(f"gradient arrays: {len(g)}; differing parent-parent: {sum(r[1] > 0 for r in g)}; parent_a-this: {sum(r[2] > 0 for r in g)}; this-this: {sum(r[4] > 0 for r in g)}")
for lab, i in (("parent_a - parent_b", 1), ("parent_a - this_a", 2), ("parent_b - this_a", 3), ("this_a - this_b", 4)):
    w = max(g, key=lambda r: r[i])
    print(f"worst {lab}: {w[i]:.2e} of the array's maximum ({w[0]})")
over = [r for r in g if min(r[2], r[3]) > 2 * max(r[1], r[4])]
print(f"arrays where both parent-this differences exceed twice the larger of parent-parent and this-this: {len(over)}")
for r in sorted(over, key=lambda r: -r[2])[:40]:
    print(f"  {r[0]:70s} pp {r[1]:.2e} tt {r[4]:.2e} pa-t {r[2]:.2e} pb-t {r[3]:.2e}  max {r[5]:.2e}")
print("--- emb / FiLM-path arrays")
for r in g:
    if "emb" in r[0].lower() or "film" in r[0].lower():
        print(f"  {r[0]:70s} pp {r[1]:.2e} tt {r[4]:.2e} pa-t {r[2]:.2e} pb-t {r[3]:.2e}  max {r[5]:.2e}")
print("--- all")
for r in g:
    print(f"  {r[0]:70s} pp {r[1]:.2e} tt {r[4]:.2e} pa-t {r[2]:.2e} pb-t {r[3]:.2e}  max {r[5]:.2e}")
